"""The fused step with norm='batch' and Config.sync_bn over data-parallel ranks on one MI355X.

Two ranks (gloo, as tests/test_gpu_dp.py) x 1 sample reproduce the reference's own B = 2 run:
the golden step_s32_bn.npz / step_s32_bn_stats.npz is two BatchNorm steps of the reference at
32x32 on two samples, rank r trains on sample r, and with synchronised statistics every rank's
BatchNorm sees the reference's batch -- the G forward, the D forward's [real] and [fake] groups,
the GAN-term pass.  The rules are tests/test_gpu_batchnorm_step.py's, unchanged (digest_check,
running_check, 1e-4 on losses and the G output).  The negative control clears the engines' sync
handle: statistics of one sample per rank must fail running_check.  And at world size 1 over
RCCL with the collectives forced on, the synchronised step is the local one bit for bit.
"""
import datetime
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, pkg
from test_gpu_dp import _free_port

pytestmark = pytest.mark.gpu
WORLD = 2


def _fx():
    d = load_golden("s32_bn")
    d.update(np.load(os.path.join(GOLDEN, "step_s32_bn_stats.npz")))
    return d


def _trainer(fx, dtype, sync_bn, force_reduce=False, deterministic=False):
    """test_gpu_batchnorm_step.make_trainer with Config.sync_bn (and the DP switches)."""
    from oracle import step as O
    from test_gpu_batchnorm_step import LAMBDA_ORDER
    irc = pkg()
    cfg = irc.Config()
    cfg.device = "cuda:0"
    cfg.compute_dtype = dtype
    cfg.norm = "batch"
    cfg.sync_bn = sync_bn
    cfg.deterministic = deterministic
    for k, v in zip(LAMBDA_ORDER, fx["lambdas"]):
        setattr(cfg, k, float(v))
    tr = irc.GANTrainer(cfg, force_reduce=force_reduce)
    G = O.seeded_params(O.g_param_shapes(use_bias=False), 1, bias_std=0.02)
    D = O.seeded_params(O.d_param_shapes(use_bias=False), 2, bias_std=0.02)
    for tag, sd in (("bnG|", G), ("bnD|", D)):
        sd.update({k[len(tag):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(tag)})
    tr.netG.store.load(G)
    tr.netD.store.load(D)
    tr.vgg.store.load(O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True), strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    return tr


def _state(tr):
    out = {"G": tr.netG.store.flat.cpu(), "D": tr.netD.store.flat.cpu()}
    for name, net in (("G", tr.netG), ("D", tr.netD)):
        out.update({f"{name}|{k}": v.cpu() for k, v in net.store.buffers.items()})
    return out


def _checked(fn, *a):
    """A rule's result, or the text of its AssertionError: a rank that raised in the middle of
    the step sequence would leave its peer waiting in a collective."""
    try:
        return float(fn(*a))
    except AssertionError as e:
        return "FAILED: " + str(e)[:300]


def _worker(rank, port, out, local_stats):
    import torch.distributed as dist
    from test_gpu_batchnorm_step import digest_check, running_check
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=60))
    fx = _fx()
    tr = _trainer(fx, "fp32", sync_bn=True)
    core = tr.core
    assert core.gen.bn_sync is not None and core.dis.bn_sync is not None
    if local_stats:   # the negative control: the handle cleared after construction
        core.gen.bn_sync = core.dis.bn_sync = None
    ir, rgb = torch.from_numpy(fx["ir"][rank:rank + 1]).cuda(), torch.from_numpy(fx["rgb"][rank:rank + 1]).cuda()
    res = {}
    for step in (1, 2):
        L = tr.losses(tr.step(ir, rgb))
        torch.cuda.synchronize()
        r = {"L": L, "running": _checked(running_check, tr, fx, step)}
        if step == 1:   # the golden record holds step 1's output, gradients and post-step parameters
            r["fake"] = tr.netG.engine.bufs.d["fake"].permute(0, 3, 1, 2).cpu()
            r["gD"] = _checked(digest_check, tr.netD.store, fx, "gD", 5e-3)
            r["gG"] = _checked(digest_check, tr.netG.store, fx, "gG", 5e-3)
        r["state"] = _state(tr)
        res[step] = r
    torch.save(res, os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _run(tmp_path, local_stats):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(_free_port(), str(tmp_path), local_stats), nprocs=WORLD, join=True)
    return [torch.load(tmp_path / f"r{k}.pt", weights_only=False) for k in range(WORLD)]


def test_two_ranks_of_one_sample_reproduce_the_reference_batch_of_two(tmp_path):
    from test_gpu_batchnorm_step import LOSS_KEYS
    fx = _fx()
    r = _run(tmp_path, local_stats=False)
    for step in (1, 2):
        a, b = r[0][step]["state"], r[1][step]["state"]
        assert a.keys() == b.keys()
        for k in a:   # parameters, running buffers, num_batches_tracked: bit-identical replicas
            assert torch.equal(a[k], b[k]), (step, k)
        for rank in range(WORLD):
            run = r[rank][step]["running"]
            print(f"step {step} rank {rank}: running buffers worst |diff| / bound {run}")
            assert isinstance(run, float), run
    for k in LOSS_KEYS:
        m, ref = sum(x[1]["L"][k] for x in r) / WORLD, float(fx["step1_" + k])
        assert abs(m - ref) <= 1e-4 * max(1.0, abs(ref)), (k, m, ref)
    for k in ("loss_D", "loss_G"):   # step 2 by test_gpu_batchnorm_step's step-2 rule
        m = sum(x[2]["L"][k] for x in r) / WORLD
        ref64, ref32 = float(fx["step2_" + k + "_64"]), float(fx["step2_" + k])
        assert abs(m - ref64) <= max(1e-3 * max(1.0, abs(ref64)), 3 * abs(ref32 - ref64)), (k, m, ref64)
    for rank in range(WORLD):
        s1 = r[rank][1]
        assert np.max(np.abs(s1["fake"].numpy()[0] - fx["fake"][rank])) <= 1e-4, rank
        print(f"rank {rank}: grad worst err / bound D {s1['gD']} G {s1['gG']}")
        assert isinstance(s1["gD"], float) and isinstance(s1["gG"], float), (s1["gD"], s1["gG"])


def test_local_statistics_per_rank_fail_the_running_buffer_rule(tmp_path):
    """The negative control: the same two ranks with the sync handle cleared normalise one sample
    each; running_check must fail after the first step already."""
    r = _run(tmp_path, local_stats=True)
    for rank in range(WORLD):
        run = r[rank][1]["running"]
        assert isinstance(run, str) and run.startswith("FAILED"), ("local statistics passed running_check", run)


def _rccl_worker(rank, store, out, dtype):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1,
                           device_id=torch.device("cuda", 0), timeout=datetime.timedelta(seconds=60))
    fx = _fx()
    res = {}
    for sync in (True, False):
        tr = _trainer(fx, dtype, sync_bn=sync, force_reduce=True, deterministic=True)
        core = tr.core
        assert core.g_reduce.active and (core.gen.bn_sync is not None) == sync == (core.dis.bn_sync is not None)
        assert not sync or core.gen.bn_sync.on_device, "RCCL reduces the fp64 sums on the device"
        g = torch.Generator().manual_seed(5)
        for _ in range(2):
            ir = (torch.rand(2, 1, 64, 64, generator=g) * 2 - 1).cuda()
            rgb = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda()
            tr.step(ir, rgb)
        torch.cuda.synchronize()
        res[sync] = dict(_state(tr), gG=core.G.grad.cpu(), gD=core.D.grad.cpu())
    # without force_reduce (and at world size 1) the option runs the plain local path
    assert _trainer(fx, dtype, sync_bn=True).core.gen.bn_sync is None
    torch.save(res, os.path.join(out, "rccl.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_rccl_world1_synced_step_is_the_local_step_bit_for_bit(tmp_path, dtype):
    """World size 1, collectives forced (RCCL, deterministic mode): the sum over one rank is the
    identity and the finishing halves share the local kernels' arithmetic, so two steps with
    sync_bn equal two steps without -- parameters, gradients, running buffers."""
    import torch.multiprocessing as mp
    mp.spawn(_rccl_worker, args=(str(tmp_path / "store"), str(tmp_path), dtype), nprocs=1, join=True)
    r = torch.load(tmp_path / "rccl.pt", weights_only=True)
    assert r[True].keys() == r[False].keys()
    for k in r[True]:
        assert torch.equal(r[True][k], r[False][k]), k
