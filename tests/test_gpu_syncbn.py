"""The SyncBN halves of csrc/batchnorm.hip on the MI355X, in one process: W ranks are emulated
by splitting a case's batch into per-rank local batches (each keeping the group order), running
the local half on each, adding the fp64 buffers with torch (the all-reduce), and running the
finishing half on each.  The reference is the fp64 ``reference(c)`` of the UNION batch of
tests/test_gpu_batchnorm.py, the bounds are that file's ``errors()``: mean, rstd and the running
buffers 1e-5; fp32 y 1e-5, dx / dgamma / dbeta 1e-4; the bf16 bound forms.  dgamma / dbeta stay
out of the collective (the gradient all-reduce takes them): the union value is the SUM of the
per-rank ones.
"""
import pytest
import torch

from conftest import pkg
from test_gpu_batchnorm import CASES, DEV, errors, from_slice, make_case, reference, run_kernels, to_slice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


# case -> per-rank lists of union-batch sample indices (group order kept inside every rank)
SPLITS = {
    "c24_g2": [[0, 2], [1, 3]],      # 2 ranks x (1 real-group + 1 fake-group sample)
    "c8": [[0, 1], [2]],             # unequal shards: the travelling count; HW = 35 < one block's rows
    "c12_scalar": [[0], [1]],        # C % 8 != 0
    "c64_wide": [[0], [1]],          # a slice: ld 96, off 16
    "c16_res_dy2": [[0], [1]],
    "c8_mean100": [[0, 1], [2]],     # mean >> std through the fp64 sums
}


def _sel(t, idx):
    return None if t is None else t[idx]


def run_sync(ops, c, split, repeat=1, G=None, reduce=True, conv_partials=False, rm0=None, rv0=None):
    """The four halves on every emulated rank; everything back on the CPU in union-batch order.
    reduce=False: every rank finishes from its OWN sums (the negative control).
    conv_partials: the forward's local half reads nb float2 partials per image from ``work`` (what a
    fused conv epilogue leaves) instead of x."""
    G = c["G"] if G is None else G
    C, H, W, dt, ld, off, act = c["C"], c["H"], c["W"], c["dt"], c["ld"], c["off"], c["act"]
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    numel = ops.bn_sync_numel(G, C)
    ranks = []
    for idx in split:
        x, dy, dy2, res = (_sel(c[k], idx) for k in ("x", "dy", "dy2", "res"))
        N = len(idx)
        r = dict(idx=idx, N=N, X=ops.Feat(to_slice(x, dt, ld, off), off, C),
                 DY=ops.Feat(to_slice(dy, dt, ld, off), off, C),
                 DY2=ops.Feat(to_slice(dy2, dt, ld, off), off, C) if dy2 is not None else None,
                 RES=ops.Feat(to_slice(res, dt, ld, off), off, C) if res is not None else None,
                 work=torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV),
                 sums=torch.full((numel + 3,), -7.0, dtype=torch.float64, device=DEV),
                 bsums=torch.full((numel + 3,), -7.0, dtype=torch.float64, device=DEV),
                 mr=torch.zeros(N * C * ops.BN_TABLE, device=DEV), ab=torch.zeros(N * C * 2, device=DEV),
                 rm=(c["rm0"] if rm0 is None else rm0).to(DEV), rv=(c["rv0"] if rv0 is None else rv0).to(DEV),
                 dgamma=torch.full((C,), 0.25, device=DEV), dbeta=torch.full((C,), -0.5, device=DEV))
        ranks.append(r)

    def allreduce(key):
        for r in ranks:
            assert bool((r[key][numel:] == -7.0).all()), "the local half wrote past its buffer"
        if reduce:
            total = torch.stack([r[key][:numel] for r in ranks]).sum(0)
            for r in ranks:
                r[key][:numel] = total

    for r in ranks:
        nb = 0
        if conv_partials:   # nb float2 {sum, sum of squares} partials per (n, c): rows of x in nb chunks
            nb = 3
            xs = r["X"].t[..., off:off + C].float().reshape(r["N"], H * W, C)
            part = torch.stack([torch.stack([ch.sum(1), (ch * ch).sum(1)], -1) for ch in xs.chunk(nb, dim=1)], 1)
            assert part.shape == (r["N"], nb, C, 2)
            r["work"].view(torch.float32)[:part.numel()] = part.reshape(-1)
            r["part"] = part
        ops.bn_sync_sums(r["X"], r["work"], r["sums"], G, nb=nb)
    allreduce("sums")
    for r in ranks:
        ops.bn_sync_finalize(r["sums"], r["N"], C, r["mr"], G, gamma, beta, r["rm"], r["rv"], repeat, ab=r["ab"])
        r["y"] = torch.full((r["N"], H, W, ld), 3.0, device=DEV, dtype=dt)
        ops.bn_apply(r["X"], r["mr"], gamma, beta, ops.Feat(r["y"], off, C), act=act, res=r["RES"])
        ops.bn_sync_backward_sums(r["DY"], r["X"], act, r["mr"], gamma, beta, r["work"], r["bsums"],
                                  dgamma=r["dgamma"], dbeta=r["dbeta"], groups=G, dy2=r["DY2"])
    allreduce("bsums")
    for r in ranks:
        r["dx"] = torch.full((r["N"], H, W, ld), 5.0, device=DEV, dtype=dt)
        ops.bn_sync_backward_dx(r["DY"], r["X"], act, r["mr"], gamma, beta, r["bsums"], ops.Feat(r["dx"], off, C),
                                groups=G, dy2=r["DY2"])
    torch.cuda.synchronize()
    NU = sum(r["N"] for r in ranks)
    y, dx = torch.zeros(NU, C, H, W, dtype=torch.float64), torch.zeros(NU, C, H, W, dtype=torch.float64)
    mean, rstd = torch.zeros(NU, C, dtype=torch.float64), torch.zeros(NU, C, dtype=torch.float64)
    for r in ranks:
        for k, fill in (("y", 3.0), ("dx", 5.0)):
            outside = torch.cat([r[k][..., :off].flatten(), r[k][..., off + C:].flatten()])
            assert bool((outside == fill).all()), f"{k}: written outside the channel slice"
        t = r["mr"].view(r["N"], C, ops.BN_TABLE).double().cpu()
        y[r["idx"]], dx[r["idx"]] = from_slice(r["y"], off, C), from_slice(r["dx"], off, C)
        mean[r["idx"]], rstd[r["idx"]] = t[..., 0] + t[..., 2], t[..., 1]
    out = dict(y=y, dx=dx, mean=mean, rstd=rstd, rm=ranks[0]["rm"].double().cpu(), rv=ranks[0]["rv"].double().cpu(),
               dgamma=sum((r["dgamma"] - 0.25).double().cpu() for r in ranks),
               dbeta=sum((r["dbeta"] + 0.5).double().cpu() for r in ranks), ranks=ranks)
    if reduce:   # every rank finished from the same bytes: the same running buffers, bit for bit
        for r in ranks[1:]:
            assert torch.equal(r["rm"], ranks[0]["rm"]) and torch.equal(r["rv"], ranks[0]["rv"])
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(SPLITS))
def test_sync_halves_vs_fp64_union_batch(ops, name, dtype):
    """Check 1, and its negative control (3): finishing every rank from its own unreduced sums
    must fail the same check on mean, rstd and dx."""
    c = make_case(name, dtype)
    ref = reference(c)
    e = errors(c, run_sync(ops, c, SPLITS[name]), ref)
    print(name, dtype, {k: round(v, 4) for k, v in e.items()})
    assert all(v <= 1.0 for v in e.values()), e
    wrong = errors(c, run_sync(ops, c, SPLITS[name], reduce=False), ref)
    print(name, dtype, "unreduced:", {k: round(wrong[k], 1) for k in ("mean", "rstd", "dx")})
    assert wrong["mean"] > 1.0 and wrong["rstd"] > 1.0 and wrong["dx"] > 1.0, ("the local-statistics control passed", wrong)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("repeat", [1, 2])
@pytest.mark.parametrize("name", ["c24_g2", "c64_wide", "c12_scalar", "c8"])
def test_one_rank_is_the_local_path_bit_for_bit(ops, name, dtype, repeat):
    """W = 1: mr, ab, y, dx, the running buffers, dgamma and dbeta of the sync halves against
    ops.bn_stats / ops.bn_backward."""
    c = make_case(name, dtype)
    loc = run_kernels(ops, c, repeat=repeat)
    r = run_sync(ops, c, [list(range(c["N"]))], repeat=repeat)["ranks"][0]
    assert torch.equal(r["mr"], loc["mr_raw"]), "mr"
    assert torch.equal(r["ab"].view(c["N"], c["C"], 2).cpu(), loc["ab"]), "ab"
    assert torch.equal(r["y"], loc["y_raw"]) and torch.equal(r["dx"], loc["dx_raw"])
    assert torch.equal(r["rm"].double().cpu(), loc["rm"]) and torch.equal(r["rv"].double().cpu(), loc["rv"])
    assert torch.equal((r["dgamma"] - 0.25).double().cpu(), loc["dgamma"])
    assert torch.equal((r["dbeta"] + 0.5).double().cpu(), loc["dbeta"])


@pytest.mark.parametrize("name", ["c24_g2", "c64_wide"])
def test_one_rank_from_conv_epilogue_partials_is_bn_finalize(ops, name):
    """W = 1 with nb > 0: the local half sums the float2 partials a fused conv epilogue left in
    ``work``; finished, it is ops.bn_stats(..., nb=nb) on the same partials, bit for bit."""
    c = make_case(name, "fp32")
    N, C = c["N"], c["C"]
    r = run_sync(ops, c, [list(range(N))], repeat=2, conv_partials=True)["ranks"][0]
    gamma, beta, rm, rv = (c[k].to(DEV) for k in ("gamma", "beta", "rm0", "rv0"))
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    work.view(torch.float32)[:r["part"].numel()] = r["part"].reshape(-1)
    mr, ab = torch.zeros(N * C * ops.BN_TABLE, device=DEV), torch.zeros(N * C * 2, device=DEV)
    ops.bn_stats(r["X"], work, mr, c["G"], gamma, beta, rm, rv, 2, ab=ab, nb=r["part"].shape[1])
    assert torch.equal(r["mr"], mr) and torch.equal(r["ab"], ab)
    assert torch.equal(r["rm"], rm) and torch.equal(r["rv"], rv)
    # and the partials were what was read: the statistics are x's (fp32 partial sums: 1e-5)
    ref = reference(c, repeat=2)
    t = mr.view(N, C, ops.BN_TABLE).double().cpu()
    ng = N // c["G"]
    assert float(((t[..., 0] + t[..., 2]) - ref["mean"].repeat_interleave(ng, 0)).abs().max()) <= 1e-5
    assert float((t[..., 1] / ref["rstd"].repeat_interleave(ng, 0) - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_group_order_of_the_running_buffers_under_sync(ops, dtype):
    """G = 2 synchronised over two ranks is two G = 1 synchronised calls in order (the second
    starting from the first one's running buffers): tables, y, dx bit for bit, the running
    buffers as the two calls in order -- tests/test_gpu_batchnorm.py::test_group_property."""
    c = make_case("c24_g2", dtype)
    split = SPLITS["c24_g2"]
    both = run_sync(ops, c, split, G=2)
    h = c["N"] // 2
    halves = []
    for i in (0, 1):
        ci = dict(c)
        for k in ("x", "dy"):
            ci[k] = c[k][i * h:(i + 1) * h]
        ci.update(N=h, G=1)
        rm0, rv0 = (halves[0]["rm"].float(), halves[0]["rv"].float()) if i else (None, None)
        halves.append(run_sync(ops, ci, [[0], [1]], G=1, rm0=rm0, rv0=rv0))
    for k in ("y", "dx", "mean", "rstd"):
        assert torch.equal(both[k], torch.cat([halves[0][k], halves[1][k]])), k
    assert torch.equal(both["rm"], halves[1]["rm"]) and torch.equal(both["rv"], halves[1]["rv"])
    assert not torch.equal(both["rm"], halves[0]["rm"])
