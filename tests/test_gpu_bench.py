"""bench.py end to end at a tiny shape (64x64, batch 2, bf16), in this process: a plain run prints
the metric line only and executes exactly --warmup + --steps steps; --dump-outputs writes what
the last timed step left (float32 / float64 .npy, under 64 MB), the same from run to run; --full
adds the roofline entries and checks the default weight-gradient reduction against the
deterministic one that a dumping run takes.

Run-to-run bounds on the dump: the inputs and initial weights are seeded and a dumping run steps
in deterministic mode (no fp32 atomics in the weight gradients), so the generator output and the
parameters are equal bit for bit; the losses are fp64 atomic block sums of at most
2*3*64*64 = 24576 terms, whose order may differ: n * eps = 2.7e-12 relative, held to 1e-11.

Bound on reduction_check: from one state the two reductions differ only in the order and
grouping of the fp32 partial sums of each dW element (n <= 2*64*64 = 8192 positions per tap):
a random-walk error of sqrt(n) * 2^-24 = 5e-6 of the summed magnitudes, times a cancellation
factor (sum|terms| / |sum|) of up to ~100 for a gradient: 5e-4, held to 1e-3 in relative L2."""
import json
import math
import sys

import numpy as np
import pytest

import bench
from conftest import pkg

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--size", "64", "--batch", "2", "--dtype", "bf16", "--steps", "2", "--warmup", "1"]
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(monkeypatch, capsys, extra):
    """bench.main() with ARGS + extra: (the parsed result line, the number of steps executed)."""
    m = pkg()
    calls, step = [], m.GANTrainer.step

    def counted(self, ir, rgb):
        calls.append(1)
        return step(self, ir, rgb)

    monkeypatch.setattr(m.GANTrainer, "step", counted)
    monkeypatch.setattr(sys, "argv", ["bench.py", *ARGS, *extra])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), len(calls)


@pytest.fixture(scope="module")
def param_counts():
    m = pkg()
    count = lambda shapes: sum(math.prod(s) for k, s in shapes.items() if not k.endswith(".filt"))  # noqa: E731
    return count(m.g_param_shapes()), count(m.d_param_shapes())


def test_plain_run_line_and_dumped_outputs(monkeypatch, capsys, tmp_path, param_counts):
    d, steps = run_bench(monkeypatch, capsys, [])
    assert steps == 1 + 2, steps                              # --warmup 1 + --steps 2, nothing after them
    assert d["deterministic"] is False
    runs = []
    for name in ("a", "b"):
        d, steps = run_bench(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / name)])
        assert steps == 1 + 2, steps
        for k in CONTRACT:
            assert k in d, k
        assert d["metric"] == bench.METRIC and d["unit"] == "img/s" and d["higher_is_better"] is True
        assert d["dtype"] == "bf16" and d["steps"] == 2 and d["warmup"] == 1
        assert d["deterministic"] is True
        assert d["ms_per_step"] > 0
        assert "roofline" not in d and "cpu_baseline" not in d and "reduction_check" not in d   # behind --full
        runs.append({p.stem: np.load(p) for p in sorted((tmp_path / name).glob("*.npy"))})
    a, b = runs
    assert sorted(a) == ["fake", "losses", "netD_params", "netG_params"]
    nG, nD = param_counts
    assert a["losses"].dtype == np.float64 and a["losses"].shape == (8,)
    assert a["fake"].dtype == np.float32 and a["fake"].shape == (2 * 64 * 64 * 3,)
    assert np.abs(a["fake"]).max() <= 1.0 and a["fake"].std() > 0          # a tanh output, not a constant
    assert a["netG_params"].dtype == np.float32 and a["netG_params"].shape == (min(nG, bench.DUMP_MAX_ELEMS),)
    assert a["netD_params"].dtype == np.float32 and a["netD_params"].shape == (min(nD, bench.DUMP_MAX_ELEMS),)
    assert sum(v.nbytes for v in a.values()) <= 64e6
    for k, v in a.items():
        assert np.isfinite(v).all(), k
        assert v.shape == b[k].shape, k
    # the line's losses are the dumped vector's (GANStep's slots: 0 loss_D, 1..5 the G terms)
    assert abs(d["losses"]["loss_D"] - b["losses"][0]) <= 1e-5 * max(1.0, abs(b["losses"][0]))
    assert a["losses"][0] != 0 and a["losses"][2] != 0
    print("losses run a", a["losses"], "run b", b["losses"])
    for i in range(6):
        assert abs(a["losses"][i] - b["losses"][i]) <= 1e-11 * max(1.0, abs(a["losses"][i])), (i, a["losses"], b["losses"])
    for k in ("fake", "netG_params", "netD_params"):
        print(k, "run-to-run max diff", np.abs(a[k] - b[k]).max())
        assert np.array_equal(a[k], b[k]), k
    # the dumping run left the process in its default (non-deterministic) mode
    assert pkg().ops.set_deterministic(False) is False


def test_failed_dumping_run_restores_the_default_mode(monkeypatch, capsys, tmp_path):
    m = pkg()

    def broken(self, ir, rgb):
        raise RuntimeError("step failed")

    monkeypatch.setattr(m.GANTrainer, "step", broken)
    monkeypatch.setattr(sys, "argv", ["bench.py", *ARGS, "--dump-outputs", str(tmp_path / "x")])
    with pytest.raises(RuntimeError, match="step failed"):
        bench.main()
    assert m.ops.set_deterministic(False) is False


def test_full_run_adds_the_roofline_and_checks_the_reductions(monkeypatch, capsys):
    d, steps = run_bench(monkeypatch, capsys, ["--full", "--no-cpu-baseline", "--kernel-steps", "1"])
    assert steps == 1 + 2 + 1 + 2, steps                      # + --kernel-steps 1 + reduction_check's two
    for k in CONTRACT:
        assert k in d, k
    assert d["steps"] == 2 and "cpu_baseline" not in d and d["deterministic"] is False
    r = d["roofline"]
    assert r["kernel"] in r["per_kernel"] and r["achieved"] > 0
    assert r["per_kernel"][r["kernel"]]["launches"] > 0
    print("reduction_check", d["reduction_check"])
    for k in ("netG_grad_rel_l2", "netD_grad_rel_l2"):
        assert 0 <= d["reduction_check"][k] <= 1e-3, d["reduction_check"]
    assert pkg().ops.set_deterministic(False) is False
