"""bench.py end to end on the GPU, as the driver runs it (one JSON line on stdout).

The contract (task statement): metric / value / unit / n_gpus / steps / warmup /
ms_per_step / higher_is_better / scaling / dtype / data / config, plus `roofline` (the
dominant kernel's bound, achieved rate, peak, fraction and how it was timed) and
`cpu_baseline` (the oracle or the compiled reference-literal chain timed on the host).  Small
shapes (C2's n = 1000, p = 5000, and a 300 x 3000 design) keep each run to seconds.

A plain run prints the contract fields only; `roofline`, `cpu_baseline` and the other
measurements that take runs of their own come with `--full`.  `--dump-outputs DIR` writes the
state the last timed sweep left.
"""
import json
import math

import numpy as np
import pytest

from tests.test_bench_cpu import run_bench

pytestmark = pytest.mark.gpu

KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline")


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_c2_line_contract():
    d = _line(run_bench("--workload", "c2", "--steps", "8", "--warmup", "2", "--full",
                        "--no-cpu-baseline", "--no-fitted"))
    for k in KEYS:
        assert k in d, k
    assert d["unit"] == "sweeps/s" and d["n_gpus"] == 1 and d["steps"] == 8
    assert d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] > 0 and math.isclose(d["value"] * d["ms_per_step"], 1000.0, rel_tol=1e-6)
    ro = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "kernel", "timing"):
        assert k in ro, k
    assert ro["peak"] > 0, ro
    # a VALU-bound kernel's rate needs the committed VALU PMC of the workload's shape (C3, C5:
    # profiles/r04_pmc_valu.json); without it achieved and frac are null
    if ro["bound"] == "valu" and ro["achieved"] is None:
        assert ro["frac"] is None, ro
    else:
        assert ro["achieved"] > 0, ro
    assert ro["frac"] is None or 0.0 < ro["frac"] <= 1.0, ro
    assert "HIP events" in ro["timing"]


def test_bench_cpu_baseline_and_timing_stride():
    """A small dense design with a short CPU baseline leg: cpu_baseline carries its value,
    unit, cores, kind and sample; --timing-stride 1 brackets every timed sweep."""
    d = _line(run_bench("--rows", "300", "--cols", "3000", "--steps", "6", "--warmup", "2",
                        "--full", "--cpu-sweeps", "2", "--no-fitted", "--timing-stride", "1"))
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["value"] > 0 and cb["kind"] in ("port", "reference")
    assert d["roofline"]["timing"].endswith("every timed launch")


PLAIN = ("--rows", "300", "--cols", "3000", "--steps", "6", "--warmup", "2")
DUMPED = ("beta", "lambda", "sig2", "tau", "alpha")


def _dump(d):
    return {k: np.load(d / (k + ".npy")) for k in DUMPED}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _line(run_bench(*PLAIN, "--dump-outputs", str(d))), d


def test_plain_run_prints_the_contract_fields_only(plain_run):
    """Without --full: the contract fields, and none of the measurements that take runs of
    their own."""
    d, _ = plain_run
    for k in KEYS:
        if k != "roofline":
            assert k in d, k
    for k in ("roofline", "roofline_secondary", "phases_ms", "cpu_baseline", "cpu_baselines",
              "fitted_regime", "reference_protocol", "parity_check"):
        assert k not in d, k
    assert d["full"] is False and d["steps"] == 6 and d["warmup"] == 2
    assert d["unit"] == "sweeps/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] > 0 and math.isclose(d["value"] * d["ms_per_step"], 1000.0, rel_tol=1e-6)


def test_dump_is_the_state_after_the_timed_sweeps(plain_run, gpu_lib):
    """--dump-outputs holds the state the last timed sweep left: an engine on bench.py's
    design and key run for exactly the --warmup sweeps, the min(--steps, 20) settling sweeps
    and the --steps timed sweeps ends in the same bits (a run is bitwise reproducible,
    DESIGN.md s5), so --steps sets the number of timed sweeps."""
    import bench

    bb = gpu_lib
    _, d = plain_run
    got = _dump(d)
    n, p = 300, 3000
    cfg = bb.EngineConfig(n=n, p=p, p_local=p, true_alpha=0.5, method=2, trace_capacity=6,
                          seed=0xB4E5B41D6E)
    eng = bb.Engine(cfg, bench.make_columns(n, 0, p), bench.make_problem_y(n, p)[0])
    eng.init_state()
    eng.run(1, 2, first_slot=-1)
    eng.run(3, 6, first_slot=-1)
    eng.run(9, 6, first_slot=0)
    eng.sync()
    st = eng.state()
    eng.close()
    for k in DUMPED:
        assert got[k].dtype == np.float64
        assert np.array_equal(got[k], np.atleast_1d(st[k])), k
    assert got["beta"].shape == (p,) and got["lambda"].shape == (p,)
    assert np.all(np.isfinite(got["beta"])) and np.any(got["beta"] != 0)


def test_dump_is_the_same_from_run_to_run(plain_run, tmp_path):
    """Same arguments, same inputs, same outputs: two builds can be compared file by file."""
    _, d = plain_run
    first = _dump(d)
    _line(run_bench(*PLAIN, "--dump-outputs", str(tmp_path)))
    again = _dump(tmp_path)
    for k in DUMPED:
        assert np.array_equal(first[k], again[k]), k


def test_full_run_dumps_what_the_plain_run_dumps(plain_run, tmp_path):
    """A --full run times the same sweeps of the chain and dumps before its further runs
    (fitted regime, reference protocol) move the chain on."""
    _, d = plain_run
    first = _dump(d)
    _line(run_bench(*PLAIN, "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)))
    again = _dump(tmp_path)
    for k in DUMPED:
        assert np.array_equal(first[k], again[k]), k
