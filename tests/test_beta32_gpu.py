"""The fp32 beta pass of a certified near-identity sweep on the GPU (bb_nid.hip,
k_beta_wb32; bb_set_tuning key 24): beta from the dots the solve's fp64 passes banked plus one
pass over the fp32 copy of X for the solve's last small increment, and X beta from the solve's
n-vectors.  One sweep with the pass on and one with it off from the same state must draw the
same lambda, tau and sig2 bits and the same beta to rounding; a second, free sweep (whose sig2
sees the X beta each route left) must agree as the suite's teacher-forced sweeps do; the counter
must show the path taken exactly where the device's rule certifies it."""
import numpy as np
import pytest

from tests.test_gpu_parity import flips, rel_err

pytestmark = pytest.mark.gpu

SEED = 0xB4E5B41D6E
B32TOL, U32 = 2.0 ** -26, 2.0 ** -24
SCALES = (1e-5, 3e-4, 1e-2)
# (n, p, key 24): n_pad = 128 and fewer columns than waves; a ragged chunk of 8 and a ragged
# wave stride; NR = 15 in the beta kernel; the cost gate itself (key 24 = 1)
SHAPES = [(100, 37, 2), (150, 2003, 2), (1900, 6251, 2), (2000, 6250, 1)]

_problems = {}


def _problem(n, p):
    if (n, p) not in _problems:
        import bench
        X = bench.make_columns(n, 0, p)
        y, btrue = bench.make_problem_y(n, p)
        X.setflags(write=False)
        y.setflags(write=False)
        _problems[(n, p)] = (X, y, btrue)
    return _problems[(n, p)]


def _engine(bb, X, y, n, p):
    # method 2: the dense Woodbury draw whatever the shape (p < n at the smallest)
    e = bb.Engine(bb.EngineConfig(n=n, p=p, seed=SEED, stream=0, true_alpha=0.5,
                                  trace_capacity=1, method=2), X, y)
    e.init_state()
    return e


def _t(e2, k):
    s1 = (1.0 + 0.5 * e2) / (0.5 * e2)
    tm1, tk = 1.0, s1
    for _ in range(1, k):
        tm1, tk = tk, 2.0 * s1 * tk - tm1
    return np.sqrt(1.0 + e2) / tk


def _certified(st, mx):
    """nid_finish's rule for the flag, from the decision the engine reports (no cost gate)."""
    K, k2, eps, eta = st["mode"], mx["k2"], st["eps"], mx["eta"]
    if K < 1:
        return False
    if k2 > 0:
        bound = eta + _t(eps + eta, K) * (1.0 + eta)
    elif K >= 2:
        bound = _t(eps, K) + _t(eps, K - 1)
    else:
        return False
    return bound * (1.0 + 1e-6) <= B32TOL


def _sweep(bb, e, key24, t, state=None):
    old = bb.set_tuning(24, key24)
    try:
        n0 = e.nid_mixed()["beta32_sweeps"]
        if state is not None:
            e.set_state(*state)
        e.run(t, 1)
        e.sync()
        mx = e.nid_mixed()
        return e.state(), e.nid_stats(), mx, mx["beta32_sweeps"] - n0
    finally:
        bb.set_tuning(24, old)


@pytest.mark.parametrize("n,p,key24", SHAPES)
def test_beta32_sweep_equals_fp64_beta_pass(gpu_lib, capsys, n, p, key24):
    """Per shape and state scale (1e-5, 3e-4, 1e-2: the near-null regime, a mixed or K >= 3
    sweep, a sweep past the near-identity regime, which takes the factor): lambda, tau, sig2 bit
    for bit, beta to 1e-12 relative, then a free sweep's sig2 and tau to 1e-11 relative (that
    checks X beta).  The counter shows the pass taken in the first two regimes and not in the
    third, and at every state exactly where the rule, restated from the decision the engine
    reports (eps, K, k2, eta), certifies it.  (The two engines may take different plans: the
    search credits the halved beta pass to the plans that qualify.)"""
    bb = gpu_lib
    X, y, btrue = _problem(n, p)
    rng = np.random.default_rng(11)
    on, off = _engine(bb, X, y, n, p), _engine(bb, X, y, n, p)
    assert on.nid_mixed()["holds_x32"] and off.nid_mixed()["holds_x32"]
    log = []
    try:
        for scale in SCALES:
            state = (btrue * scale + scale * rng.standard_normal(p), scale, 1.0, 0.5)
            a, sa, ma, took = _sweep(bb, on, key24, 3, state)
            o, so, mo, took_off = _sweep(bb, off, 0, 3, state)
            a2, _, _, _ = _sweep(bb, on, key24, 4)
            o2, _, _, _ = _sweep(bb, off, 0, 4)
            err = rel_err(a["beta"], o["beta"])
            d_s2 = abs(a2["sig2"] - o2["sig2"]) / o2["sig2"]
            d_tau = abs(a2["tau"] - o2["tau"]) / o2["tau"]
            log.append((scale, sa["mode"], ma["k2"], f"{sa['eps']:.2e}", took, f"{err:.1e}",
                        f"{d_s2:.1e}", f"{d_tau:.1e}"))
            with capsys.disabled():
                print(f"\n[beta32 {n}x{p}] (scale, K, k2, eps, taken, beta rel, sig2 rel, "
                      f"tau rel) {log[-1]}")
            assert sa["eps"] == so["eps"] and (sa["mode"] > 0) == (so["mode"] > 0)
            assert a["tau"] == o["tau"] and a["sig2"] == o["sig2"]
            assert np.array_equal(a["lambda"], o["lambda"])
            assert err < 1e-12, log[-1]
            assert d_s2 < 1e-11 and d_tau < 1e-11, log[-1]
            assert took_off == 0
            assert took == int(_certified(sa, ma)) and ma["beta32"] == bool(took), log[-1]
            assert took == (0 if scale == SCALES[-1] else 1), log[-1]
            if took:
                assert sa["mode"] >= 2 or ma["k2"] >= 1
        assert on.nid_mixed()["beta32_sweeps"] > 0
        assert off.nid_mixed()["beta32_sweeps"] == 0
        assert on.error_flags() == 0 and off.error_flags() == 0
    finally:
        on.close()
        off.close()


def test_beta32_not_taken_without_certificate_or_x32(gpu_lib):
    """Sweep 1 from the reference start follows the rule (a single iterate banks nothing: never
    taken at K = 1; at this shape the start's eps ~ 1e-9 gives K = 2, and no state of the
    chain reaches the eps < 2^-55 of K = 1, so that refusal rests on the rule's restatement in
    tests/test_beta32_cpu.py); a factor sweep has no solve; an engine created without the fp32
    copy (key 10 = 0) never takes the pass; at a shape below the cost gate the default (key 24
    = 1) does not take it either."""
    bb = gpu_lib
    n, p, _ = SHAPES[1]
    X, y, btrue = _problem(n, p)
    rng = np.random.default_rng(5)
    small = (btrue * 1e-5 + 1e-5 * rng.standard_normal(p), 1e-5, 1.0, 0.5)
    e = _engine(bb, X, y, n, p)
    _, st, mx, took = _sweep(bb, e, 2, 1)           # the reference start, sweep 1
    assert took == int(_certified(st, mx)) and (st["mode"] >= 2 or took == 0), (st, mx)
    _, st, _, took = _sweep(bb, e, 2, 3, (btrue + rng.standard_normal(p), 1.0, 1.0, 0.5))
    assert st["mode"] == 0 and took == 0
    _, st, _, took = _sweep(bb, e, 2, 3, small)
    assert st["mode"] >= 2 and took == 1
    _, st, _, took = _sweep(bb, e, 1, 3, small)     # c64 - c32 < a launch at this shape
    assert st["mode"] >= 1 and took == 0
    assert e.error_flags() == 0
    e.close()
    old = bb.set_tuning(10, 0)
    try:
        e = _engine(bb, X, y, n, p)
    finally:
        bb.set_tuning(10, old)
    assert not e.nid_mixed()["holds_x32"]
    _, st, _, took = _sweep(bb, e, 2, 3, small)
    assert st["mode"] >= 2 and took == 0 and e.nid_stats()["beta32_sweeps"] == 0
    assert e.error_flags() == 0
    e.close()


def test_beta32_teacher_forced_against_oracle(gpu_lib, capsys):
    """Free sweeps at the smallest shape after one through the fp32 beta pass, each
    teacher-forced against the oracle's Cholesky-based Woodbury draw from the engine's own
    state, with test_mixed_plan_teacher_forced_against_oracle's tolerances (beta 1e-10 relative
    L2, lambda / tau / sig2 1e-11, no flips).  Their sig2 is drawn from the X beta the pass's
    n-vector route left, never from a product with beta."""
    from tests.test_steady_state_gpu import oracle_sweep
    bb = gpu_lib
    n, p, _ = SHAPES[0]
    X, y, btrue = _problem(n, p)
    rng = np.random.default_rng(3)
    e = _engine(bb, X, y, n, p)
    beta, tau, sig2 = btrue * 3e-4 + 3e-4 * rng.standard_normal(p), 3e-4, 1.0
    g, _, _, took = _sweep(bb, e, 2, 2, (beta, tau, sig2, 0.5))  # leaves the route's X beta
    assert took == 1
    beta, tau, sig2 = g["beta"], g["tau"], g["sig2"]
    for t in (1001, 1002):
        g, st, mx, took = _sweep(bb, e, 2, t)
        b, lam, tau, sig2 = oracle_sweep(X, y, beta, tau, sig2, 0.5, t, SEED, 0)
        with capsys.disabled():
            print(f"\n[beta32 oracle t={t}] eps={st['eps']:.3g} K={st['mode']} k2={mx['k2']} "
                  f"taken={took} beta rel {rel_err(g['beta'], b):.2e}")
        assert took == 1 or t != 1001, (st, mx)
        assert abs(g["tau"] - tau) / tau < 1e-11 and abs(g["sig2"] - sig2) / sig2 < 1e-11
        assert flips(g["lambda"], lam) == 0
        assert np.max(np.abs(g["lambda"] - lam) / lam) < 1e-11
        assert rel_err(g["beta"], b) < 1e-10
        beta = g["beta"]  # free-running: the engine's own state, its X beta from the n-vectors
    assert e.error_flags() == 0
    e.close()
