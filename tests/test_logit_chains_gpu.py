"""GPU tests of the logistic chain batch (bb_logit_chain.hip k_logit_chains; .C
bridge_reg_logit_chains and its summary call; ChainBatch(method=6)) against the oracle
(oracle/gibbs.py logit_sweep / bridge_regression_logit) on the same Philox counters.

The batch sums X'Omega X in its own order, so it agrees with the oracle, and with the general
path, up to roundoff and not bit for bit.  Two CPU implementations with different summation
orders (the numpy oracle and oracle.cpu_logit_chain) agree over these runs (nsamp = 120 after
burn = 40) within 1.1e-11 elementwise on beta, 1.4e-14 on tau and 1e-15 on the posterior mean,
so the whole-chain bars below (those of tests/test_logit_gpu.py::test_logit_c_entry_point_chain)
leave reordering five orders of magnitude: a miss is a bug, not roundoff.  What must be bit for
bit is a chain against itself: at another K, beside a forced or a lost neighbour, through a
wrapped ring.
"""
import time

import numpy as np
import pytest

from oracle import gibbs
from tests.test_gpu_parity import flips, rel_err
from tests.test_logit_gpu import SEED, logit_problem

pytestmark = pytest.mark.gpu

_cache = {}


def problem(n, p):
    if (n, p) not in _cache:
        _cache[n, p] = logit_problem(n, p, n + p)[:2]
    return _cache[n, p]


def oracle_chain(n, p, nsamp, burn, seed, stream, **kw):
    """gibbs.bridge_regression_logit of problem(n, p), computed once per key and left unchanged."""
    key = (n, p, nsamp, burn, seed, stream, tuple(sorted(kw.items())))
    if key not in _cache:
        X, y = problem(n, p)
        o = gibbs.bridge_regression_logit(y, X, nsamp, burn=burn, seed=seed, stream=stream, **kw)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = o
    return _cache[key]


def assert_batch(bb, n, p, K, **cfg):
    """tests/test_posterior_law_gpu.py assert_batch_kernel's rule: the .C call runs the chains
    one after another where the batch refuses the design, so a ChainBatch of the design must
    exist, hold K chains and have a resident kernel."""
    X, y = problem(n, p)
    b = bb.ChainBatch(bb.EngineConfig(n=n, p=p, method=6, seed=SEED, **cfg), K, X, y)
    try:
        assert b.nchains == K and b.resident_per_cu() >= 1
        assert b.threads() == 512
    finally:
        b.close()


def same_bits(a, b, what, keys=("beta", "lambda", "tau", "alpha")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# ---------------------------------------------------------------------------------------
# 1. whole chains against the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,kw", [
    (50, 5, {}), (80, 13, {}), (100, 20, {}), (150, 32, {}), (1200, 8, {}), (3000, 8, {}),
    (100, 13, dict(tau_true=0.7)),
], ids=["50x5", "80x13", "100x20", "150x32", "1200x8", "3000x8", "100x13_tau_known"])
def test_whole_chains_match_oracle(gpu_lib, n, p, kw):
    """161 sweeps: across the 32-sweep look-ahead refill and the 50-sweep launch block."""
    bb = gpu_lib
    X, y = problem(n, p)
    K, M, B = 2, 120, 40
    seed = SEED + 71
    assert_batch(bb, n, p, K, true_tau=kw.get("tau_true", 0.0))
    bb.set_rng_state(seed, 0)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=M, nchains=K, burn=B, **kw)
    assert bb.get_rng_state() == (seed, K)
    assert g["beta"].shape == (K, M, p) and g["tau"].shape == (K, M)
    for c in range(K):
        o = oracle_chain(n, p, M, B, seed, c, true_tau=kw.get("tau_true", 0.0))
        d_tau = np.max(np.abs(g["tau"][c] - o["tau"]) / o["tau"])
        d_beta = np.max(np.abs(g["beta"][c].T - o["beta"]) / np.maximum(np.abs(o["beta"]), 1e-8))
        d_mean = rel_err(g["beta"][c].mean(axis=0), o["beta"].mean(axis=1))
        print(f"{n}x{p} chain {c}: tau {d_tau:.2e}, beta {d_beta:.2e}, mean {d_mean:.2e}")
        assert d_tau < 1e-8
        assert np.all(g["alpha"][c] == 0.5)
        assert d_beta < 1e-6
        assert d_mean < 1e-8
        assert flips(g["lambda"][c].T, o["lambda"]) == 0


# ---------------------------------------------------------------------------------------
# 2. alpha sampled
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(80, 13), (150, 32)])
def test_alpha_sampled_matches_oracle(gpu_lib, n, p):
    bb = gpu_lib
    X, y = problem(n, p)
    K, M, B = 2, 120, 40
    seed = SEED + 72
    kw = dict(alpha=0.0, alpha_a=2.0, alpha_b=3.0)
    assert_batch(bb, n, p, K, true_alpha=0.0, alpha_a=2.0, alpha_b=3.0)
    bb.set_rng_state(seed, 0)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=M, nchains=K, burn=B, **kw)
    for c in range(K):
        o = oracle_chain(n, p, M, B, seed, c, **kw)
        d_alpha = np.max(np.abs(g["alpha"][c] - o["alpha"]))
        d_mean = rel_err(g["beta"][c].mean(axis=0), o["beta"].mean(axis=1))
        print(f"{n}x{p} chain {c}: alpha {d_alpha:.2e}, mean {d_mean:.2e}")
        assert d_alpha < 1e-9
        assert d_mean < 1e-8
    # the MH step is exercised both ways: the oracle's trace of stream 1 moves and stays
    a = oracle_chain(n, p, M, B, seed, 1, **kw)["alpha"]
    moved = int(np.sum(np.diff(a) != 0))
    stayed = int(np.sum(np.diff(a) == 0))
    print(f"{n}x{p}: {moved} accepted, {stayed} rejected proposals in the oracle's trace")
    assert moved >= 10 and stayed >= 10


# ---------------------------------------------------------------------------------------
# 3. teacher-forced single sweeps
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(100, 13), (150, 32)])
def test_teacher_forced_sweeps(gpu_lib, n, p):
    bb = gpu_lib
    X, y = problem(n, p)
    seed, s0 = SEED + 73, 4
    o = gibbs.bridge_regression_logit(y, X, 6, burn=0, seed=seed, stream=s0 + 1,
                                      record_state=True)
    st = o["states"]
    assert len(st) == 6
    b = bb.ChainBatch(bb.EngineConfig(n=n, p=p, method=6, seed=seed, stream=s0), 3, X, y)
    free = bb.ChainBatch(bb.EngineConfig(n=n, p=p, method=6, seed=seed, stream=s0), 3, X, y)
    e = bb.Engine(bb.EngineConfig(n=n, p=p, method=6, seed=seed, stream=s0 + 1), X, y)
    assert b.resident_per_cu() >= 1
    for q in (b, free, e):
        q.init_state()
    for k in range(1, len(st)):
        t, tau, lam, om, beta, _ = st[k]
        _, tau0, _, _, beta0, alpha0 = st[k - 1]
        b.set_state(1, beta0, tau0, 1.0, alpha0)
        e.set_state(beta0, tau0, 1.0, alpha0)
        for q in (b, free, e):
            q.run(t, 1, first_slot=-1)
        s, se = b.state(1), e.state()
        og, oe = b.omega(1), e.omega()
        for what, ref_tau, ref_lam, ref_om, ref_beta in (("oracle", tau, lam, om, beta),
                                                        ("engine", se["tau"], se["lambda"], oe,
                                                         se["beta"])):
            assert abs(s["tau"] - ref_tau) <= 1e-12 * ref_tau, (what, t)
            assert flips(s["lambda"], ref_lam) == 0, (what, t)
            assert np.max(np.abs(s["lambda"] - ref_lam) / ref_lam) < 1e-11, (what, t)
            assert np.max(np.abs(og - ref_om) / ref_om) < 1e-11, (what, t)
            assert rel_err(s["beta"], ref_beta) < 1e-10, (what, t, rel_err(s["beta"], ref_beta))
        assert s["sig2"] == 1.0
        for c in (0, 2):  # the forced chain's neighbours do not notice
            sc, sf = b.state(c), free.state(c)
            for key in ("beta", "lambda", "tau", "alpha"):
                assert np.array_equal(sc[key], sf[key]), (c, key, t)
            assert np.array_equal(b.omega(c), free.omega(c)), (c, t)
    for c in range(3):
        assert b.error_flags(c) == 0
    assert e.error_flags() == 0
    for q in (b, free, e):
        q.close()


# ---------------------------------------------------------------------------------------
# 4. a chain does not depend on K
# ---------------------------------------------------------------------------------------
def single_chain(bb, y, X, seed, c, **kw):
    bb.set_rng_state(seed, c)
    g = bb.bridge_reg_logit_chains(y, X, nchains=1, **kw)
    assert bb.get_rng_state() == (seed, c + 1)
    return {k: g[k][0] for k in ("beta", "lambda", "tau", "alpha")}


@pytest.mark.parametrize("kw", [{}, dict(alpha=0.0, alpha_a=2.0, alpha_b=3.0)],
                         ids=["alpha_known", "alpha_sampled"])
def test_chain_is_bitwise_the_same_at_any_k(gpu_lib, kw):
    bb = gpu_lib
    n, p, K = 80, 13, 3
    X, y = problem(n, p)
    seed = SEED + 74
    run = dict(nsamp=60, burn=45, **kw)
    bb.set_rng_state(seed, 0)
    g = bb.bridge_reg_logit_chains(y, X, nchains=K, **run)
    assert bb.get_rng_state() == (seed, K)
    for c in range(K):
        one = single_chain(bb, y, X, seed, c, **run)
        same_bits({k: g[k][c] for k in one}, one, f"chain {c} of {K}")
    if kw:
        assert len(np.unique(g["alpha"])) > K


def test_more_chains_than_the_device_holds(gpu_lib):
    bb = gpu_lib
    n, p = 50, 5
    X, y = problem(n, p)
    b = bb.ChainBatch(bb.EngineConfig(n=n, p=p, method=6), 1, X, y)
    K = b.resident_per_cu() * bb.compute_units() + 4
    b.close()
    assert K > 4
    seed = SEED + 75
    run = dict(nsamp=10, burn=5)
    bb.set_rng_state(seed, 0)
    g = bb.bridge_reg_logit_chains(y, X, nchains=K, **run)
    assert bb.get_rng_state() == (seed, K)
    for k in ("beta", "lambda", "tau", "alpha"):
        assert np.all(np.isfinite(g[k])), k
    for c in (0, 1, K - 5, K - 4, K - 1):
        one = single_chain(bb, y, X, seed, c, **run)
        same_bits({k: g[k][c] for k in one}, one, f"chain {c} of {K}")


# ---------------------------------------------------------------------------------------
# 5. a lost chain leaves at once and alone
# ---------------------------------------------------------------------------------------
def test_lost_chain_is_isolated(gpu_lib):
    """Chain 2's beta is NaN: psi is NaN, and PG(1, NaN) would walk 1000 x 1000 attempts per
    row.  The guard gives NaN and error bit 32 at once; the other chains do not notice."""
    bb = gpu_lib
    n, p, K = 100, 13, 4
    X, y = problem(n, p)
    cfg = bb.EngineConfig(n=n, p=p, method=6, seed=SEED + 76)
    b, free = bb.ChainBatch(cfg, K, X, y), bb.ChainBatch(cfg, K, X, y)
    for q in (b, free):
        q.init_state()
    free.run(1, 1, first_slot=-1)
    free.sync()
    b.set_state(2, np.full(p, np.nan), b.state(2)["tau"], 1.0, 0.5)
    t0 = time.perf_counter()
    b.run(1, 1, first_slot=-1)
    b.sync()
    dt = time.perf_counter() - t0
    print(f"one sweep with a lost chain: {dt * 1e3:.2f} ms")
    # a sweep is microseconds; 100 rows x 10^6 attempts of the unguarded draw are seconds
    assert dt < 1.0
    f = b.error_flags(2)
    assert f & 32 and f & 2, f
    assert not np.any(np.isfinite(b.omega(2)))
    for c in (0, 1, 3):
        assert b.error_flags(c) == 0 and free.error_flags(c) == 0
        sc, sf = b.state(c), free.state(c)
        for key in ("beta", "lambda", "tau", "alpha"):
            assert np.array_equal(sc[key], sf[key]), (c, key)
        assert np.all(np.isfinite(sc["beta"]))
        assert np.array_equal(b.omega(c), free.omega(c)), c
    b.close()
    free.close()


# ---------------------------------------------------------------------------------------
# 6. ring wrap, 7. the sequential path, 8. the summary call
# ---------------------------------------------------------------------------------------
def test_ring_wrap_equals_unwrapped(gpu_lib):
    bb = gpu_lib
    n, p, K, nsamp = 100, 13, 4, 120
    X, y = problem(n, p)
    bb.set_rng_state(SEED + 77, 0)
    whole = bb.bridge_reg_logit_chains(y, X, nsamp=nsamp, nchains=K, burn=40)
    assert bb.last_call_info()["trace_capacity"] == nsamp
    per_slot = 2 * p * 8 + 3 * 8
    try:
        bb.set_trace_budget(K * 37 * per_slot)
        bb.set_rng_state(SEED + 77, 0)
        wrapped = bb.bridge_reg_logit_chains(y, X, nsamp=nsamp, nchains=K, burn=40)
        assert bb.last_call_info()["trace_capacity"] == 37
    finally:
        bb.set_trace_budget(0)
    same_bits(wrapped, whole, "capacity 37")


def test_refused_design_runs_chain_after_chain(gpu_lib):
    """p = 40 > 32: the two chains are two bridge_reg_logit calls on streams 0 and 1."""
    bb = gpu_lib
    X, y = problem(60, 40)
    with pytest.raises(RuntimeError, match="p <= 32"):
        bb.ChainBatch(bb.EngineConfig(n=60, p=40, method=6), 2, X, y)
    bb.set_rng_state(SEED + 78, 0)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=12, nchains=2, burn=6)
    assert bb.get_rng_state() == (SEED + 78, 2)
    bb.set_rng_state(SEED + 78, 0)
    for c in range(2):
        one = bb.bridge_reg_logit(y, X, nsamp=12, burn=6)
        same_bits({k: g[k][c] for k in ("beta", "lambda", "tau", "alpha")}, one, f"chain {c}")


def test_summary_call_matches_trace_call(gpu_lib):
    from tests.test_summary_gpu import check_against_trace_call

    bb = gpu_lib
    n, p, K = 100, 13, 3
    X, y = problem(n, p)
    assert_batch(bb, n, p, K)
    bb.set_rng_state(SEED + 79, 0)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=120, nchains=K, burn=60)
    bb.set_rng_state(SEED + 79, 0)
    s = bb.bridge_reg_logit_chains_summary(y, X, nsamp=120, nchains=K, burn=60)
    assert bb.get_rng_state() == (SEED + 79, K)
    g = dict(g, sig2=np.ones_like(g["tau"]))
    check_against_trace_call(bb, s, g, K, f"logit {n}x{p}")
    assert np.all(s["chain_mean"][:, p] == 1.0) and np.all(s["chain_var"][:, p] == 0.0)
    assert np.all(s["chain_mean"][:, p + 2] == 0.5) and np.all(s["chain_var"][:, p + 2] == 0.0)
