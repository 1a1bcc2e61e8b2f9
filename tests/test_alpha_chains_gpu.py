"""GPU tests of alpha sampling inside the fused small chains: with bb_set_tuning key 26 set at
creation, stable-mixture engines and chain batches with p <= 32 and alpha unknown run
bb_small_mh.hip's k_small_chain_mh / k_small_chains_mh, the sweep body of bb_small.hip with the
reference's alpha MH step (BridgeRegression.cpp:469-503) after beta.

The definitions under test are those of tests/test_chains_gpu.py: the fused kernel draws the
general path's chain up to summation order, so whole chains match the CPU oracle within the
whole-chain tolerances of tests/test_gpu_parity.py (elementwise 1e-6, posterior mean 1e-8; a
flipped MH decision moves alpha by up to 0.1), and under one setting of the key chain c of a
batch is bit for bit the c-th of K consecutive bridge_reg_stb calls.  The unequal priors
(alpha_a, alpha_b) = (2, 3) tell the reference's (alpha_b, alpha_b) quirk of the non-orthogonal
MCMC loop from (alpha_a, alpha_b).  Every test that sets the key restores it in a finally.
"""
import ctypes

import numpy as np
import pytest

from oracle import gibbs
from tests.conftest import synthetic_problem
from tests.test_chains_gpu import (KEYS, assert_chain_equal, compare_chain, one_sweep,
                                   ortho_problem, sequential)
from tests.test_summary_gpu import check_against_trace_call
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

SEED = 0xB4E5B41D6E
ALPHA_KEY = 26  # bb_set_tuning: alpha sampled in the fused small chains (bb.set_fused_alpha)
PRIOR = dict(alpha_a=2.0, alpha_b=3.0)
MIN_MOVES = 10  # accepted, and rejected, proposals the oracle's alpha trace must hold


def fused_alpha(bb, on=True):
    return tuning(bb, ALPHA_KEY, 1 if on else 0)


def assert_both_branches(alpha_trace, what):
    """The condition on the inputs: the oracle's chain takes both branches of the MH step often
    (its alpha trace changes where a proposal was accepted)."""
    moved = np.diff(np.asarray(alpha_trace)) != 0
    acc, rej = int(moved.sum()), int((~moved).sum())
    print(f"{what}: {acc} accepted, {rej} rejected proposals in the oracle's trace")
    assert acc >= MIN_MOVES and rej >= MIN_MOVES, (what, acc, rej)


def oracle_kw(kw):
    """bridge_reg_stb's keywords under the oracle's names."""
    names = dict(sig2_true="true_sig2", tau_true="true_tau")
    return {names.get(k, k): v for k, v in kw.items()}


# ---- 1. whole chains against the oracle ----
@pytest.mark.parametrize("n,p,pk,kw", [
    (50, 6, {}, {}),                     # 64 lanes per lambda draw
    (80, 12, dict(seed=3), {}),          # 32 lanes
    (100, 20, {}, {}),                   # 16 lanes, two Cholesky entries per thread
    (150, 32, {}, {}),                   # the full p
    (3000, 8, {}, {}),                   # X is read from memory, not from LDS
    (1200, 8, {}, {}),                   # X is 76 800 B of LDS: the instance's opt-in above 64 KB
    (120, 15, {}, dict(ortho=True)),     # the orthogonal driver: (alpha_a, alpha_b) throughout
    (100, 13, {}, dict(tau_true=0.8)),
    (100, 13, {}, dict(sig2_true=1.5)),
], ids=["50x6", "80x12", "100x20", "150x32", "3000x8", "1200x8", "ortho120x15", "tau_known",
        "sig2_known"])
def test_chain_matches_oracle(gpu_lib, n, p, pk, kw):
    """nsamp = 120 after burn = 40: 161 sweeps, across the 32-sweep look-ahead refill and the
    50-sweep launch block."""
    bb = gpu_lib
    X, y = ortho_problem() if kw.get("ortho") else synthetic_problem(n, p, **pk)[:2]
    with fused_alpha(bb):
        bb.set_seed(SEED + 41)
        g = bb.bridge_reg_stb(y, X, nsamp=120, burn=40, alpha=0.0, **PRIOR, **kw)
    o = gibbs.bridge_regression_stable(y, X, 120, burn=40, alpha=0.0, seed=SEED + 41, stream=0,
                                       **PRIOR, **oracle_kw(kw),
                                       **({} if kw.get("ortho") else dict(method="chol")))
    assert_both_branches(o["alpha"], f"{n}x{p} {kw}")
    compare_chain(g, o)


# ---- 2. batch == sequential calls, bitwise, key on ----
def test_batch_equals_sequential_calls(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(80, 12, seed=3)
    K = 3
    kw = dict(nsamp=120, burn=40, alpha=0.0, **PRIOR)
    with fused_alpha(bb):
        bb.set_seed(SEED + 42)
        g = bb.bridge_reg_stb_chains(y, X, nchains=K, **kw)
        assert bb.get_rng_state() == (SEED + 42, K)
        singles = sequential(bb, y, X, K, SEED + 42, **kw)
        assert bb.get_rng_state() == (SEED + 42, K)
    for c in range(K):
        assert_chain_equal(g, c, singles[c])
    assert not np.array_equal(g["alpha"][0], g["alpha"][1])
    assert np.all((g["alpha"] > 0) & (g["alpha"] <= 1))


def test_more_chains_than_resident(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(50, 6)
    K = bb.compute_units() + 4
    kw = dict(nsamp=10, burn=5, alpha=0.0, **PRIOR)
    with fused_alpha(bb):
        bb.set_seed(SEED + 43)
        g = bb.bridge_reg_stb_chains(y, X, nchains=K, **kw)
        assert bb.get_rng_state() == (SEED + 43, K)
        for c in (0, 1, K - 5, K - 4, K - 1):
            bb.set_rng_state(SEED + 43, c)
            assert_chain_equal(g, c, bb.bridge_reg_stb(y, X, **kw))
    for key in KEYS:
        assert np.all(np.isfinite(g[key])), key


# ---- 3. the batch against the oracle directly ----
def test_batch_matches_oracle(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 20)
    K = 3
    with fused_alpha(bb):
        bb.set_seed(SEED + 44)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=120, nchains=K, burn=40, alpha=0.0, **PRIOR)
    for c in range(K):
        o = gibbs.bridge_regression_stable(y, X, 120, burn=40, alpha=0.0, seed=SEED + 44,
                                           stream=c, method="chol", **PRIOR)
        assert_both_branches(o["alpha"], f"chain {c}")
        compare_chain({key: g[key][c] for key in KEYS}, o)


# ---- 4 / 5. ChainBatch: teacher forcing and failure isolation ----
def fresh_batch(bb, X, y, K, stream=5):
    n, p = X.shape
    cfg = bb.EngineConfig(n=n, p=p, trace_capacity=2, seed=SEED + 45, stream=stream,
                          true_alpha=0.0, **PRIOR)
    b = bb.ChainBatch(cfg, K, X, y)
    b.init_state()
    return b


@pytest.mark.parametrize("mcmc", [0, 1], ids=["burn", "mcmc"])
def test_chain_batch_teacher_forcing(gpu_lib, mcmc):
    """One sweep from a forced state with alpha = 0.37, under the burn-in prior (alpha_a,
    alpha_b) and under the MCMC loop's (alpha_b, alpha_b): batch chain 1 against a fused engine
    (bitwise) and against an engine created with the key off, which runs and keeps the general
    path (alpha exactly -- both decide on the same proposal and uniform --, the rest within
    1e-10 relative: one sweep's summation-order differences)."""
    bb = gpu_lib
    n, p, K = 100, 13, 3
    X, y, _ = synthetic_problem(n, p)
    cfg1 = bb.EngineConfig(n=n, p=p, trace_capacity=2, seed=SEED + 45, stream=6, true_alpha=0.0,
                           **PRIOR)
    base = forced = eng = gen = None
    try:
        with fused_alpha(bb, False):
            gen = bb.Engine(cfg1, X, y)
        with fused_alpha(bb):
            base = fresh_batch(bb, X, y, K)
            forced = fresh_batch(bb, X, y, K)
            eng = bb.Engine(cfg1, X, y)
        # key restored: what exists keeps the path it was created with
        eng.init_state()
        gen.init_state()
        s0, e0, g0 = base.state(1), eng.state(), gen.state()
        assert np.array_equal(s0["beta"], e0["beta"]) and np.array_equal(s0["beta"], g0["beta"])
        assert (s0["tau"], s0["sig2"], s0["alpha"]) == (e0["tau"], e0["sig2"], e0["alpha"])
        assert (s0["tau"], s0["sig2"], s0["alpha"]) == (g0["tau"], g0["sig2"], g0["alpha"])
        beta = np.linspace(-1.0, 2.0, p)
        forced.set_state(1, beta, 0.7, 1.3, 0.37)
        want = {}
        for name, e in (("fused", eng), ("general", gen)):
            e.set_state(beta, 0.7, 1.3, 0.37)
            e.run(1, 1, 1, 1, mcmc)
            e.sync()
            assert e.error_flags() == 0, name
            want[name] = e.trace(1, 1)
        trs, sts = {}, {}
        for name, b in (("base", base), ("forced", forced)):
            b.run(1, 1, 1, 1, mcmc)
            b.sync()
            trs[name] = [b.trace(c, 1, 1) for c in range(K)]
            sts[name] = [b.state(c) for c in range(K)]
        tr_f, tr_b = trs["forced"], trs["base"]
        for key in KEYS:
            assert np.array_equal(tr_f[1][key], want["fused"][key]), key
        assert np.array_equal(sts["forced"][1]["beta"], eng.state()["beta"])
        assert sts["forced"][1]["alpha"] == eng.state()["alpha"] == tr_f[1]["alpha"][0]
        assert np.array_equal(tr_f[1]["alpha"], want["general"]["alpha"])
        assert abs(tr_f[1]["alpha"][0] - 0.37) <= 0.1
        for key in ("beta", "lambda", "tau", "sig2"):
            a, w = tr_f[1][key], want["general"][key]
            e = np.max(np.abs(a - w) / np.abs(w))
            print(f"mcmc={mcmc} {key}: max rel d against the general path = {e:.3e}")
            assert e <= 1e-10, (key, e)
        assert not np.array_equal(tr_f[1]["beta"], tr_b[1]["beta"])
        for c in (0, 2):
            for key in KEYS:
                assert np.array_equal(tr_f[c][key], tr_b[c][key]), (c, key)
            assert np.array_equal(sts["forced"][c]["beta"], sts["base"][c]["beta"])
    finally:
        for h in (base, forced, eng, gen):
            if h is not None:
                h.close()


def test_chain_batch_failure_isolation(gpu_lib):
    """tests/test_chains_gpu.py::test_chain_batch_failure_isolation with alpha unknown: a NaN
    beta loses chain 2, whose error word alone is raised while the launch ends, and the other
    chains draw what they would have."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K = 4
    base = bad = None
    with fused_alpha(bb):
        try:
            base = fresh_batch(bb, X, y, K)
            bad = fresh_batch(bb, X, y, K)
            st = bad.state(2)
            bad.set_state(2, np.full(13, np.nan), st["tau"], st["sig2"], st["alpha"])
            tr_b, st_b = one_sweep(base, K)
            tr_x, st_x = one_sweep(bad, K)
            assert bad.error_flags(2) != 0
            for c in (0, 1, 3):
                assert bad.error_flags(c) == 0 and base.error_flags(c) == 0
                for key in KEYS:
                    assert np.array_equal(tr_x[c][key], tr_b[c][key]), (c, key)
                assert np.array_equal(st_x[c]["beta"], st_b[c]["beta"])
                assert st_x[c]["alpha"] == st_b[c]["alpha"]
        finally:
            for h in (base, bad):
                if h is not None:
                    h.close()


# ---- 6. ring wrap ----
def test_ring_wrap_equals_unwrapped(gpu_lib):
    bb = gpu_lib
    n, p, K, nsamp = 100, 13, 4, 120
    X, y, _ = synthetic_problem(n, p)
    kw = dict(nsamp=nsamp, nchains=K, burn=40, alpha=0.0, **PRIOR)
    with fused_alpha(bb):
        bb.set_seed(SEED + 46)
        whole = bb.bridge_reg_stb_chains(y, X, **kw)
        assert bb.last_call_info()["trace_capacity"] == nsamp
        per_slot = 2 * p * 8 + 3 * 8
        try:
            bb.set_trace_budget(K * 37 * per_slot)
            bb.set_seed(SEED + 46)
            wrapped = bb.bridge_reg_stb_chains(y, X, **kw)
            assert bb.last_call_info()["trace_capacity"] == 37
        finally:
            bb.set_trace_budget(0)
    for key in KEYS:
        assert np.array_equal(wrapped[key], whole[key]), key
    assert np.all(whole["alpha"].std(axis=1) > 0)


# ---- 7. the summary call ----
def test_summary_call(gpu_lib):
    bb = gpu_lib
    n, p, K = 100, 13, 3
    X, y, _ = synthetic_problem(n, p)
    kw = dict(nsamp=120, nchains=K, burn=40, alpha=0.0, **PRIOR)
    with fused_alpha(bb):
        bb.set_seed(SEED + 47)
        g = bb.bridge_reg_stb_chains(y, X, **kw)
        bb.set_seed(SEED + 47)
        s = bb.bridge_reg_stb_chains_summary(y, X, **kw)
        assert bb.get_rng_state() == (SEED + 47, K)
    check_against_trace_call(bb, s, g, K, f"alpha sampled {n}x{p}")
    assert np.all(s["chain_var"][:, p + 2] > 0)


# ---- 8. the switch ----
def test_switch(gpu_lib):
    bb = gpu_lib
    L = bb.library()
    X, y, _ = synthetic_problem(200, 40, seed=3)

    def create(cfg, K, Xa):
        h = ctypes.c_void_p()
        c = cfg.to_c()
        Xf = np.asfortranarray(Xa)
        rc = L.bb_chains_create(ctypes.byref(c), K, bb._p(Xf), bb._p(y[:cfg.n]), ctypes.byref(h))
        return rc, h.value, bb._err()

    Xs = X[:80, :12]
    kept = ref = None
    try:
        with fused_alpha(bb, False):
            rc, h, msg = create(bb.EngineConfig(n=80, p=12, true_alpha=0.0), 2, Xs)
            assert rc == -1 and not h and "bb_chains_create" in msg and "alpha" in msg, msg
        with tuning(bb, 25, 1), fused_alpha(bb):
            # 32 < p <= 128 and the triangle mixture: unchanged, whatever the keys
            rc, h, msg = create(bb.EngineConfig(n=200, p=40, true_alpha=0.0), 2, X)
            assert rc == -1 and not h and "alpha" in msg, msg
            rc, h, msg = create(bb.EngineConfig(n=80, p=12, true_alpha=0.0, method=4), 2, Xs)
            assert rc == -1 and not h and "alpha" in msg, msg
        with tuning(bb, 21, 1), fused_alpha(bb):
            kept = fresh_batch(bb, Xs, y[:80], 2)
            ref = fresh_batch(bb, Xs, y[:80], 2)
            assert kept.threads() == 512 and kept.resident_per_cu() >= 1
            tr_ref, st_ref = one_sweep(ref, 2)
        # the key is back at 0: a new batch is refused, the one created under it keeps its kernel
        assert bb.set_tuning(ALPHA_KEY, -1) == 0
        with pytest.raises(RuntimeError):
            bb.ChainBatch(bb.EngineConfig(n=80, p=12, true_alpha=0.0), 2, Xs, y[:80])
        tr_kept, st_kept = one_sweep(kept, 2)
        for c in range(2):
            for key in KEYS:
                assert np.array_equal(tr_kept[c][key], tr_ref[c][key]), (c, key)
            assert np.array_equal(st_kept[c]["beta"], st_ref[c]["beta"])
            assert st_kept[c]["alpha"] == tr_kept[c]["alpha"][0]  # one MH step from 0.5
            assert abs(st_kept[c]["alpha"] - 0.5) <= 0.1
    finally:
        for b in (kept, ref):
            if b is not None:
                b.close()
