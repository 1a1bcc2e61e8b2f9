"""GPU tests of the wide fused chains: stable-mixture designs with 32 < p <= 128 run as one
workgroup per chain (bb_wide.hip k_wide_chain / k_wide_chains) once bb_set_tuning key 25 is set.

The definitions under test are those of tests/test_chains_gpu.py one size class up: under one
setting of the key, chain c of a batch call is bit for bit the c-th of K consecutive
bridge_reg_stable calls (np.array_equal on every returned array), and the batch matches the CPU
oracle within the whole-chain tolerances of tests/test_gpu_parity.py (elementwise 1e-6,
posterior mean 1e-8).  Every test that sets the key restores it in a finally.
"""
import ctypes

import numpy as np
import pytest

from oracle import gibbs
from tests.conftest import synthetic_problem
from tests.test_chains_gpu import (KEYS, assert_chain_equal, compare_chain, one_sweep,
                                   sequential)
from tests.test_summary_gpu import assert_bitwise, check_against_trace_call, raw_of
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

SEED = 0xB4E5B41D6E
WIDE_KEY = 25  # bb_set_tuning: wide fused chains (bb.set_wide_chains)


def wide_chains(bb, on=True):
    return tuning(bb, WIDE_KEY, 1 if on else 0)


def ortho_wide_problem():
    """An orthogonal 200 x 70 design, QR-based as test_chains_gpu.ortho_problem."""
    rng = np.random.default_rng(9)
    Q, _ = np.linalg.qr(rng.standard_normal((200, 70)))
    X = Q * 4.0
    y = X @ np.r_[np.ones(5), np.zeros(65)] + rng.standard_normal(200)
    return X, y


# ---- 1. batch == sequential calls, bitwise, key on ----
@pytest.mark.parametrize("n,p,kw", [
    (150, 33, {}),           # first above the old bound
    (200, 64, {}),           # full MAXP = 64
    (200, 65, {}),           # first of the 128 instance
    (300, 103, {}),          # BHI's p: not a multiple of a lambda pass
    (300, 128, {}),
    (200, 70, dict(ortho=True)),
    (200, 64, dict(sig2_true=1.5)),
    (200, 64, dict(tau_true=0.8)),
], ids=["150x33", "200x64", "200x65", "300x103", "300x128", "ortho200x70", "sig2_known",
        "tau_known"])
def test_batch_equals_sequential_calls(gpu_lib, n, p, kw):
    """nsamp = 60 and burn = 40 cross several 16-sweep blocks, which are also the pre-draw's."""
    bb = gpu_lib
    X, y = ortho_wide_problem() if kw.get("ortho") else synthetic_problem(n, p)[:2]
    K = 5
    with wide_chains(bb):
        bb.set_seed(SEED + 31)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=60, nchains=K, burn=40, **kw)
        assert bb.get_rng_state() == (SEED + 31, K)
        assert g["beta"].shape == (K, 60, p) and g["lambda"].shape == (K, 60, p)
        assert g["sig2"].shape == g["tau"].shape == g["alpha"].shape == (K, 60)
        singles = sequential(bb, y, X, K, SEED + 31, nsamp=60, burn=40, **kw)
        assert bb.get_rng_state() == (SEED + 31, K)
    for c in range(K):
        assert_chain_equal(g, c, singles[c])
    for key in KEYS:
        assert np.all(np.isfinite(g[key])), key
    assert not np.array_equal(g["beta"][0], g["beta"][1])


# ---- 2. more chains than can be resident ----
def test_more_chains_than_resident(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(80, 33)
    K = 300
    with wide_chains(bb):
        bb.set_seed(SEED + 32)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=10, nchains=K, burn=5)
        assert bb.get_rng_state() == (SEED + 32, K)
        for c in (0, 255, 256, 299):
            bb.set_rng_state(SEED + 32, c)
            assert_chain_equal(g, c, bb.bridge_reg_stb(y, X, nsamp=10, burn=5))
        for key in KEYS:
            assert np.all(np.isfinite(g[key])), key
        # the flag words, from a ChainBatch that runs the same 300 chains for the same 16 sweeps
        cfg = bb.EngineConfig(n=80, p=33, trace_capacity=4, seed=SEED + 32, stream=0)
        b = bb.ChainBatch(cfg, K, X, y)
        try:
            assert b.nchains == K and b.resident_per_cu() >= 1 and b.threads() == 256
            b.init_state()
            b.run(1, 16, 0, 0, 0)
            b.sync()
            assert all(b.error_flags(c) == 0 for c in range(K))
        finally:
            b.close()


# ---- 3. against the oracle, independently of the single-chain GPU path ----
@pytest.mark.parametrize("n,p", [(200, 64), (300, 128)], ids=["200x64", "300x128"])
def test_batch_matches_oracle(gpu_lib, n, p):
    bb = gpu_lib
    X, y, _ = synthetic_problem(n, p)
    K = 2
    with wide_chains(bb):
        bb.set_seed(SEED)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=60, nchains=K, burn=20)
    for c in range(K):
        o = gibbs.bridge_regression_stable(y, X, 60, burn=20, alpha=0.5, seed=SEED, stream=c,
                                           method="chol")
        compare_chain({key: g[key][c] for key in KEYS}, o)


# ---- 4 / 5. ChainBatch: teacher forcing and failure isolation ----
def fresh_batch(bb, X, y, K, stream=5):
    n, p = X.shape
    cfg = bb.EngineConfig(n=n, p=p, trace_capacity=2, seed=SEED + 33, stream=stream)
    b = bb.ChainBatch(cfg, K, X, y)
    b.init_state()
    return b


def test_chain_batch_teacher_forcing(gpu_lib):
    bb = gpu_lib
    n, p, K = 200, 64, 3
    X, y, _ = synthetic_problem(n, p)
    base = forced = eng = None
    with wide_chains(bb):
        try:
            base = fresh_batch(bb, X, y, K)
            forced = fresh_batch(bb, X, y, K)
            cfg1 = bb.EngineConfig(n=n, p=p, trace_capacity=2, seed=SEED + 33, stream=6)
            eng = bb.Engine(cfg1, X, y)
            eng.init_state()
            s0, e0 = base.state(1), eng.state()
            assert np.array_equal(s0["beta"], e0["beta"])
            assert (s0["tau"], s0["sig2"], s0["alpha"]) == (e0["tau"], e0["sig2"], e0["alpha"])
            beta = np.linspace(-1.0, 2.0, p)
            forced.set_state(1, beta, 0.7, 1.3, 0.5)
            eng.set_state(beta, 0.7, 1.3, 0.5)
            eng.run(1, 1, 1, 1, 1)
            eng.sync()
            want = eng.trace(1, 1)
            tr_b, st_b = one_sweep(base, K)
            tr_f, st_f = one_sweep(forced, K)
            for key in KEYS:
                assert np.array_equal(tr_f[1][key], want[key]), key
            assert np.array_equal(st_f[1]["beta"], eng.state()["beta"])
            assert not np.array_equal(tr_f[1]["beta"], tr_b[1]["beta"])
            for c in (0, 2):
                for key in KEYS:
                    assert np.array_equal(tr_f[c][key], tr_b[c][key]), (c, key)
                assert np.array_equal(st_f[c]["beta"], st_b[c]["beta"])
        finally:
            for h in (base, forced, eng):
                if h is not None:
                    h.close()


def test_chain_batch_failure_isolation(gpu_lib):
    """A NaN beta loses chain 2: its error word alone is raised, and the other chains draw what
    they would have."""
    bb = gpu_lib
    n, p, K = 200, 64, 4
    X, y, _ = synthetic_problem(n, p)
    base = bad = None
    with wide_chains(bb):
        try:
            base = fresh_batch(bb, X, y, K)
            bad = fresh_batch(bb, X, y, K)
            st = bad.state(2)
            bad.set_state(2, np.full(p, np.nan), st["tau"], st["sig2"], st["alpha"])
            tr_b, st_b = one_sweep(base, K)
            tr_x, st_x = one_sweep(bad, K)
            assert bad.error_flags(2) != 0
            for c in (0, 1, 3):
                assert bad.error_flags(c) == 0 and base.error_flags(c) == 0
                for key in KEYS:
                    assert np.array_equal(tr_x[c][key], tr_b[c][key]), (c, key)
                assert np.array_equal(st_x[c]["beta"], st_b[c]["beta"])
        finally:
            for h in (base, bad):
                if h is not None:
                    h.close()


# ---- 6. ring wrap ----
def test_ring_wrap_equals_unwrapped(gpu_lib):
    bb = gpu_lib
    n, p, K, nsamp = 200, 64, 4, 60
    X, y, _ = synthetic_problem(n, p)
    with wide_chains(bb):
        bb.set_seed(SEED + 34)
        whole = bb.bridge_reg_stb_chains(y, X, nsamp=nsamp, nchains=K, burn=40)
        assert bb.last_call_info()["trace_capacity"] == nsamp
        per_slot = 2 * p * 8 + 3 * 8
        try:
            bb.set_trace_budget(K * 23 * per_slot)
            bb.set_seed(SEED + 34)
            wrapped = bb.bridge_reg_stb_chains(y, X, nsamp=nsamp, nchains=K, burn=40)
            assert bb.last_call_info()["trace_capacity"] == 23
        finally:
            bb.set_trace_budget(0)
    for key in KEYS:
        assert np.array_equal(wrapped[key], whole[key]), key


# ---- 7. the summary call ----
def test_summary_call(gpu_lib):
    bb = gpu_lib
    n, p, K = 200, 64, 3
    X, y, _ = synthetic_problem(n, p)
    with wide_chains(bb):
        bb.set_seed(SEED + 35)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=60, nchains=K, burn=40)
        bb.set_seed(SEED + 35)
        s = bb.bridge_reg_stb_chains_summary(y, X, nsamp=60, nchains=K, burn=40)
        assert bb.get_rng_state() == (SEED + 35, K)
    check_against_trace_call(bb, s, g, K, f"wide {n}x{p}")
    assert np.all(s["chain_mean"][:, p + 2] == 0.5) and np.all(s["chain_var"][:, p + 2] == 0.0)


# ---- 8. bounds and the switch ----
def test_bounds_and_switch(gpu_lib):
    bb = gpu_lib
    L = bb.library()
    X, y, _ = synthetic_problem(200, 129, seed=3)

    def create(cfg, K, Xa):
        h = ctypes.c_void_p()
        c = cfg.to_c()
        Xf = np.asfortranarray(Xa)
        rc = L.bb_chains_create(ctypes.byref(c), K, bb._p(Xf), bb._p(y[:cfg.n]), ctypes.byref(h))
        return rc, h.value, bb._err()

    kept = ref = None
    try:
        with wide_chains(bb):
            rc, h, msg = create(bb.EngineConfig(n=200, p=129), 2, X)
            assert rc == -1 and not h and "bb_chains_create" in msg and "128" in msg, msg
            rc, h, msg = create(bb.EngineConfig(n=60, p=100), 2, X[:60, :100])  # p > n
            assert rc == -1 and not h and "p <= n" in msg, msg
            rc, h, msg = create(bb.EngineConfig(n=200, p=40, true_alpha=0.0), 2, X[:, :40])
            assert rc == -1 and not h and "alpha" in msg, msg
            # alpha unknown: the .C call runs the chains one after another
            Xa = X[:80, :40]
            bb.set_seed(SEED + 36)
            g = bb.bridge_reg_stb_chains(y[:80], Xa, nsamp=20, nchains=2, burn=10, alpha=0.0)
            assert bb.get_rng_state() == (SEED + 36, 2)
            singles = sequential(bb, y[:80], Xa, 2, SEED + 36, nsamp=20, burn=10, alpha=0.0)
            for c in range(2):
                assert_chain_equal(g, c, singles[c])
            Xw, yw, _ = synthetic_problem(200, 64)
            kept = fresh_batch(bb, Xw, yw, 2)
            ref = fresh_batch(bb, Xw, yw, 2)
            tr_ref, st_ref = one_sweep(ref, 2)
        # the key is back at 0: p = 40 is refused again, and the batch created while it was on
        # keeps the wide kernel
        assert bb.set_tuning(WIDE_KEY, -1) == 0
        with pytest.raises(RuntimeError):
            bb.ChainBatch(bb.EngineConfig(n=60, p=40), 2, X[:60, :40], y[:60])
        assert kept.threads() == 256  # k_wide_chains<64, 256>; k_small_chains runs 512
        tr_kept, st_kept = one_sweep(kept, 2)
        for c in range(2):
            for key in KEYS:
                assert np.array_equal(tr_kept[c][key], tr_ref[c][key]), (c, key)
            assert np.array_equal(st_kept[c]["beta"], st_ref[c]["beta"])
    finally:
        for b in (kept, ref):
            if b is not None:
                b.close()
