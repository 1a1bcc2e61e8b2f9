"""GPU tests of the chain batch: K independent small-design chains in one launch
(bb_small.hip k_small_chains, bb_chains_*, bridge_reg_stable_chains).

The definition under test: chain c of a batch call returns exactly what the c-th of K
consecutive bridge_reg_stable calls returns, so "equal" below is np.array_equal on every
returned array -- the batch kernel runs the single-chain kernel's sweep body on chain c's state
under the key (seed, stream + c).  Test 4 checks the batch against the CPU oracle directly,
with the whole-chain tolerances of tests/test_gpu_parity.py.
"""
import ctypes

import numpy as np
import pytest

from oracle import gibbs
from tests.conftest import synthetic_problem
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

SEED = 0xB4E5B41D6E
KEYS = ("beta", "lambda", "sig2", "tau", "alpha")


def ortho_problem():
    rng = np.random.default_rng(9)
    Q, _ = np.linalg.qr(rng.standard_normal((120, 15)))
    X = Q * 4.0
    y = X @ np.r_[np.ones(3), np.zeros(12)] + rng.standard_normal(120)
    return X, y


def assert_chain_equal(batch, c, single):
    for key in KEYS:
        assert np.array_equal(batch[key][c], single[key]), (key, c)


def sequential(bb, y, X, K, seed, **kw):
    bb.set_seed(seed)
    return [bb.bridge_reg_stb(y, X, **kw) for _ in range(K)]


# ---- 1. batch == sequential calls, bitwise ----
@pytest.mark.parametrize("n,p,kw", [
    (50, 6, {}),            # 64 lanes per lambda draw
    (100, 13, {}),          # 32 lanes
    (90, 17, {}),           # 16 lanes
    (150, 32, {}),          # two Cholesky entries per thread
    (1800, 8, {}),          # X is 115 200 B > 112 KB: read from memory, not LDS
    (120, 15, dict(ortho=True)),
    (100, 13, dict(sig2_true=1.5)),
    (100, 13, dict(tau_true=0.8)),
], ids=["50x6", "100x13", "90x17", "150x32", "1800x8", "ortho120x15", "sig2_known", "tau_known"])
def test_batch_equals_sequential_calls(gpu_lib, n, p, kw):
    """nsamp = 120 and burn = 60 cross the 50-sweep block and the 32-sweep pre-draw bounds."""
    bb = gpu_lib
    X, y = ortho_problem() if kw.get("ortho") else synthetic_problem(n, p)[:2]
    K = 5
    bb.set_seed(SEED + 7)
    g = bb.bridge_reg_stb_chains(y, X, nsamp=120, nchains=K, burn=60, **kw)
    assert bb.get_rng_state() == (SEED + 7, K)
    assert g["beta"].shape == (K, 120, p) and g["lambda"].shape == (K, 120, p)
    assert g["sig2"].shape == g["tau"].shape == g["alpha"].shape == (K, 120)
    singles = sequential(bb, y, X, K, SEED + 7, nsamp=120, burn=60, **kw)
    assert bb.get_rng_state() == (SEED + 7, K)
    for c in range(K):
        assert_chain_equal(g, c, singles[c])
    # distinct keys: the chains are not copies of one another
    assert not np.array_equal(g["beta"][0], g["beta"][1])


# ---- 2. more chains than can be resident ----
def test_more_chains_than_resident(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(50, 6)
    K = 300
    bb.set_seed(SEED + 8)
    g = bb.bridge_reg_stb_chains(y, X, nsamp=20, nchains=K, burn=5)
    assert bb.get_rng_state() == (SEED + 8, K)
    for c in (0, 255, 256, 299):
        bb.set_rng_state(SEED + 8, c)
        assert_chain_equal(g, c, bb.bridge_reg_stb(y, X, nsamp=20, burn=5))
    for key in KEYS:
        assert np.all(np.isfinite(g[key])), key
    # The .C call returns no flag words (it prints flagged chains), so what is checked on it is
    # that every output is finite.  The flag words themselves are read from a ChainBatch that
    # runs the same 300 chains for the same 25 sweeps under the same keys.
    cfg = bb.EngineConfig(n=50, p=6, trace_capacity=4, seed=SEED + 8, stream=0)
    b = bb.ChainBatch(cfg, K, X, y)
    try:
        assert b.nchains == K and b.resident_per_cu() >= 1
        b.init_state()
        b.run(1, 25, 0, 0, 0)
        b.sync()
        assert all(b.error_flags(c) == 0 for c in range(K))
    finally:
        b.close()


# ---- 3. ring wrap ----
def test_ring_wrap_equals_unwrapped(gpu_lib):
    bb = gpu_lib
    n, p, K, nsamp = 100, 13, 4, 120
    X, y, _ = synthetic_problem(n, p)
    bb.set_seed(SEED + 9)
    whole = bb.bridge_reg_stb_chains(y, X, nsamp=nsamp, nchains=K, burn=60)
    assert bb.last_call_info()["trace_capacity"] == nsamp
    # a slot holds the two traced P-vectors and three scalars; the budget bounds the batch
    per_slot = 2 * p * 8 + 3 * 8
    try:
        bb.set_trace_budget(K * 37 * per_slot)
        bb.set_seed(SEED + 9)
        wrapped = bb.bridge_reg_stb_chains(y, X, nsamp=nsamp, nchains=K, burn=60)
        assert bb.last_call_info()["trace_capacity"] == 37
    finally:
        bb.set_trace_budget(0)
    for key in KEYS:
        assert np.array_equal(wrapped[key], whole[key]), key


# ---- 4. against the oracle, independently of the single-chain GPU path ----
def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def compare_chain(g, o, tol_mean=1e-8, tol_elem=1e-6):
    """tests/test_gpu_parity.py compare_chain: g in the R layout (M x P), o the oracle's."""
    for key in KEYS:
        gv = np.asarray(g[key])
        ov = np.asarray(o[key])
        if key in ("beta", "lambda"):
            gv = gv.T  # R-style M x P  ->  P x M
        assert gv.shape == ov.shape, (key, gv.shape, ov.shape)
        assert np.all(np.isfinite(gv)), key
        e = np.max(np.abs(gv - ov) / np.maximum(np.abs(ov), 1e-8))
        assert e < tol_elem, (key, e)
    pm_g = np.asarray(g["beta"]).mean(axis=0)
    pm_o = np.asarray(o["beta"]).mean(axis=1)
    assert rel_err(pm_g, pm_o) < tol_mean


def test_batch_matches_oracle(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 20)
    K = 3
    bb.set_seed(SEED)
    g = bb.bridge_reg_stb_chains(y, X, nsamp=300, nchains=K, burn=100)
    for c in range(K):
        o = gibbs.bridge_regression_stable(y, X, 300, burn=100, alpha=0.5, seed=SEED, stream=c,
                                           method="chol")
        compare_chain({key: g[key][c] for key in KEYS}, o)


def test_packed_instance_matches_oracle(gpu_lib):
    """The 256-thread instance (bb_set_tuning key 21, batches of at least 2 x CUs chains: two
    workgroups per CU) sums rss and S_alpha in another order than the single-chain kernel, so
    it is checked against the oracle, on the first, second and last chain of a 2 x CUs batch."""
    import torch

    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 20)
    K = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    with tuning(bb, 21, 1):
        b = bb.ChainBatch(bb.EngineConfig(n=100, p=20, seed=SEED), K, X, y)
        small = bb.ChainBatch(bb.EngineConfig(n=100, p=20, seed=SEED), K - 1, X, y)
        try:
            assert b.resident_per_cu() == 2 and small.resident_per_cu() == 1
        finally:
            b.close()
            small.close()
        bb.set_seed(SEED)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=300, nchains=K, burn=100)
    for c in (0, 1, K - 1):
        o = gibbs.bridge_regression_stable(y, X, 300, burn=100, alpha=0.5, seed=SEED, stream=c,
                                           method="chol")
        compare_chain({key: g[key][c] for key in KEYS}, o)


# ---- 5. fallback: designs the batch kernel does not cover ----
@pytest.mark.parametrize("n,p,K,kw", [(60, 40, 3, {}), (80, 12, 2, dict(alpha=0.0))],
                         ids=["p40", "alpha_mh"])
def test_fallback_equals_sequential_calls(gpu_lib, n, p, K, kw):
    bb = gpu_lib
    X, y, _ = synthetic_problem(n, p, seed=3)
    bb.set_seed(SEED + 10)
    g = bb.bridge_reg_stb_chains(y, X, nsamp=40, nchains=K, burn=20, **kw)
    assert bb.get_rng_state() == (SEED + 10, K)
    singles = sequential(bb, y, X, K, SEED + 10, nsamp=40, burn=20, **kw)
    for c in range(K):
        assert_chain_equal(g, c, singles[c])


# ---- 6 / 7. ChainBatch: teacher forcing and failure isolation ----
def fresh_batch(bb, X, y, K, stream=5):
    n, p = X.shape
    cfg = bb.EngineConfig(n=n, p=p, trace_capacity=2, seed=SEED + 11, stream=stream)
    b = bb.ChainBatch(cfg, K, X, y)
    b.init_state()
    return b


def one_sweep(b, K):
    b.run(1, 1, 1, 1, 1)
    b.sync()
    return [b.trace(c, 1, 1) for c in range(K)], [b.state(c) for c in range(K)]


def test_chain_batch_teacher_forcing(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K = 3
    base = fresh_batch(bb, X, y, K)
    forced = fresh_batch(bb, X, y, K)
    eng = None
    try:
        # a fresh batch's chain c starts as a single engine on stream + c does
        cfg1 = bb.EngineConfig(n=100, p=13, trace_capacity=2, seed=SEED + 11, stream=6)
        eng = bb.Engine(cfg1, X, y)
        eng.init_state()
        s0, e0 = base.state(1), eng.state()
        assert np.array_equal(s0["beta"], e0["beta"])
        assert (s0["tau"], s0["sig2"], s0["alpha"]) == (e0["tau"], e0["sig2"], e0["alpha"])
        beta = np.linspace(-1.0, 2.0, 13)
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
        base.close()
        forced.close()
        if eng is not None:
            eng.close()


def test_chain_batch_failure_isolation(gpu_lib):
    """A NaN beta makes chain 2's Cholesky pivot fail: the kernel's numerical flag (bit 8) is
    raised in that chain's error word only, and the other chains draw what they would have."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K = 4
    base = fresh_batch(bb, X, y, K)
    bad = fresh_batch(bb, X, y, K)
    try:
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
    finally:
        base.close()
        bad.close()


# ---- 8. bad arguments ----
def test_bad_arguments(gpu_lib):
    bb = gpu_lib
    L = bb.library()
    X, y, _ = synthetic_problem(60, 40)

    def create(cfg, K, Xa):
        h = ctypes.c_void_p()
        c = cfg.to_c()
        Xf = np.asfortranarray(Xa)
        rc = L.bb_chains_create(ctypes.byref(c), K, bb._p(Xf), bb._p(y), ctypes.byref(h))
        return rc, h.value, bb._err()

    for cfg, K, Xa in (
            (bb.EngineConfig(n=60, p=40), 2, X),                        # p > 32
            (bb.EngineConfig(n=60, p=10), 0, X[:, :10]),                # no chains
            (bb.EngineConfig(n=60, p=10, true_alpha=0.0), 2, X[:, :10]),  # alpha unknown
    ):
        rc, h, msg = create(cfg, K, Xa)
        assert rc == -1 and not h and "bb_chains_create" in msg, (rc, h, msg)
    with pytest.raises(RuntimeError):
        bb.ChainBatch(bb.EngineConfig(n=60, p=40), 2, X, y)

    # .C("bridge_reg_stable_chains", ..., nchains = 0) returns without writing or taking a key
    P, N, M = 10, 60, 5
    out = [np.full(P * M, 7.0), np.full(P * M, 7.0), np.full(M, 7.0), np.full(M, 7.0),
           np.full(M, 7.0)]
    d = lambda v: ctypes.byref(ctypes.c_double(float(v)))  # noqa: E731
    i = lambda v: ctypes.byref(ctypes.c_int(int(v)))  # noqa: E731
    rt = ctypes.c_double(-1.0)
    Xf = np.asfortranarray(X[:, :P])
    bb.set_seed(SEED + 12)
    L.bridge_reg_stable_chains(*[bb._p(a) for a in out], bb._p(y), bb._p(Xf), d(0), d(0), d(2),
                               d(2), d(1), d(1), d(0), d(0), d(0.5), i(P), i(N), i(M), i(3),
                               ctypes.byref(rt), i(0), i(0))
    assert all(np.all(a == 7.0) for a in out) and rt.value == -1.0
    assert bb.get_rng_state() == (SEED + 12, 0)
    with pytest.raises(ValueError):
        bb.bridge_reg_stb_chains(y, X[:, :P], nsamp=5, nchains=0)
