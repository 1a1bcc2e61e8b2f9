"""GPU tests of the triangle-mixture chain batch: K independent bridge.reg.tri chains in one
launch (bb_tri.hip k_tri_chains, bb_chains_* with method 4, bridge_regression_chains).

The definition under test: chain c of a batch call returns exactly what the c-th of K
consecutive bridge_regression calls returns, so "equal" below is np.array_equal on beta, u, w,
shape, sig2, tau and alpha -- every instance of the batch kernel runs the single-chain kernel's
sweep body on chain c's state under the key (seed, stream + c) and keeps its summation order.
Test 5 checks the batch against the CPU oracle directly, with the per-sweep teacher-forced bar
of tests/test_triangle_gpu.py (free-running triangle chains are chaotic under roundoff).
"""
import ctypes
import time

import numpy as np
import pytest

from bayesbridge_amd import diagnostics as dg
from oracle import gibbs
from tests.conftest import synthetic_problem

pytestmark = pytest.mark.gpu

SEED = 0x7C1A9E5
KEYS = ("beta", "u", "w", "shape", "sig2", "tau", "alpha")
TRACE_KEYS = ("beta", "lambda", "sig2", "tau", "alpha")
_cache = {}


def ortho_problem():
    """As ortho_problem() of tests/test_chains_gpu.py."""
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
    return [bb.bridge_reg_tri(y, X, extras=True, **kw) for _ in range(K)]


# ---- 1. batch == sequential calls, bitwise ----
@pytest.mark.parametrize("n,p,kw", [
    (50, 6, {}),
    (100, 20, {}),
    (150, 32, {}),          # p at the kernel's limit
    (400, 32, {}),          # X is 102 400 B > 96 KB: read from memory, not LDS
    (120, 15, dict(ortho=True)),
    (80, 24, dict(betaburn=2)),
    (100, 20, dict(sig2_true=1.5)),
    (100, 20, dict(tau_true=0.8)),
], ids=["50x6", "100x20", "150x32", "400x32", "ortho120x15", "betaburn", "sig2_known",
        "tau_known"])
def test_batch_equals_sequential_calls(gpu_lib, n, p, kw):
    """nsamp = 120 and burn = 60 cross the 50-sweep block."""
    bb = gpu_lib
    X, y = ortho_problem() if kw.get("ortho") else synthetic_problem(n, p)[:2]
    K = 5
    bb.set_seed(SEED + 7)
    g = bb.bridge_reg_tri_chains(y, X, nsamp=120, nchains=K, burn=60, **kw)
    assert bb.get_rng_state() == (SEED + 7, K)
    for key in ("beta", "u", "w", "shape"):
        assert g[key].shape == (K, 120, p), key
    assert g["sig2"].shape == g["tau"].shape == g["alpha"].shape == (K, 120)
    singles = sequential(bb, y, X, K, SEED + 7, nsamp=120, burn=60, **kw)
    assert bb.get_rng_state() == (SEED + 7, K)
    for c in range(K):
        assert_chain_equal(g, c, singles[c])
    # distinct keys: the chains are not copies of one another
    assert not np.array_equal(g["beta"][0], g["beta"][1])
    if (n, p) == (100, 20) and not kw:
        _cache["c1"] = g


# ---- 2. every shipped instance ----
@pytest.mark.parametrize("per_cu,threads", [(1, 256), (2, 128)], ids=["256t", "128t"])
def test_narrow_instances_are_bitwise(gpu_lib, per_cu, threads):
    """A batch runs the widest instance that holds all its chains at once.  The narrow
    instances keep 512 virtual threads and size their LDS by p; DESIGN.md s6.4: at 100 x 20
    they take 39 472 B of LDS and 256 VGPRs, so the 256-thread instance holds two chains per
    CU and the 128-thread instance four, where the 512-thread instance holds one."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 20)
    K = per_cu * bb.compute_units() + 1  # one more than the next wider instance holds
    cfg = bb.EngineConfig(n=100, p=20, method=4, seed=SEED)
    wider = bb.ChainBatch(cfg, K - 1, X, y)
    narrow = bb.ChainBatch(cfg, K, X, y)
    try:
        assert wider.threads() == 2 * threads and wider.resident_per_cu() == per_cu
        assert narrow.threads() == threads and narrow.resident_per_cu() == 2 * per_cu
    finally:
        wider.close()
        narrow.close()
    bb.set_seed(SEED + 1)
    g = bb.bridge_reg_tri_chains(y, X, nsamp=120, nchains=K, burn=60)
    for c in (0, 1, K - 1):
        bb.set_rng_state(SEED + 1, c)
        assert_chain_equal(g, c, bb.bridge_reg_tri(y, X, nsamp=120, burn=60, extras=True))


@pytest.mark.parametrize("case", ["general", "ortho", "x_in_memory"])
def test_instances_agree_bitwise(gpu_lib, case):
    """The 512-, 256- and 128-thread instances on the same small batch: the same bits in
    every trace, for the general and the orthogonal pass and with X read from memory."""
    bb = gpu_lib
    if case == "ortho":
        X, y = ortho_problem()
    else:
        X, y, _ = synthetic_problem(*((400, 32) if case == "x_in_memory" else (90, 17)))
    n, p = X.shape
    got = []
    for threads in (512, 256, 128):
        cfg = bb.EngineConfig(n=n, p=p, method=4, seed=SEED + 2, stream=3, trace_capacity=8,
                              ortho=case == "ortho")
        b = bb.ChainBatch(cfg, 3, X, y)
        try:
            b.set_threads(threads)
            assert b.threads() == threads
            b.init_state()
            b.run(1, 7, 1, 1, 1)
            b.sync()
            assert all(b.error_flags(c) == 0 for c in range(3))
            got.append([(b.trace(c, 0, 8), b.tri_trace(c, 0, 8)) for c in range(3)])
            with pytest.raises(RuntimeError):
                b.set_threads(96)
        finally:
            b.close()
    for narrow in got[1:]:
        for (t5, r5), (t1, r1) in zip(got[0], narrow):
            for key in TRACE_KEYS:
                assert np.array_equal(t5[key], t1[key]), key
            for key in ("u", "shape"):
                assert np.array_equal(r5[key], r1[key]), key


# ---- 3. more chains than can be resident ----
def test_more_chains_than_resident(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(50, 6)
    K = 300
    bb.set_seed(SEED + 8)
    g = bb.bridge_reg_tri_chains(y, X, nsamp=20, nchains=K, burn=5)
    assert bb.get_rng_state() == (SEED + 8, K)
    for c in (0, 255, 256, 299):
        bb.set_rng_state(SEED + 8, c)
        assert_chain_equal(g, c, bb.bridge_reg_tri(y, X, nsamp=20, burn=5, extras=True))
    for key in KEYS:
        assert np.all(np.isfinite(g[key])), key
    # the flag words, from a ChainBatch that runs the same 300 chains under the same keys
    cfg = bb.EngineConfig(n=50, p=6, method=4, trace_capacity=4, seed=SEED + 8, stream=0)
    b = bb.ChainBatch(cfg, K, X, y)
    try:
        assert b.nchains == K and b.resident_per_cu() >= 1
        b.init_state()
        b.run(1, 25, 0, 0, 0)
        b.sync()
        assert all(b.error_flags(c) == 0 for c in range(K))
    finally:
        b.close()


# ---- 4. ring wrap ----
def test_ring_wrap_equals_unwrapped(gpu_lib):
    bb = gpu_lib
    n, p, K, nsamp = 100, 20, 4, 120
    X, y, _ = synthetic_problem(n, p)
    bb.set_seed(SEED + 9)
    whole = bb.bridge_reg_tri_chains(y, X, nsamp=nsamp, nchains=K, burn=60)
    assert bb.last_call_info()["trace_capacity"] == nsamp
    # a slot holds the four traced P-vectors and three scalars; the budget bounds the batch
    per_slot = 4 * p * 8 + 3 * 8
    try:
        bb.set_trace_budget(K * 37 * per_slot)
        bb.set_seed(SEED + 9)
        wrapped = bb.bridge_reg_tri_chains(y, X, nsamp=nsamp, nchains=K, burn=60)
        assert bb.last_call_info()["trace_capacity"] == 37
    finally:
        bb.set_trace_budget(0)
    for key in KEYS:
        assert np.array_equal(wrapped[key], whole[key]), key


# ---- 5. against the oracle, not through the single-chain GPU path ----
def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-12)))


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("ortho", [False, True], ids=["general", "ortho"])
def test_batch_sweeps_teacher_forced_from_oracle(gpu_lib, ortho):
    """tests/test_triangle_gpu.py test_tri_sweeps_teacher_forced on chains 0 and 2 of a K = 3
    batch: every sweep forced from the oracle's state of stream c agrees to 1e-10 with
    identical mixture shapes."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 20, seed=5)
    seed, M, tol, K = 777, 40, 1e-10, 3
    cfg = bb.EngineConfig(n=100, p=20, method=4, seed=seed, stream=0, trace_capacity=1,
                          ortho=ortho)
    b = bb.ChainBatch(cfg, K, X, y)
    try:
        basis = b.tri_basis()
        for c in (0, 2):
            b.init_state()
            o = gibbs.bridge_regression_tri(y, X, M, basis, burn=0, betaburn=0, seed=seed,
                                            stream=c, true_alpha=0.5, ortho=ortho)
            for i in range(1, M):
                b.set_state(c, o["beta"][i - 1], o["tau"][i - 1], o["sig2"][i - 1], 0.5)
                b.set_tri_state(c, o["u"][i - 1])
                b.run(i, 1, first_slot=0, slot_step=0, mcmc_phase=1)
                g, gt = b.trace(c, 0, 1), b.tri_trace(c, 0, 1)
                assert np.array_equal(gt["shape"][:, 0], o["shape"][i]), (c, i)
                assert rel_l2(g["beta"][:, 0], o["beta"][i]) < tol, (c, i)
                assert rel_l2(gt["u"][:, 0], o["u"][i]) < tol, (c, i)
                assert rel_l2(g["lambda"][:, 0], o["w"][i]) < tol, (c, i)
                for k in ("tau", "sig2", "alpha"):
                    assert rel(g[k][0], o[k][i]) < 1e-10, (c, i, k)
        assert all(b.error_flags(c) == 0 for c in range(K))
    finally:
        b.close()


# ---- 6. ChainBatch: teacher forcing and failure isolation ----
def fresh_batch(bb, X, y, K, stream=5):
    n, p = X.shape
    cfg = bb.EngineConfig(n=n, p=p, method=4, trace_capacity=2, seed=SEED + 11, stream=stream)
    b = bb.ChainBatch(cfg, K, X, y)
    b.init_state()
    return b


def one_sweep(b, K):
    b.run(1, 1, 1, 1, 1)
    b.sync()
    tr = []
    for c in range(K):
        t = b.trace(c, 1, 1)
        t.update(b.tri_trace(c, 1, 1))
        tr.append(t)
    return tr, [b.state(c) for c in range(K)]


SWEEP_KEYS = TRACE_KEYS + ("u", "shape")


def test_chain_batch_teacher_forcing(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K = 3
    base = fresh_batch(bb, X, y, K)
    forced = fresh_batch(bb, X, y, K)
    eng = None
    try:
        # a fresh batch's chain c starts as a single engine on stream + c does
        cfg1 = bb.EngineConfig(n=100, p=13, method=4, trace_capacity=2, seed=SEED + 11,
                               stream=6)
        eng = bb.Engine(cfg1, X, y)
        eng.init_state()
        s0, e0 = base.state(1), eng.state()
        assert np.array_equal(s0["beta"], e0["beta"])
        assert np.array_equal(s0["lambda"], e0["lambda"])
        assert (s0["tau"], s0["sig2"], s0["alpha"]) == (e0["tau"], e0["sig2"], e0["alpha"])
        t0, te = base.trace(1, 0, 1), eng.trace(0, 1)
        for key in TRACE_KEYS:
            assert np.array_equal(t0[key], te[key]), key
        assert np.array_equal(base.tri_trace(1, 0, 1)["u"], eng.tri_trace(0, 1)["u"])
        beta = np.linspace(-1.0, 2.0, 13)
        u = np.linspace(0.1, 0.7, 13)
        forced.set_state(1, beta, 0.7, 1.3, 0.5)
        forced.set_tri_state(1, u)
        eng.set_state(beta, 0.7, 1.3, 0.5)
        eng.set_tri_state(u)
        eng.run(1, 1, 1, 1, 1)
        eng.sync()
        want = eng.trace(1, 1)
        want.update(eng.tri_trace(1, 1))
        tr_b, st_b = one_sweep(base, K)
        tr_f, st_f = one_sweep(forced, K)
        for key in SWEEP_KEYS:
            assert np.array_equal(tr_f[1][key], want[key]), key
        assert np.array_equal(st_f[1]["beta"], eng.state()["beta"])
        assert not np.array_equal(tr_f[1]["beta"], tr_b[1]["beta"])
        for c in (0, 2):
            for key in SWEEP_KEYS:
                assert np.array_equal(tr_f[c][key], tr_b[c][key]), (c, key)
            assert np.array_equal(st_f[c]["beta"], st_b[c]["beta"])
    finally:
        base.close()
        forced.close()
        if eng is not None:
            eng.close()


def test_chain_batch_failure_isolation(gpu_lib):
    """A NaN beta gives chain 2 an empty truncation interval: the kernel's flag (bit 128) is
    raised in that chain's error word only, at once, and the other chains draw what they
    would have."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K = 4
    base = fresh_batch(bb, X, y, K)
    bad = fresh_batch(bb, X, y, K)
    try:
        st = bad.state(2)
        bad.set_state(2, np.full(13, np.nan), st["tau"], st["sig2"], st["alpha"])
        tr_b, st_b = one_sweep(base, K)
        t0 = time.perf_counter()
        tr_x, st_x = one_sweep(bad, K)
        # a sweep takes tens of microseconds; 2^22 rejected attempts per draw take seconds
        assert time.perf_counter() - t0 < 1.0
        assert bad.error_flags(2) != 0
        for c in (0, 1, 3):
            assert bad.error_flags(c) == 0 and base.error_flags(c) == 0
            for key in SWEEP_KEYS:
                assert np.array_equal(tr_x[c][key], tr_b[c][key]), (c, key)
            assert np.array_equal(st_x[c]["beta"], st_b[c]["beta"])
    finally:
        base.close()
        bad.close()


# ---- 7. fallback and bad arguments ----
@pytest.mark.parametrize("n,p,K,kw", [(80, 33, 3, {}), (80, 12, 2, dict(alpha=0.0))],
                         ids=["p33", "alpha_mh"])
def test_fallback_equals_sequential_calls(gpu_lib, n, p, K, kw):
    bb = gpu_lib
    X, y, _ = synthetic_problem(n, p, seed=3)
    bb.set_seed(SEED + 10)
    g = bb.bridge_reg_tri_chains(y, X, nsamp=40, nchains=K, burn=20, **kw)
    assert bb.get_rng_state() == (SEED + 10, K)
    singles = sequential(bb, y, X, K, SEED + 10, nsamp=40, burn=20, **kw)
    for c in range(K):
        assert_chain_equal(g, c, singles[c])


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
            (bb.EngineConfig(n=60, p=40, method=4), 2, X),                        # p > 32
            (bb.EngineConfig(n=60, p=10, method=4), 0, X[:, :10]),                # no chains
            (bb.EngineConfig(n=60, p=10, method=4, true_alpha=0.0), 2, X[:, :10]),
    ):
        rc, h, msg = create(cfg, K, Xa)
        assert rc == -1 and not h and "bb_chains_create" in msg, (rc, h, msg)

    # the triangle calls refuse a stable batch
    sb = bb.ChainBatch(bb.EngineConfig(n=60, p=10), 2, X[:, :10], y)
    try:
        with pytest.raises(RuntimeError):
            sb.tri_basis()
        with pytest.raises(RuntimeError):
            sb.set_tri_state(0, np.zeros(10))
    finally:
        sb.close()

    # .C("bridge_regression_chains", ..., nchains = 0) returns without writing or taking a key
    P, N, M = 10, 60, 5
    out = [np.full(P * M, 7.0) for _ in range(4)] + [np.full(M, 7.0) for _ in range(3)]
    d = lambda v: ctypes.byref(ctypes.c_double(float(v)))  # noqa: E731
    i = lambda v: ctypes.byref(ctypes.c_int(int(v)))  # noqa: E731
    rt = ctypes.c_double(-1.0)
    Xf = np.asfortranarray(X[:, :P])
    bb.set_seed(SEED + 12)
    L.bridge_regression_chains(*[bb._p(a) for a in out], bb._p(y), bb._p(Xf), d(0), d(0), d(2),
                               d(2), d(1), d(1), d(0), d(0), d(0.5), i(P), i(N), i(M), i(3),
                               ctypes.byref(rt), i(0), i(0), i(0), i(0))
    assert all(np.all(a == 7.0) for a in out) and rt.value == -1.0
    assert bb.get_rng_state() == (SEED + 12, 0)
    with pytest.raises(ValueError):
        bb.bridge_reg_tri_chains(y, X[:, :P], nsamp=5, nchains=0)


# ---- 8. diagnostics ----
def test_diagnostics_take_the_batch_output(gpu_lib):
    bb = gpu_lib
    g = _cache.get("c1")
    if g is None:  # run alone: the (100, 20) batch of test 1
        X, y, _ = synthetic_problem(100, 20)
        bb.set_seed(SEED + 7)
        g = bb.bridge_reg_tri_chains(y, X, nsamp=120, nchains=5, burn=60)
    r = dg.rhat(g["beta"])
    assert r.shape == (20,) and np.all(np.isfinite(r))
    s = dg.sum_stat_chains(g["beta"], g["runtime"])
    assert s["chains"] == 5 and s["rhat"].shape == (20,)
    for key in ("mean", "sd", "ess", "esr", "rhat"):
        assert np.asarray(s[key]).shape == (20,) and np.all(np.isfinite(s[key])), key
