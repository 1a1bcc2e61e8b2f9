"""GPU tests of alpha sampling inside the fused triangle-mixture chains: with bb_set_tuning key 27
set at creation, triangle engines and chain batches with p <= 32, p <= n and alpha unknown run
bb_tri_mh.hip's k_tri_chain_mh / k_tri_chains_mh, the sweep body of bb_tri.hip with the
reference's alpha MH step (BridgeRegression.cpp:469-503) after the sweep's last beta.

Free-running triangle chains are chaotic under roundoff (tests/test_triangle_gpu.py), so the
comparisons with the CPU oracle are teacher-forced sweep by sweep, at that file's bars (mixture
shapes equal, beta, u, omega within 1e-10 relative L2, tau, sig2 and alpha within 1e-10), and
whole chains are compared only against the device itself, bit for bit: one launch against its
sweeps, the batch against sequential calls, the narrow instances against the 512-thread one.
The prior is (alpha_a, alpha_b) = (2, 3) wherever alpha is compared.  Every test that sets the
key restores it in a finally (tests/tuning.py).
"""
import ctypes
import time

import numpy as np
import pytest

from oracle import gibbs
from tests.conftest import synthetic_problem
from tests.test_summary_gpu import check_against_trace_call
from tests.test_tri_chains_gpu import (KEYS, SWEEP_KEYS, TRACE_KEYS, assert_chain_equal,
                                       one_sweep, ortho_problem, rel, rel_l2, sequential)
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

SEED = 0x7A1F4A3
TRI_ALPHA_KEY = 27  # bb_set_tuning: alpha sampled in the fused triangle chains
PRIOR = dict(alpha_a=2.0, alpha_b=3.0)
MIN_MOVES = 10  # accepted, and rejected, proposals the oracle's alpha trace must hold
TOL = 1e-10


def fused_tri_alpha(bb, on=True):
    return tuning(bb, TRI_ALPHA_KEY, 1 if on else 0)


def assert_both_branches(alpha_trace, what, bind=True):
    """The condition on the inputs: the oracle's chain takes both branches of the MH step often
    (its alpha trace changes where a proposal was accepted)."""
    moved = np.diff(np.asarray(alpha_trace)) != 0
    acc, rej = int(moved.sum()), int((~moved).sum())
    print(f"{what}: {acc} accepted, {rej} rejected proposals in the oracle's trace")
    assert not bind or (acc >= MIN_MOVES and rej >= MIN_MOVES), (what, acc, rej)


def tri_config(bb, n, p, **kw):
    cfg = bb.EngineConfig(n=n, p=p, method=4, true_alpha=0.0, **PRIOR)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def launch_brackets(bb, e, count=5):
    """Timing brackets that run(1, count) opens on engine e, from its starting state: a fused
    engine brackets the whole run once (one launch), the general path every sweep.  The engine
    is left at its starting state, timing off."""
    L = bb.library()
    e.init_state()
    e.enable_timing(True)
    e.reset_timing()
    e.run(1, count, -1, 1, 1)
    e.sync()
    ms, n = np.zeros(L.bb_phase_count()), ctypes.c_int()
    bb._check(L.bb_engine_phase_times(e._h, bb._p(ms), len(ms), ctypes.byref(n)),
              "bb_engine_phase_times")
    e.enable_timing(False)
    e.reset_timing()
    assert e.error_flags() == 0
    e.init_state()
    return n.value


def assert_fused(bb, e, fused=True):
    assert launch_brackets(bb, e) == (1 if fused else 5)


# ---- 1. every sweep teacher-forced from the oracle's state ----
# (n, p, problem seed, engine settings, streams on which the condition on the inputs is asserted).
# The engine draws under stream 0 and chain c of the batch under stream c; chains 0 and 2 are
# compared at every shape (chain 2 is the one whose state, ring and key offsets are not zero).
# assert_both_branches holds for stream 0 at every shape (18-28 accepted, 12-22 rejected) and for
# stream 2 at every shape but 50 x 6 (21-30 and 10-19; 50 x 6: 36 accepted, 4 rejected), where
# chain 2 is compared all the same and the condition rests on stream 0.
CHAINS = (0, 2)
FORCED = {
    "100x20": (100, 20, 5, {}, (0, 2)),
    "ortho100x20": (100, 20, 5, dict(ortho=True), (0, 2)),
    "50x6": (50, 6, 5, {}, (0,)),
    "150x32": (150, 32, 5, {}, (0, 2)),                     # the full p
    "x_in_memory400x32": (400, 32, 5, {}, (0, 2)),          # 102 400 B > the LDS staging limit
    "betaburn80x24": (80, 24, 5, dict(betaburn=2), (0, 2)),
    "tau_known": (100, 20, 5, dict(true_tau=0.8), (0, 2)),
    "sig2_known": (100, 20, 5, dict(true_sig2=1.5), (0, 2)),
    "tau_sig2_known": (100, 20, 5, dict(true_tau=0.8, true_sig2=1.5), (0, 2)),
}


def assert_sweep(g, gt, o, i, what):
    assert np.array_equal(gt["shape"][:, 0], o["shape"][i]), (what, i)
    for name, a, w in (("beta", g["beta"][:, 0], o["beta"][i]), ("u", gt["u"][:, 0], o["u"][i]),
                       ("omega", g["lambda"][:, 0], o["w"][i])):
        err = rel_l2(a, w)
        assert err < TOL, (what, i, name, err)
    for k in ("tau", "sig2", "alpha"):
        err = rel(g[k][0], o[k][i])
        assert err < TOL, (what, i, k, err)


@pytest.mark.parametrize("case", list(FORCED))
def test_sweeps_teacher_forced(gpu_lib, case):
    """tests/test_triangle_gpu.py::test_tri_sweeps_teacher_forced with alpha forced to the
    oracle's previous value: 40 sweeps of a fused engine (stream 0) and of chains 0 and 2 of a
    K = 3 batch (streams 0 and 2)."""
    bb = gpu_lib
    n, p, pseed, kw, both = FORCED[case]
    X, y, _ = synthetic_problem(n, p, seed=pseed)
    seed, M, K = 777, 41, 3
    okw = dict(burn=0, betaburn=kw.get("betaburn", 0), seed=seed, true_alpha=0.0,
               ortho=kw.get("ortho", False), true_tau=kw.get("true_tau", 0.0),
               true_sig2=kw.get("true_sig2", 0.0), **PRIOR)
    e = b = None
    try:
        with fused_tri_alpha(bb):
            e = bb.Engine(tri_config(bb, n, p, seed=seed, stream=0, trace_capacity=1, **kw), X, y)
            b = bb.ChainBatch(tri_config(bb, n, p, seed=seed, stream=0, trace_capacity=1, **kw),
                              K, X, y)
        assert_fused(bb, e)
        basis = e.tri_basis()
        oracle = {c: gibbs.bridge_regression_tri(y, X, M, basis, stream=c, **okw) for c in CHAINS}
        for c in CHAINS:  # every stream's counts are printed; the condition binds those listed
            assert_both_branches(oracle[c]["alpha"], f"{case} stream {c}", bind=c in both)
        e.init_state()
        o = oracle[0]
        for i in range(1, M):
            e.set_state(o["beta"][i - 1], o["tau"][i - 1], o["sig2"][i - 1], o["alpha"][i - 1])
            e.set_tri_state(o["u"][i - 1])
            e.run(i, 1, first_slot=0, slot_step=0, mcmc_phase=1)
            assert_sweep(e.trace(0, 1), e.tri_trace(0, 1), o, i, f"{case} engine")
            assert e.state()["alpha"] == e.trace(0, 1)["alpha"][0]
        assert e.error_flags() == 0
        for c, o in oracle.items():
            b.init_state()
            for i in range(1, M):
                b.set_state(c, o["beta"][i - 1], o["tau"][i - 1], o["sig2"][i - 1],
                            o["alpha"][i - 1])
                b.set_tri_state(c, o["u"][i - 1])
                b.run(i, 1, first_slot=0, slot_step=0, mcmc_phase=1)
                assert_sweep(b.trace(c, 0, 1), b.tri_trace(c, 0, 1), o, i, f"{case} chain {c}")
        assert all(b.error_flags(c) == 0 for c in range(K))
    finally:
        for h in (e, b):
            if h is not None:
                h.close()


# ---- 2. one launch equals its sweeps ----
@pytest.mark.parametrize("ortho", [False, True], ids=["general", "ortho"])
def test_one_launch_equals_its_sweeps(gpu_lib, ortho):
    """run(t0, 50) against fifty run(t0 + k, 1), bit for bit in the traces and the state, on the
    engine and on the batch: alpha carried in LDS, tau's gamma variate drawn in the sweep and the
    look-ahead buffer across sweeps give what the one-sweep launches of test 1 give."""
    bb = gpu_lib
    n, p, K, count = 100, 13, 3, 50
    X, y, _ = synthetic_problem(n, p)
    cfg = dict(seed=SEED + 2, stream=4, trace_capacity=count + 1, ortho=ortho)
    hs = []
    try:
        with fused_tri_alpha(bb):
            eng = [bb.Engine(tri_config(bb, n, p, **cfg), X, y) for _ in range(2)]
            hs += eng
            bat = [bb.ChainBatch(tri_config(bb, n, p, **cfg), K, X, y) for _ in range(2)]
            hs += bat
        for e in eng:
            assert_fused(bb, e)
        for h in hs:
            h.init_state()
        for whole, steps in (eng, bat):
            whole.run(1, count, 1, 1, 1)
            for k in range(count):
                steps.run(1 + k, 1, 1 + k, 1, 1)
            whole.sync()
            steps.sync()
        tw, ts = eng[0].trace(1, count), eng[1].trace(1, count)
        tw.update(eng[0].tri_trace(1, count))
        ts.update(eng[1].tri_trace(1, count))
        for key in SWEEP_KEYS:
            assert np.array_equal(tw[key], ts[key]), ("engine", key)
        sw, ss = eng[0].state(), eng[1].state()
        assert np.array_equal(sw["beta"], ss["beta"]) and sw["alpha"] == ss["alpha"]
        assert (sw["tau"], sw["sig2"]) == (ss["tau"], ss["sig2"])
        assert sw["alpha"] == tw["alpha"][-1] and np.std(tw["alpha"]) > 0
        assert eng[0].error_flags() == 0 and eng[1].error_flags() == 0
        for c in range(K):
            tw, ts = bat[0].trace(c, 1, count), bat[1].trace(c, 1, count)
            tw.update(bat[0].tri_trace(c, 1, count))
            ts.update(bat[1].tri_trace(c, 1, count))
            for key in SWEEP_KEYS:
                assert np.array_equal(tw[key], ts[key]), (c, key)
            sw, ss = bat[0].state(c), bat[1].state(c)
            assert np.array_equal(sw["beta"], ss["beta"]) and sw["alpha"] == ss["alpha"]
            assert (sw["tau"], sw["sig2"]) == (ss["tau"], ss["sig2"])
            assert sw["alpha"] == tw["alpha"][-1] and np.std(tw["alpha"]) > 0
            assert bat[0].error_flags(c) == 0 and bat[1].error_flags(c) == 0
    finally:
        for h in hs:
            h.close()


# ---- 3. the first sweeps free-running against the oracle ----
@pytest.mark.parametrize("ortho", [False, True], ids=["general", "ortho"])
def test_first_sweeps_match_oracle(gpu_lib, ortho):
    """tests/test_triangle_gpu.py::test_tri_chain_matches_oracle under the key: sweeps 0-3 of
    bridge_reg_tri(nsamp=8, burn=0, alpha=0) at its bars."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 20, seed=5)
    e = None
    with fused_tri_alpha(bb):
        try:
            # the engine the call below creates from this design under the key is fused
            e = bb.Engine(tri_config(bb, 100, 20, ortho=ortho), X, y)
            assert_fused(bb, e)
            basis = e.tri_basis()
        finally:
            if e is not None:
                e.close()
        bb.set_seed(4321)
        g = bb.bridge_reg_tri(y, X, nsamp=8, burn=0, alpha=0.0, extras=True, ortho=ortho, **PRIOR)
    o = gibbs.bridge_regression_tri(y, X, 8, basis, burn=0, seed=4321, stream=0, true_alpha=0.0,
                                    ortho=ortho, **PRIOR)
    assert np.array_equal(g["shape"], o["shape"])
    for s in range(4):
        l2 = rel_l2(g["beta"][s], o["beta"][s])
        assert l2 < 1e-9, (s, l2)
    for k in ("sig2", "tau", "alpha"):
        assert rel(g[k][1:4], o[k][1:4]) < 1e-9, k


# ---- 4. batch == sequential calls, bitwise, key on ----
def test_batch_equals_sequential_calls(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(80, 12, seed=3)
    K = 3
    kw = dict(nsamp=120, burn=40, alpha=0.0, **PRIOR)
    with fused_tri_alpha(bb):
        # the call below runs the batch kernel, not the chains one after another: the batch of
        # this design exists under the key (bb_chains_create's rule is the call's)
        b = bb.ChainBatch(tri_config(bb, 80, 12), K, X, y)
        try:
            assert b.nchains == K and b.resident_per_cu() >= 1
        finally:
            b.close()
        bb.set_seed(SEED + 4)
        g = bb.bridge_reg_tri_chains(y, X, nchains=K, **kw)
        assert bb.get_rng_state() == (SEED + 4, K)
        singles = sequential(bb, y, X, K, SEED + 4, **kw)
        assert bb.get_rng_state() == (SEED + 4, K)
    for c in range(K):
        assert_chain_equal(g, c, singles[c])
    assert not np.array_equal(g["alpha"][0], g["alpha"][1])
    assert not np.array_equal(g["alpha"][1], g["alpha"][2])
    assert np.all((g["alpha"] > 0) & (g["alpha"] <= 1))
    assert np.all(g["alpha"].std(axis=1) > 0)


# ---- 5. the narrow instances ----
@pytest.mark.parametrize("case", ["general", "ortho", "x_in_memory"])
def test_instances_agree_bitwise(gpu_lib, case):
    """tests/test_tri_chains_gpu.py::test_instances_agree_bitwise with alpha sampled: the alpha
    step is wave 0's alone, so the 256- and 128-thread instances give the 512-thread one's
    bits."""
    bb = gpu_lib
    if case == "ortho":
        X, y = ortho_problem()
    else:
        X, y, _ = synthetic_problem(*((400, 32) if case == "x_in_memory" else (90, 17)))
    n, p = X.shape
    got = []
    for threads in (512, 256, 128):
        with fused_tri_alpha(bb):
            b = bb.ChainBatch(tri_config(bb, n, p, seed=SEED + 5, stream=3, trace_capacity=8,
                                         ortho=case == "ortho"), 3, X, y)
        try:
            b.set_threads(threads)
            assert b.threads() == threads and b.resident_per_cu() >= 1
            b.init_state()
            b.run(1, 7, 1, 1, 1)
            b.sync()
            assert all(b.error_flags(c) == 0 for c in range(3))
            got.append([(b.trace(c, 0, 8), b.tri_trace(c, 0, 8), b.state(c)) for c in range(3)])
            with pytest.raises(RuntimeError):
                b.set_threads(96)
        finally:
            b.close()
    for c in range(3):
        assert np.std(got[0][c][0]["alpha"]) > 0
    for narrow in got[1:]:
        for (t5, r5, s5), (t1, r1, s1) in zip(got[0], narrow):
            for key in TRACE_KEYS:
                assert np.array_equal(t5[key], t1[key]), key
            for key in ("u", "shape"):
                assert np.array_equal(r5[key], r1[key]), key
            assert s5["alpha"] == s1["alpha"]


# ---- 6. more chains than can be resident ----
def test_more_chains_than_resident(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(50, 6)
    K = bb.compute_units() + 4
    kw = dict(nsamp=10, burn=5, alpha=0.0, **PRIOR)
    with fused_tri_alpha(bb):
        bb.set_seed(SEED + 6)
        g = bb.bridge_reg_tri_chains(y, X, nchains=K, **kw)
        assert bb.get_rng_state() == (SEED + 6, K)
        for c in (0, 1, K - 5, K - 4, K - 1):
            bb.set_rng_state(SEED + 6, c)
            assert_chain_equal(g, c, bb.bridge_reg_tri(y, X, extras=True, **kw))
    for key in KEYS:
        assert np.all(np.isfinite(g[key])), key


# ---- 7 / 8. ChainBatch: teacher forcing and failure isolation ----
def fresh_batch(bb, X, y, K, stream=5):
    n, p = X.shape
    b = bb.ChainBatch(tri_config(bb, n, p, trace_capacity=2, seed=SEED + 7, stream=stream), K, X,
                      y)
    b.init_state()
    return b


def test_chain_batch_teacher_forcing(gpu_lib):
    """One sweep from a forced state with alpha = 0.37: batch chain 1 against a fused engine
    (bitwise) and against an engine created with the key off, which runs and keeps the general
    path (alpha exactly -- both decide on the same proposal and uniform --, the rest within
    1e-10: one sweep's summation-order differences)."""
    bb = gpu_lib
    n, p, K = 100, 13, 3
    X, y, _ = synthetic_problem(n, p)
    cfg1 = tri_config(bb, n, p, trace_capacity=2, seed=SEED + 7, stream=6)
    base = forced = eng = gen = None
    try:
        with fused_tri_alpha(bb, False):
            gen = bb.Engine(cfg1, X, y)
        with fused_tri_alpha(bb):
            base = fresh_batch(bb, X, y, K)
            forced = fresh_batch(bb, X, y, K)
            eng = bb.Engine(cfg1, X, y)
        # key restored: what exists keeps the path it was created with
        assert_fused(bb, eng)
        assert_fused(bb, gen, False)
        s0, e0, g0 = base.state(1), eng.state(), gen.state()
        assert np.array_equal(s0["beta"], e0["beta"]) and np.array_equal(s0["beta"], g0["beta"])
        assert (s0["tau"], s0["sig2"], s0["alpha"]) == (e0["tau"], e0["sig2"], e0["alpha"])
        assert (s0["tau"], s0["sig2"], s0["alpha"]) == (g0["tau"], g0["sig2"], g0["alpha"])
        beta = np.linspace(-1.0, 2.0, p)
        u = np.linspace(0.1, 0.7, p)
        forced.set_state(1, beta, 0.7, 1.3, 0.37)
        forced.set_tri_state(1, u)
        want = {}
        for name, e in (("fused", eng), ("general", gen)):
            e.set_state(beta, 0.7, 1.3, 0.37)
            e.set_tri_state(u)
            e.run(1, 1, 1, 1, 1)
            e.sync()
            assert e.error_flags() == 0, name
            want[name] = e.trace(1, 1)
            want[name].update(e.tri_trace(1, 1))
        tr_b, st_b = one_sweep(base, K)
        tr_f, st_f = one_sweep(forced, K)
        for key in SWEEP_KEYS:
            assert np.array_equal(tr_f[1][key], want["fused"][key]), key
        assert np.array_equal(st_f[1]["beta"], eng.state()["beta"])
        assert st_f[1]["alpha"] == eng.state()["alpha"] == tr_f[1]["alpha"][0]
        assert np.array_equal(tr_f[1]["alpha"], want["general"]["alpha"])
        assert abs(tr_f[1]["alpha"][0] - 0.37) <= 0.1
        assert np.array_equal(tr_f[1]["shape"], want["general"]["shape"])
        for key in ("beta", "lambda", "u"):
            err = rel_l2(tr_f[1][key], want["general"][key])
            print(f"{key}: rel L2 against the general path = {err:.3e}")
            assert err < TOL, (key, err)
        for key in ("tau", "sig2"):
            assert rel(tr_f[1][key], want["general"][key]) < TOL, key
        assert not np.array_equal(tr_f[1]["beta"], tr_b[1]["beta"])
        for c in (0, 2):
            for key in SWEEP_KEYS:
                assert np.array_equal(tr_f[c][key], tr_b[c][key]), (c, key)
            assert np.array_equal(st_f[c]["beta"], st_b[c]["beta"])
            assert st_f[c]["alpha"] == st_b[c]["alpha"]
    finally:
        for h in (base, forced, eng, gen):
            if h is not None:
                h.close()


def test_chain_batch_failure_isolation(gpu_lib):
    """tests/test_tri_chains_gpu.py::test_chain_batch_failure_isolation with alpha unknown: a
    NaN beta loses chain 2, whose error word alone is raised, at once, and the other chains draw
    what they would have."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K = 4
    base = bad = None
    with fused_tri_alpha(bb):
        try:
            base = fresh_batch(bb, X, y, K)
            bad = fresh_batch(bb, X, y, K)
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
                assert st_x[c]["alpha"] == st_b[c]["alpha"]
        finally:
            for h in (base, bad):
                if h is not None:
                    h.close()


# ---- 9. ring wrap and the summary call ----
def test_ring_wrap_equals_unwrapped(gpu_lib):
    bb = gpu_lib
    n, p, K, nsamp = 100, 13, 4, 120
    X, y, _ = synthetic_problem(n, p)
    kw = dict(nsamp=nsamp, nchains=K, burn=40, alpha=0.0, **PRIOR)
    with fused_tri_alpha(bb):
        bb.set_seed(SEED + 9)
        whole = bb.bridge_reg_tri_chains(y, X, **kw)
        assert bb.last_call_info()["trace_capacity"] == nsamp
        # a slot holds the four traced P-vectors and three scalars; the budget bounds the batch
        per_slot = 4 * p * 8 + 3 * 8
        try:
            bb.set_trace_budget(K * 37 * per_slot)
            bb.set_seed(SEED + 9)
            wrapped = bb.bridge_reg_tri_chains(y, X, **kw)
            assert bb.last_call_info()["trace_capacity"] == 37
        finally:
            bb.set_trace_budget(0)
    for key in KEYS:
        assert np.array_equal(wrapped[key], whole[key]), key
    assert np.all(whole["alpha"].std(axis=1) > 0)


def test_summary_call(gpu_lib):
    bb = gpu_lib
    n, p, K = 100, 13, 3
    X, y, _ = synthetic_problem(n, p)
    kw = dict(nsamp=120, nchains=K, burn=40, alpha=0.0, **PRIOR)
    with fused_tri_alpha(bb):
        bb.set_seed(SEED + 10)
        g = bb.bridge_reg_tri_chains(y, X, **kw)
        bb.set_seed(SEED + 10)
        s = bb.bridge_reg_tri_chains_summary(y, X, **kw)
        assert bb.get_rng_state() == (SEED + 10, K)
    check_against_trace_call(bb, s, g, K, f"triangle, alpha sampled {n}x{p}")
    assert np.all(s["chain_var"][:, p + 2] > 0)


# ---- 10. the switch ----
def test_switch(gpu_lib):
    bb = gpu_lib
    L = bb.library()
    X, y, _ = synthetic_problem(80, 33, seed=3)

    def create(cfg, K, Xa):
        h = ctypes.c_void_p()
        c = cfg.to_c()
        Xf = np.asfortranarray(Xa)
        rc = L.bb_chains_create(ctypes.byref(c), K, bb._p(Xf), bb._p(y[:cfg.n]), ctypes.byref(h))
        return rc, h.value, bb._err()

    Xs = np.asfortranarray(X[:, :12])
    kept = ref = None
    try:
        with fused_tri_alpha(bb, False):
            rc, h, msg = create(tri_config(bb, 80, 12), 2, Xs)
            assert rc == -1 and not h and "bb_chains_create" in msg and "alpha" in msg, msg
        with tuning(bb, k26=1), fused_tri_alpha(bb, False):
            # key 26 is the stable mixture's: it does not enable the triangle batch
            rc, h, msg = create(tri_config(bb, 80, 12), 2, Xs)
            assert rc == -1 and not h and "alpha" in msg, msg
        with fused_tri_alpha(bb):
            # outside the accepted shapes nothing changes: the messages are those of alpha known
            rc, h, msg = create(tri_config(bb, 80, 33), 2, X)
            assert rc == -1 and not h and "p <= 32" in msg, msg
            rc, h, msg = create(tri_config(bb, 10, 12), 2, Xs[:10])
            assert rc == -1 and not h and "p <= n" in msg, msg
            kept = fresh_batch(bb, Xs, y, 2)
            ref = fresh_batch(bb, Xs, y, 2)
            assert kept.resident_per_cu() >= 1 and kept.threads() == 512
            tr_ref, st_ref = one_sweep(ref, 2)
        # the key is back at 0: a new batch is refused, the one created under it keeps its kernel
        assert bb.set_tuning(TRI_ALPHA_KEY, -1) == 0
        with pytest.raises(RuntimeError):
            bb.ChainBatch(tri_config(bb, 80, 12), 2, Xs, y)
        tr_kept, st_kept = one_sweep(kept, 2)
        for c in range(2):
            for key in SWEEP_KEYS:
                assert np.array_equal(tr_kept[c][key], tr_ref[c][key]), (c, key)
            assert np.array_equal(st_kept[c]["beta"], st_ref[c]["beta"])
            assert st_kept[c]["alpha"] == tr_kept[c]["alpha"][0]  # one MH step from 0.5
            assert abs(st_kept[c]["alpha"] - 0.5) <= 0.1
    finally:
        for b in (kept, ref):
            if b is not None:
                b.close()
