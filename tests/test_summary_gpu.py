"""GPU tests of the summary mode: posterior summaries of chain batches reduced on the device
(bb_summary.hip k_trace_summary, bb_chains_summary_*, bridge_reg_stable_chains_summary,
bridge_regression_chains_summary).

The sampling kernels are not touched, so a summary call under the same key runs bit for bit the
chains of the trace call; the summaries are therefore checked against moments computed in
np.longdouble from the returned traces, and the kernel alone (bb.trace_summary) against
synthetic data.  Tolerances (a running fp64 sum of M <= 3000 products, started within a few sd
of the mean: error <= M 2^-53 (1 + (mean - x0)^2 / var) var):
  acov   |d| <= 1e-11 acov_0          mean   |d| <= 1e-12 sd + 2 ulp(|mean|)
  var, hvar  1e-11 relative           R-hat  1e-10 absolute        ESS  1e-8 relative
"""
import ctypes

import numpy as np
import pytest

from bayesbridge_amd import diagnostics as dg
from tests.conftest import synthetic_problem
from tests.test_chains_gpu import ortho_problem

pytestmark = pytest.mark.gpu

SEED = 0xB4E5B41D6E
RAW = ("mean", "var", "acov", "hmean", "hvar")


# ---------------------------------------------------------------------------
# references and comparisons
# ---------------------------------------------------------------------------
def ref_summary(x, L):
    """mean, var, acov[0..L], hmean, hvar of x (K, M, Q) in extended precision."""
    x = np.asarray(x, dtype=np.longdouble)
    K, M, Q = x.shape
    xc = x - x.mean(axis=1, keepdims=True)
    acov = np.zeros((K, Q, L + 1), dtype=np.longdouble)
    for k in range(min(L, M - 1) + 1):
        acov[:, :, k] = (xc[:, k:] * xc[:, :M - k]).sum(axis=1) / M
    n = M // 2
    out = {"mean": x.mean(axis=1), "acov": acov,
           "var": (xc * xc).sum(axis=1) / (M - 1) if M > 1 else np.full((K, Q), np.nan)}
    hm, hv = [], []
    for h in (x[:, :n], x[:, M - n:]):
        hc = h - h.mean(axis=1, keepdims=True) if n else h
        hm.append(h.mean(axis=1) if n else np.full((K, Q), np.nan))
        hv.append((hc * hc).sum(axis=1) / (n - 1) if n > 1 else np.full((K, Q), np.nan))
    out["hmean"], out["hvar"] = np.stack(hm, axis=-1), np.stack(hv, axis=-1)
    return out


def mean_tol(sd, mean):
    return 1e-12 * np.asarray(sd, dtype=np.float64) + 2 * np.spacing(np.abs(np.asarray(
        mean, dtype=np.float64)))


def assert_summary_close(got, ref, what=""):
    """got (the device's raw arrays) against ref_summary within the documented tolerances; the
    figures are printed before they are asserted."""
    r0 = ref["acov"][:, :, :1]
    sd = np.sqrt(np.asarray(ref["acov"][:, :, 0], dtype=np.float64))
    d_acov = np.abs(got["acov"] - ref["acov"])
    d_mean = np.abs(got["mean"] - ref["mean"])
    print(f"{what}: max |d acov| / acov0 = {float(np.max(d_acov / np.maximum(r0, 1e-300))):.3e}, "
          f"max |d mean| / sd = {float(np.max(d_mean / np.maximum(sd, 1e-300))):.3e}")
    assert np.all(d_acov <= 1e-11 * r0), what
    assert np.all(d_mean <= mean_tol(sd, ref["mean"])), what
    for key in ("var", "hvar"):
        ok = np.isfinite(np.asarray(ref[key], dtype=np.float64))
        rel = np.abs(got[key][ok] - ref[key][ok])
        print(f"{what}: max rel d {key} = "
              f"{float(np.max(rel / np.maximum(ref[key][ok], 1e-300), initial=0.0)):.3e}")
        assert np.all(rel <= 1e-11 * ref[key][ok]), (what, key)
        assert np.all(np.isnan(got[key][~ok])), (what, key)
    ok = np.isfinite(np.asarray(ref["hmean"], dtype=np.float64))
    hsd = np.sqrt(np.asarray(np.where(np.isfinite(np.asarray(ref["hvar"], dtype=np.float64)),
                                      ref["hvar"], 0), dtype=np.float64))
    assert np.all((np.abs(got["hmean"] - ref["hmean"]) <= mean_tol(hsd, ref["hmean"]))[ok]), what
    assert np.all(np.isnan(got["hmean"][~ok])), what


def assert_bitwise(a, b, what=""):
    for key in RAW:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


def ar1(rng, phi, M, mean=0.0):
    x = np.zeros(M)
    x[0] = rng.standard_normal() / np.sqrt(1.0 - phi * phi)
    for t in range(1, M):
        x[t] = phi * x[t - 1] + rng.standard_normal()
    return x + mean


def synthetic(K, M, Q, seed):
    """Columns cycle through: AR(1) phi = 0.6 with mean 300; phi = 0.95; iid with mean 1e4 and
    sd 1; a constant; phi = -0.4."""
    rng = np.random.default_rng(seed)
    make = [lambda: ar1(rng, 0.6, M, 300.0), lambda: ar1(rng, 0.95, M),
            lambda: 1e4 + rng.standard_normal(M), lambda: np.full(M, 2.75),
            lambda: ar1(rng, -0.4, M)]
    return np.stack([np.stack([make[q % 5]() for q in range(Q)], axis=1) for _ in range(K)])


# ---------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def values_case():
    x = synthetic(3, 257, 5, seed=11)
    return x, ref_summary(x, 24)


def test_kernel_values_and_chunking(gpu_lib, values_case):
    bb = gpu_lib
    x, ref = values_case
    whole = bb.trace_summary(x, 24)
    assert whole["mean"].shape == (3, 5) and whole["acov"].shape == (3, 5, 25)
    assert whole["hmean"].shape == whole["hvar"].shape == (3, 5, 2)
    assert_summary_close(whole, ref, "K3 M257 Q5")
    # the constant column: exactly its value, no variance, no covariance
    assert np.all(whole["mean"][:, 3] == 2.75) and np.all(whole["var"][:, 3] == 0.0)
    assert np.all(whole["acov"][:, 3] == 0.0) and np.all(whole["hvar"][:, 3] == 0.0)
    for chunk in (1, 7, 100):
        assert_bitwise(bb.trace_summary(x, 24, chunk=chunk), whole, f"chunk {chunk}")


@pytest.mark.parametrize("K,M,Q,L,chunk", [
    (2, 5, 5, 4, 2),      # every lag has a single product at most
    (2, 3, 5, 10, None),  # lags >= M are zero
    (2, 64, 5, 63, 9),    # all 64 lanes, M = maxlag + 1
    (2, 130, 5, 0, 64),   # variance only
    (1, 70, 1, 5, 33),    # one wave
    (2, 70, 35, 6, 64),   # more than one parameter tile, a partial last one
    (300, 40, 9, 8, 13),  # more waves than are resident
], ids=["M5L4", "M3L10", "M64L63", "L0", "Q1K1", "Q35", "K300"])
def test_kernel_edges(gpu_lib, K, M, Q, L, chunk):
    bb = gpu_lib
    x = synthetic(K, M, Q, seed=100 + M + Q)
    got = bb.trace_summary(x, L, chunk=chunk)
    assert got["acov"].shape == (K, Q, L + 1)
    assert_summary_close(got, ref_summary(x, L), f"K{K} M{M} Q{Q} L{L}")
    if L >= M:
        assert np.all(got["acov"][:, :, M:] == 0.0)
    assert_bitwise(bb.trace_summary(x, L), got, "one chunk")
    # the number of chains and the grid do not enter: chain 0 alone gives chain 0's bits
    alone = bb.trace_summary(x[:1], L, chunk=chunk)
    for key in RAW:
        assert np.array_equal(alone[key][0], got[key][0], equal_nan=True), key


def test_kernel_nan_isolation(gpu_lib, values_case):
    bb = gpu_lib
    x, _ = values_case
    clean = bb.trace_summary(x, 24, chunk=50)
    bad = x.copy()
    bad[1, 10, 2] = np.nan  # chain 1, parameter 2, a sample of the first half
    got = bb.trace_summary(bad, 24, chunk=50)
    for key in ("mean", "var", "acov"):
        assert np.all(np.isnan(got[key][1, 2])), key
    assert np.isnan(got["hmean"][1, 2, 0]) and np.isnan(got["hvar"][1, 2, 0])
    # the half without the sample keeps its bits, and so does every other entry
    keep = np.ones((3, 5), dtype=bool)
    keep[1, 2] = False
    for key in RAW:
        assert np.array_equal(got[key][keep], clean[key][keep]), key
    for key in ("hmean", "hvar"):
        assert got[key][1, 2, 1] == clean[key][1, 2, 1], key


# ---------------------------------------------------------------------------
# through the entries
# ---------------------------------------------------------------------------
def stack_traces(g):
    """(K, M, Q) of a trace call: beta, sig2, tau, alpha."""
    return np.concatenate([g["beta"], g["sig2"][:, :, None], g["tau"][:, :, None],
                           g["alpha"][:, :, None]], axis=2)


def raw_of(s):
    return {"mean": s["chain_mean"], "var": s["chain_var"], "acov": s["acov"],
            "hmean": s["hmean"], "hvar": s["hvar"]}


def check_against_trace_call(bb, s, g, K, what):
    """The summary call s against the trace call g of the same key."""
    x = stack_traces(g)
    _, M, Q = x.shape
    assert s["names"] == [f"beta{j + 1}" for j in range(Q - 3)] + ["sig2", "tau", "alpha"]
    assert s["maxlag"] == min(63, dg.default_maxlag(M)) and s["nsamp"] == M
    assert s["chain_mean"].shape == (K, Q) and s["acov"].shape == (K, Q, s["maxlag"] + 1)
    assert_summary_close(raw_of(s), ref_summary(x, s["maxlag"]), what)
    assert s["flags"].shape == (K,) and np.all(s["flags"] == 0)
    assert s["runtime"] > 0 and s["chains"] == K
    want = dg.sum_stat_chains(g["beta"], s["runtime"])
    sd = want["sd"]
    print(f"{what}: max rel d ess = {np.max(np.abs(s['ess'] - want['ess']) / want['ess']):.3e}, "
          f"max d rhat = {np.max(np.abs(s['rhat'] - want['rhat'])):.3e}")
    assert np.all(np.abs(s["mean"] - want["mean"]) <= mean_tol(sd, want["mean"]))
    assert np.all(np.abs(s["sd"] - sd) <= 1e-11 * sd)
    assert np.all(np.abs(s["ess"] - want["ess"]) <= 1e-8 * want["ess"])
    assert np.all(np.abs(s["rhat"] - want["rhat"]) <= 1e-10)
    assert np.allclose(s["esr"], s["ess"] / s["runtime"], rtol=1e-15)


@pytest.mark.parametrize("n,p,kw", [
    (100, 13, {}),
    (120, 15, dict(ortho=True)),
    (100, 13, dict(sig2_true=1.5)),
], ids=["100x13", "ortho120x15", "sig2_known"])
def test_stable_batch_summary(gpu_lib, n, p, kw):
    """nsamp = 120 and burn = 60 cross the 50-sweep block and the 32-sweep pre-draw bounds."""
    bb = gpu_lib
    X, y = ortho_problem() if kw.get("ortho") else synthetic_problem(n, p)[:2]
    K = 5
    bb.set_seed(SEED + 21)
    g = bb.bridge_reg_stb_chains(y, X, nsamp=120, nchains=K, burn=60, **kw)
    bb.set_seed(SEED + 21)
    s = bb.bridge_reg_stb_chains_summary(y, X, nsamp=120, nchains=K, burn=60, **kw)
    assert bb.get_rng_state() == (SEED + 21, K)
    check_against_trace_call(bb, s, g, K, f"stable {n}x{p} {kw}")
    if "sig2_true" in kw:  # a known parameter is a constant trace: no variance, ESS 0
        q = p
        assert np.all(s["chain_mean"][:, q] == 1.5) and np.all(s["chain_var"][:, q] == 0.0)
        assert np.all(dg.effective_size_from_acov(120, s["acov"][:, q]) == 0.0)
    # alpha is known here
    assert np.all(s["chain_mean"][:, p + 2] == 0.5) and np.all(s["chain_var"][:, p + 2] == 0.0)


def test_ring_wrap_equals_unwrapped(gpu_lib):
    bb = gpu_lib
    n, p, K, nsamp = 100, 13, 4, 120
    X, y, _ = synthetic_problem(n, p)
    bb.set_seed(SEED + 22)
    whole = bb.bridge_reg_stb_chains_summary(y, X, nsamp=nsamp, nchains=K, burn=60)
    assert bb.last_call_info()["trace_capacity"] == nsamp
    per_slot = 2 * p * 8 + 3 * 8
    try:
        bb.set_trace_budget(K * 37 * per_slot)
        bb.set_seed(SEED + 22)
        wrapped = bb.bridge_reg_stb_chains_summary(y, X, nsamp=nsamp, nchains=K, burn=60)
        assert bb.last_call_info()["trace_capacity"] == 37
    finally:
        bb.set_trace_budget(0)
    assert_bitwise(raw_of(wrapped), raw_of(whole), "capacity 37")
    assert np.array_equal(wrapped["flags"], whole["flags"])


def test_triangle_batch_summary(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K = 3
    bb.set_seed(SEED + 23)
    g = bb.bridge_reg_tri_chains(y, X, nsamp=120, nchains=K, burn=60)
    bb.set_seed(SEED + 23)
    s = bb.bridge_reg_tri_chains_summary(y, X, nsamp=120, nchains=K, burn=60)
    assert bb.get_rng_state() == (SEED + 23, K)
    check_against_trace_call(bb, s, g, K, "triangle 100x13")


@pytest.mark.parametrize("n,p,K,kw", [
    (60, 40, 3, dict(nsamp=40, burn=20)),
    (80, 12, 2, dict(nsamp=40, burn=20, alpha=0.0)),
    (40, 96, 2, dict(nsamp=30, burn=10)),
], ids=["p40", "alpha_mh", "woodbury40x96"])
def test_fallback_summary(gpu_lib, n, p, K, kw):
    """Designs a chain batch does not take: the chains run one after another, each single
    engine's ring reduced by the same kernel."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(n, p, seed=3)
    bb.set_seed(SEED + 24)
    g = bb.bridge_reg_stb_chains(y, X, nchains=K, **kw)
    bb.set_seed(SEED + 24)
    s = bb.bridge_reg_stb_chains_summary(y, X, nchains=K, **kw)
    assert bb.get_rng_state() == (SEED + 24, K)
    check_against_trace_call(bb, s, g, K, f"fallback {n}x{p}")
    if kw.get("alpha") == 0.0:  # alpha is sampled: its summary is that of a moving trace
        assert np.all(s["chain_var"][:, p + 2] > 0)


def fresh_batch(bb, X, y, K, cap):
    n, p = X.shape
    cfg = bb.EngineConfig(n=n, p=p, trace_capacity=cap, seed=SEED + 25, stream=5)
    b = bb.ChainBatch(cfg, K, X, y)
    b.init_state()
    return b


def test_chain_batch_summary_pieces(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K, M, L = 3, 90, 12
    one = fresh_batch(bb, X, y, K, cap=M)
    two = fresh_batch(bb, X, y, K, cap=60)  # its second piece wraps the ring
    try:
        one.run(1, M - 1, 1, 1, 1)
        one.summary_reset(M, L)
        one.summary_add(0, M, 0)
        a = one.summary()
        two.summary_reset(M, L)
        two.run(1, 49, 1, 1, 1)
        two.summary_add(0, 50, 0)
        two.run(50, 40, 50, 1, 1)
        two.summary_add(50, 40, 50)
        b = two.summary()
        assert_bitwise(a, b, "pieces of 50 and 40")
        assert np.all(a["flags"] == 0) and np.all(b["flags"] == 0)
        tr = [one.trace(c, 0, M) for c in range(K)]
        x = np.stack([np.concatenate([t["beta"].T, t["sig2"][:, None], t["tau"][:, None],
                                      t["alpha"][:, None]], axis=1) for t in tr])
        assert_summary_close(a, ref_summary(x, L), "ChainBatch 90 samples")
        # out of order, too many, before all are in
        with pytest.raises(RuntimeError, match="in order"):
            one.summary_add(0, 1, 0)
        two.summary_reset(M, L)
        with pytest.raises(RuntimeError, match="samples added"):
            two.summary()
    finally:
        one.close()
        two.close()


def test_chain_batch_summary_failure_isolation(gpu_lib):
    """A NaN beta makes chain 2 fail (as test_chain_batch_failure_isolation): only its
    summaries and its flag differ."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(100, 13)
    K, M, L = 4, 30, 6
    base = fresh_batch(bb, X, y, K, cap=M)
    bad = fresh_batch(bb, X, y, K, cap=M)
    try:
        st = bad.state(2)
        bad.set_state(2, np.full(13, np.nan), st["tau"], st["sig2"], st["alpha"])
        out = []
        for b in (base, bad):
            b.summary_reset(M, L)
            b.run(1, M - 1, 1, 1, 1)
            b.summary_add(0, M, 0)
            out.append(b.summary())
        good, got = out
        assert np.all(good["flags"] == 0)
        assert got["flags"][2] != 0 and np.all(got["flags"][[0, 1, 3]] == 0)
        for key in RAW:
            assert np.array_equal(got[key][[0, 1, 3]], good[key][[0, 1, 3]]), key
        assert not np.array_equal(got["mean"][2], good["mean"][2], equal_nan=True)
    finally:
        base.close()
        bad.close()


def call_stable_summary(bb, y, X, M, K, maxlag, burn=5):
    """.C("bridge_reg_stable_chains_summary", ...) itself, outputs prefilled with a marker."""
    L = bb.library()
    P = X.shape[1]
    lag = min(max(maxlag, 0), 63)
    out = [np.full(s, -7.0) for s in ((max(K, 1), P + 3), (max(K, 1), P + 3),
                                      (max(K, 1), P + 3, lag + 1), (max(K, 1), P + 3, 2),
                                      (max(K, 1), P + 3, 2))]
    flags = np.full(max(K, 1), -7, dtype=np.int32)
    d = lambda v: ctypes.byref(ctypes.c_double(float(v)))  # noqa: E731
    i = lambda v: ctypes.byref(ctypes.c_int(int(v)))  # noqa: E731
    rt = ctypes.c_double(-7.0)
    Xf = np.asfortranarray(X)
    L.bridge_reg_stable_chains_summary(
        *[bb._p(a) for a in out], flags.ctypes.data_as(bb._ip), i(maxlag), bb._p(y), bb._p(Xf),
        d(0.0), d(0.0), d(2.0), d(2.0), d(1.0), d(1.0), d(0.0), d(0.0), d(0.5), i(P),
        i(X.shape[0]), i(M), i(burn), ctypes.byref(rt), i(0), i(K))
    return out, flags, rt.value


def test_bad_arguments(gpu_lib):
    bb = gpu_lib
    X, y, _ = synthetic_problem(50, 6)
    for maxlag, K, word in ((64, 2, "maxlag"), (-1, 2, "maxlag"), (3, 0, "nchains")):
        bb.set_rng_state(SEED + 26, 4)
        out, flags, rt = call_stable_summary(bb, y, X, 10, K, maxlag)
        assert word in bb._err() and "bridge_reg_stable_chains_summary" in bb._err()
        assert bb.get_rng_state() == (SEED + 26, 4)  # no key taken
        assert all(np.all(a == -7.0) for a in out) and np.all(flags == -7) and rt == -7.0
    # the same call with good arguments writes everything and takes two keys
    bb.set_rng_state(SEED + 26, 4)
    out, flags, rt = call_stable_summary(bb, y, X, 10, 2, 3)
    assert bb.get_rng_state() == (SEED + 26, 6)
    assert all(np.all(np.isfinite(a)) and not np.any(a == -7.0) for a in out[:3])
    assert np.all(flags == 0) and rt > 0
    for maxlag in (64, -1):
        with pytest.raises(ValueError, match="maxlag"):
            bb.bridge_reg_stb_chains_summary(y, X, nsamp=10, nchains=2, burn=5, maxlag=maxlag)
        with pytest.raises(RuntimeError, match="maxlag"):
            bb.trace_summary(np.zeros((1, 8, 2)), maxlag)
    with pytest.raises(RuntimeError, match="samples"):
        bb.trace_summary(np.zeros((1, 0, 2)), 3)
    b = fresh_batch(bb, X, y, 2, cap=8)
    try:
        with pytest.raises(RuntimeError, match="maxlag"):
            b.summary_reset(8, 64)
        with pytest.raises(RuntimeError, match="before reset"):
            b.summary_add(0, 1, 0)
    finally:
        b.close()
