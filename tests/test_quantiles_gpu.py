"""GPU tests of the pooled quantile sketch (bb_quantile.hip k_trace_hist / k_quantile_select,
bb_chains_quantiles_*, the `_q` summary entries).

No tolerance appears: the histogram's bins are a fixed function of the bits of x - centre and
its counts are integers, so the brackets, the counts below and inside them and the sign counts
are compared bit for bit with numpy on draws the device did not bin (tests/quantile_ref.py) --
synthetic data for the kernels alone, and for the entries the traces of the trace call under the
same key, whose chains the summary call runs bit for bit."""
import numpy as np
import pytest

from tests import quantile_ref as qr
from tests.conftest import synthetic_problem

pytestmark = pytest.mark.gpu

SEED = 0xB4E5B41D6E
PROBS = qr.PROBS
MOMENTS = ("chain_mean", "chain_var", "acov", "hmean", "hvar", "flags")
QKEYS = ("centre", "zlo", "zhi", "below", "inbin", "counts")


# ---------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------
def synthetic():
    """(K, M, Q) = (3, 130, 9): two 64-slot chunks and a ragged third, one parameter past a
    tile of 8.  Columns: normal at 500 +- 60; at 1e-3 +- 1e-5; a constant; exact ties (chain
    0's first 70 equal to the centre, so its window is anchored late); both signs about 0;
    values at 2^-70 and 1e30 from a centre of 0 (zero and overflow bins) among ordinary ones
    over 20 octaves (in and out of the window); two NaNs and a +inf; a NaN centre; subnormals."""
    K, M, Q = 3, 130, 9
    rng = np.random.default_rng(20240917)
    x = np.zeros((K, M, Q))
    x[:, :, 0] = 500.0 + 60.0 * rng.standard_normal((K, M))
    x[:, :, 1] = 1e-3 + 1e-5 * rng.standard_normal((K, M))
    x[:, :, 2] = 2.75
    x[:, :, 3] = 1.0 + 0.25 * rng.integers(-2, 3, (K, M))
    x[0, :70, 3] = 1.25
    x[:, :, 4] = rng.standard_normal((K, M))
    pick = rng.integers(0, 6, (K, M))
    vals = np.array([2.0 ** -70, -2.0 ** -70, 1e30, -1e30])
    wide = rng.standard_normal((K, M)) * 2.0 ** rng.integers(-10, 10, (K, M))
    x[:, :, 5] = np.where(pick < 4, vals[np.minimum(pick, 3)], wide)
    x[0, 0, 5] = 0.0
    x[:, :, 6] = -3.0 + rng.standard_normal((K, M))
    x[0, 17, 6] = x[2, 129, 6] = np.nan
    x[1, 64, 6] = np.inf
    x[:, :, 7] = rng.standard_normal((K, M))
    x[0, 0, 7] = np.nan
    x[:, :, 8] = rng.integers(-1000, 1000, (K, M)) * 5e-324
    return x


@pytest.fixture(scope="module")
def kernel_case():
    x = synthetic()
    return x, qr.selection(x, PROBS)


def test_kernel_selection_is_exact(gpu_lib, kernel_case):
    bb = gpu_lib
    x, want = kernel_case
    K, M, Q = x.shape
    got = bb.trace_quantiles(x, PROBS)
    assert got["zlo"].shape == (Q, len(PROBS)) and got["counts"].shape == (Q, 6)
    qr.assert_selection_equal(got, want, "K3 M130 Q9")
    c = got["counts"]
    assert np.all(c[:, 0] + c[:, 1] == K * M)
    assert c[2, 4] == K * M                      # the constant column: all in the zero bin
    assert c[5, 4] > 0 and c[5, 5] > 0           # zero and overflow bins are populated
    assert c[6, 1] == 2 and c[6, 5] == 1         # two NaNs, one +inf
    assert c[7, 0] == 0 and c[7, 1] == K * M     # a NaN centre: every sample is a NaN
    assert np.all(np.isnan(got["zlo"][7])) and np.all(np.isnan(got["quantile"][7]))
    assert c[8, 4] == K * M                      # subnormals
    # the rank is inside its bin, the estimate inside its bracket
    live = c[:, 0] > 0
    k = np.minimum(c[:, :1], np.maximum(1, np.ceil(np.asarray(PROBS)[None] * c[:, :1])))
    assert np.all((got["below"] < k)[live] & (k <= got["below"] + got["inbin"])[live])
    fin = np.isfinite(got["quantile_lo"]) & np.isfinite(got["quantile_hi"])
    assert np.all((got["quantile_lo"] <= got["quantile"])[fin])
    assert np.all((got["quantile"] <= got["quantile_hi"])[fin])
    # against numpy's own order statistics (type 1: inverted_cdf)
    for q in (0, 1, 4):
        t1 = np.quantile(x[:, :, q].ravel(), PROBS, method="inverted_cdf")
        ulp = np.spacing(np.abs(t1))  # the bracket of x is centre + z edge: one rounding
        assert np.all((got["quantile_lo"][q] <= t1 + ulp) & (t1 - ulp <= got["quantile_hi"][q])), q
    assert np.array_equal(got["prob_pos"][:2], [1.0, 1.0]) and got["prob_neg"][6] > 0.9


@pytest.mark.parametrize("chunk", [1, 7, 64, 130])
def test_kernel_chunking_changes_nothing(gpu_lib, kernel_case, chunk):
    x, want = kernel_case
    qr.assert_selection_equal(gpu_lib.trace_quantiles(x, PROBS, chunk=chunk), want,
                              f"chunk {chunk}")


@pytest.mark.parametrize("K,M", [(1, 1), (3, 1), (1, 65), (3, 65)])
def test_kernel_small_shapes(gpu_lib, kernel_case, K, M):
    x = kernel_case[0][:K, :M]
    qr.assert_selection_equal(gpu_lib.trace_quantiles(x, PROBS, chunk=64),
                              qr.selection(x, PROBS), f"K{K} M{M}")


def test_kernel_beta_only_and_many_probs(gpu_lib, kernel_case):
    """Q <= 3 has no scalar rings; 64 probabilities are the most a call takes."""
    x = np.ascontiguousarray(kernel_case[0][:, :, [0, 4]])
    probs = np.linspace(0.0, 1.0, 64)
    qr.assert_selection_equal(gpu_lib.trace_quantiles(x, probs, chunk=50),
                              qr.selection(x, probs), "Q2 64 probs")


# ---------------------------------------------------------------------------
# through the entries
# ---------------------------------------------------------------------------
def stack_traces(g):
    """(K, M, Q) of a trace call: beta, sig2 (the constant 1 of a logistic call), tau, alpha."""
    sig2 = g["sig2"] if "sig2" in g else np.ones_like(g["tau"])
    return np.concatenate([g["beta"], sig2[:, :, None], g["tau"][:, :, None],
                           g["alpha"][:, :, None]], axis=2)


def logit_y(X, y):
    return (y > np.median(y)).astype(np.float64)


def run_pair(bb, kind, X, y, K, seed, **kw):
    """The trace call, the summary call and the summary call with probs under one key."""
    trace = {"stable": bb.bridge_reg_stb_chains, "tri": bb.bridge_reg_tri_chains,
             "logit": bb.bridge_reg_logit_chains}[kind]
    summ = {"stable": bb.bridge_reg_stb_chains_summary, "tri": bb.bridge_reg_tri_chains_summary,
            "logit": bb.bridge_reg_logit_chains_summary}[kind]
    out = []
    for f, extra in ((trace, {}), (summ, {}), (summ, dict(probs=PROBS))):
        bb.set_seed(seed)
        out.append(f(y, X, nsamp=130, nchains=K, burn=20, **kw, **extra))
        assert bb.get_rng_state() == (seed, K)
    return out


def check_pair(g, s, sq, K, P, what):
    x = stack_traces(g)
    assert x.shape == (K, 130, P + 3)
    want = qr.selection(x, PROBS)
    qr.assert_selection_equal(sq, want, what)
    assert np.array_equal(sq["probs"], PROBS)
    N = want["counts"][:, 0]
    assert np.all(N == K * 130)
    assert np.array_equal(sq["prob_pos"], want["counts"][:, 3] / N)
    assert np.array_equal(sq["prob_neg"], want["counts"][:, 2] / N)
    # the moment outputs and the flags are those of the call without probs
    for key in MOMENTS:
        assert np.array_equal(sq[key], s[key], equal_nan=True), (what, key)
    for key in QKEYS:
        assert key not in s
    # numpy's type-1 quantiles of the pooled draws lie in their brackets (exact in z; the
    # bracket of x is centre + z edge, one rounding)
    t1 = np.quantile(x.reshape(-1, P + 3), PROBS, axis=0, method="inverted_cdf").T
    assert np.all(sq["quantile_lo"] <= t1 + np.spacing(np.abs(t1))), what
    assert np.all(t1 - np.spacing(np.abs(t1)) <= sq["quantile_hi"]), what


@pytest.mark.parametrize("P", [1, 6])
def test_stable_batch_quantiles(gpu_lib, P):
    bb = gpu_lib
    X, y, _ = synthetic_problem(24, P, seed=31)
    g, s, sq = run_pair(bb, "stable", X, y, 3, SEED + 41)
    check_pair(g, s, sq, 3, P, f"stable 24x{P}")
    assert sq["counts"][P + 2, 4] == 3 * 130  # alpha is known: a constant column


@pytest.mark.parametrize("P", [1, 6])
def test_stable_fused_alpha_batch_quantiles(gpu_lib, P):
    bb = gpu_lib
    X, y, _ = synthetic_problem(24, P, seed=32)
    old = bb.set_fused_alpha(True)
    try:
        g, s, sq = run_pair(bb, "stable", X, y, 3, SEED + 42, alpha=0.0)
    finally:
        bb.set_fused_alpha(old)
    check_pair(g, s, sq, 3, P, f"stable fused alpha 24x{P}")
    assert sq["counts"][P + 2, 4] < 3 * 130  # the alpha column moves


@pytest.mark.parametrize("P", [1, 6])
def test_triangle_batch_quantiles(gpu_lib, P):
    bb = gpu_lib
    X, y, _ = synthetic_problem(24, P, seed=33)
    g, s, sq = run_pair(bb, "tri", X, y, 3, SEED + 43)
    check_pair(g, s, sq, 3, P, f"triangle 24x{P}")


@pytest.mark.parametrize("P", [1, 6])
def test_logit_batch_quantiles(gpu_lib, P):
    bb = gpu_lib
    X, y, _ = synthetic_problem(24, P, seed=34)
    g, s, sq = run_pair(bb, "logit", X, logit_y(X, y), 3, SEED + 44)
    check_pair(g, s, sq, 3, P, f"logit 24x{P}")
    assert sq["centre"][P] == 1.0 and sq["counts"][P, 4] == 3 * 130  # sig2 is the constant 1
    assert np.all(sq["quantile"][P] == 1.0)


@pytest.mark.parametrize("P", [1, 6])
def test_fallback_quantiles(gpu_lib, P):
    """alpha unknown and no key set: the chains run one after another, one sketch pools them
    about chain 0's first kept draw."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(24, P, seed=35)
    old = bb.set_fused_alpha(False)
    try:
        g, s, sq = run_pair(bb, "stable", X, y, 2, SEED + 45, alpha=0.0)
    finally:
        bb.set_fused_alpha(old)
    check_pair(g, s, sq, 2, P, f"fallback 24x{P}")
    assert sq["counts"][P + 2, 4] < 2 * 130


def test_ring_wrap_changes_nothing(gpu_lib):
    bb = gpu_lib
    P, K = 6, 3
    X, y, _ = synthetic_problem(24, P, seed=31)
    bb.set_seed(SEED + 46)
    whole = bb.bridge_reg_stb_chains_summary(y, X, nsamp=130, nchains=K, burn=20, probs=PROBS)
    assert bb.last_call_info()["trace_capacity"] == 130
    per_slot = 2 * P * 8 + 3 * 8
    try:
        bb.set_trace_budget(K * 37 * per_slot)
        bb.set_seed(SEED + 46)
        wrapped = bb.bridge_reg_stb_chains_summary(y, X, nsamp=130, nchains=K, burn=20,
                                                   probs=PROBS)
        assert bb.last_call_info()["trace_capacity"] == 37  # three wraps
    finally:
        bb.set_trace_budget(0)
    qr.assert_selection_equal(wrapped, whole, "capacity 37")
    for key in MOMENTS:
        assert np.array_equal(wrapped[key], whole[key], equal_nan=True), key


def test_chain_batch_quantile_steps(gpu_lib):
    """The step API: the sketch is fed by summary_add, in one piece or in wrapping pieces."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(24, 6, seed=31)
    K, M = 3, 90

    def fresh(cap):
        cfg = bb.EngineConfig(n=24, p=6, trace_capacity=cap, seed=SEED + 47, stream=5)
        b = bb.ChainBatch(cfg, K, X, y)
        b.init_state()
        return b

    one, two = fresh(M), fresh(60)
    try:
        one.run(1, M - 1, 1, 1, 1)
        one.summary_reset(M, 5)
        one.quantiles_reset()
        one.summary_add(0, M, 0)
        a = one.quantiles(PROBS)
        tr = [one.trace(c, 0, M) for c in range(K)]
        x = np.stack([np.concatenate([t["beta"].T, t["sig2"][:, None], t["tau"][:, None],
                                      t["alpha"][:, None]], axis=1) for t in tr])
        qr.assert_selection_equal(a, qr.selection(x, PROBS), "ChainBatch 90 samples")
        # another selection from the same sketch
        qr.assert_selection_equal(one.quantiles([0.1, 0.9]), qr.selection(x, [0.1, 0.9]), "again")
        two.summary_reset(M, 5)
        two.quantiles_reset()
        two.run(1, 49, 1, 1, 1)
        two.summary_add(0, 50, 0)
        with pytest.raises(RuntimeError, match="samples added"):
            two.quantiles(PROBS)
        two.run(50, 40, 50, 1, 1)
        two.summary_add(50, 40, 50)
        qr.assert_selection_equal(two.quantiles(PROBS), a, "pieces of 50 and 40")
        with pytest.raises(RuntimeError, match="before the first"):
            two.quantiles_reset()
        two.summary_reset(M, 5)  # drops the sketch
        with pytest.raises(RuntimeError, match="before reset"):
            two.quantiles(PROBS)
    finally:
        one.close()
        two.close()


def test_refusals_leave_the_outputs_untouched(gpu_lib):
    bb = gpu_lib
    P, K, M = 3, 2, 10
    X, y, _ = synthetic_problem(24, P, seed=31)
    Q = P + 3

    def call(probs):
        n = len(probs)
        mark = lambda *s: np.full(s, -7.0)  # noqa: E731
        return bb.dot_c(
            "bridge_reg_stable_chains_summary_q", mark(K, Q), mark(K, Q), mark(K, Q, 4),
            mark(K, Q, 2), mark(K, Q, 2), np.full(K, -7), 3, y, np.asfortranarray(X).ravel("F"),
            0.0, 0.0, 2.0, 2.0, 1.0, 1.0, 0.0, 0.0, 0.5, P, 24, M, 5, -7.0, 0, K,
            np.asarray(probs, dtype=np.float64), n, mark(Q), mark(Q, n), mark(Q, n), mark(Q, n),
            mark(Q, n), mark(Q, 6))

    for probs, word in ((np.linspace(0, 1, 65), "at most 64"), ([0.5, 1.5], "[0, 1]"),
                        ([np.nan], "[0, 1]")):
        bb.set_rng_state(SEED + 48, 4)
        out = call(probs)
        err = bb._err()
        assert word in err and "bridge_reg_stable_chains_summary_q" in err, err
        assert bb.get_rng_state() == (SEED + 48, 4)  # no key taken
        for a in out[:6] + out[27:]:
            assert np.all(a == -7), a
        assert out[22][0] == -7.0  # runtime
    # the same call with good probabilities writes everything and takes two keys
    bb.set_rng_state(SEED + 48, 4)
    out = call([0.025, 0.975])
    assert bb.get_rng_state() == (SEED + 48, 6)
    assert np.all(np.isfinite(out[0])) and np.all(out[5] == 0) and out[22][0] > 0
    assert np.all(np.isfinite(out[27])) and np.all(out[28] < out[29])
    assert np.all(out[32][:, 0] == K * M)
    # the sketch counts in 32 bits: K M = 2^32 is refused before x is read
    rc = bb.library().bb_trace_quantiles(bb._p(np.zeros(1)), 1 << 16, 1 << 16, 1, 1,
                                         bb._p(np.array([0.5])), 1, *[bb._p(np.zeros(1))] * 6)
    assert rc == -1 and "2^32" in bb._err()
