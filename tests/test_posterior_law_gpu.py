"""GPU tests: every chain kernel against the exact posterior laws of tests/posterior_law.py.

The other GPU tests of a sampler say "the device draws what the oracle draws on the same
counters".  These say "what the device draws follows the model's posterior", judged by a
reference that shares no code with the kernels or the oracle: quadrature targets (Q1 alpha
sampled, Q2 p = 2 with tau and sig2 unknown, Q3 sig2 alone unknown at small n) and the
integration-by-parts identities (S1) for the designs where quadrature is impossible.  The
cases, the verdicts (|z| <= 5 per scalar target, max |z| <= z_m per family of m identities) and
the three conditions that keep a pass from being empty (resolution, power, convergence) are
those of tests/posterior_law.py and tests/test_posterior_law_cpu.py; each condition is asserted
here.  Chain batches give K independent chains under the keys (seed, stream + c), so the
Monte-Carlo error is the between-chain spread of chain means.  The paths that run one chain per
call run a few chains one after another, each cut into consecutive batches that stand in for
chains (posterior_law.batches; the Stein cases assert the batches long against the measured
autocorrelation time).  The general alpha path (k_alpha_mh) alone has a resolution bound other
than 0.03: 0.03 scaled by sqrt(256 x 2000 / sweeps), the Monte-Carlo rate.  Before a batch call,
assert_batch_kernel pins that the batch kernel takes the design under the keys in force.

The last test reads the traces of the four batch kernels again for cross-chain independence:
chain keys (k0, k1 + c) and sweep counters that overlapped would correlate neighbouring chains
at some shift of the sweep index, which parity with an oracle sharing the counter scheme cannot
see.

Every test that sets a tuning key restores it in a finally.
"""
import math

import numpy as np
import pytest

from bayesbridge_amd.diagnostics import effective_size, rhat
from tests import posterior_law as pl
from tests.conftest import synthetic_problem
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

SEED = 0x9051E4
PACKED_KEY, WIDE_KEY, ALPHA_KEY = 21, 25, 26
K_BATCH, M_BATCH = 256, 2000
_traces = {}


def assert_converged(beta, what):
    r = float(np.max(rhat(beta)))
    print(f"{what}: split R-hat of beta over {beta.shape[0]} chains = {r:.4f}")
    assert r <= pl.RHAT_MAX, (what, r)


def scaled_resolution(sweeps):
    return pl.RESOLUTION * math.sqrt(K_BATCH * M_BATCH / sweeps)


def linear_bs(X, y, alpha=0.5, **kw):
    return lambda b, c: pl.bs_linear(b, X, y, alpha, **kw)


def conditional_bs(X, y, g, nb=1, alpha=0.5):
    """beta_j s_j given the traced tau and sig2 of the chain (or batch) c."""
    tau, sig2 = pl.batches(g["tau"], nb), pl.batches(g["sig2"], nb)
    return lambda b, c: pl.bs_linear(b, X, y, alpha, sig2=sig2[c], tau=tau[c])


def assert_batch_kernel(bb, X, y, K, threads=None, **cfg):
    """The .C chain calls run the chains one after another, through the general path, when the
    batch kernel refuses the design (bb_chains_create's rule).  So a ChainBatch of the same
    design and hyper-parameters, created under the same tuning keys, must exist, hold K chains
    and run the expected instance: a key that did not engage fails here instead of passing the
    law test through another kernel."""
    X = np.asfortranarray(X)
    n, p = X.shape
    b = bb.ChainBatch(bb.EngineConfig(n=n, p=p, seed=SEED, **cfg), K, X, y)
    try:
        assert b.nchains == K and b.resident_per_cu() >= 1
        if threads is not None:
            assert b.threads() == threads, (b.threads(), threads)
    finally:
        b.close()


def autocorr_time(beta, cols=None):
    """The largest integrated autocorrelation time, in sweeps, over the coefficients ``cols``
    of traces beta (K, M, p): M / (coda's effective size), averaged over the chains."""
    cols = np.arange(beta.shape[2]) if cols is None else np.asarray(cols)
    ess = np.mean([effective_size(b[:, cols]) for b in beta], axis=0)
    return float(beta.shape[1] / ess.min())


def assert_batches_long(what, beta, nb, cols=None):
    """Batch means stand in for chain means only if a batch is long against the autocorrelation
    time tau: the variance of a batch mean is short by about tau / length, so 20 tau keeps the
    s.e. within 2.5 %."""
    tau, length = autocorr_time(beta, cols), beta.shape[1] // nb
    print(f"{what}: autocorrelation time {tau:.1f} sweeps, batches of {length}")
    assert length >= 20.0 * tau, (what, tau, length)


def signal_swap(X):
    """The two most correlated of synthetic_problem's five signal columns."""
    return pl.most_correlated(X, among=5)


# ---------------------------------------------------------------------------------------
# the traces of the four batch kernels, kept for the independence test
# ---------------------------------------------------------------------------------------
def small_traces(bb):
    if "small" not in _traces:
        X, y = pl.s1_problem(60, 6)
        assert_batch_kernel(bb, X, y, K_BATCH, threads=512)
        bb.set_seed(SEED + 1)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=M_BATCH, nchains=K_BATCH)
        _traces["small"] = (X, y, {k: g[k] for k in ("beta", "tau", "sig2")})
    return _traces["small"]


def alpha_traces(bb, ortho, alpha_b):
    key = ("alpha", ortho, alpha_b)
    if key not in _traces:
        x, y, sig2, tau = pl.q1_data()
        with tuning(bb, k26=1):
            assert_batch_kernel(bb, x[:, None], y, K_BATCH, threads=512, true_alpha=0.0,
                                alpha_a=1.0, alpha_b=alpha_b, true_sig2=sig2, true_tau=tau,
                                ortho=ortho)
            bb.set_seed(SEED + 2)
            g = bb.bridge_reg_stb_chains(y, x[:, None], nsamp=M_BATCH, nchains=K_BATCH,
                                         alpha=0.0, alpha_a=1.0, alpha_b=alpha_b, sig2_true=sig2,
                                         tau_true=tau, ortho=ortho)
        _traces[key] = {k: g[k] for k in ("beta", "alpha")}
    return _traces[key]


def wide_traces(bb, n, p):
    key = ("wide", n, p)
    if key not in _traces:
        X, y, _ = synthetic_problem(n, p)
        with tuning(bb, k25=1):
            assert_batch_kernel(bb, X, y, 64, threads=256 if p <= 64 else None)
            bb.set_seed(SEED + 3)
            g = bb.bridge_reg_stb_chains(y, X, nsamp=1000, nchains=64)
        _traces[key] = (X, y, {k: g[k] for k in ("beta", "tau", "sig2")})
    return _traces[key]


def tri_traces(bb):
    if "tri" not in _traces:
        X, y, _ = synthetic_problem(100, 13)
        assert_batch_kernel(bb, X, y, 64, method=4)
        bb.set_seed(SEED + 4)
        g = bb.bridge_reg_tri_chains(y, X, nsamp=4000, nchains=64)
        _traces["tri"] = (X, y, {k: g[k] for k in ("beta", "tau", "sig2")})
    return _traces["tri"]


# ---------------------------------------------------------------------------------------
# small batch, 64-lane instance: Q2, Q3, S1 at 60 x 6
# ---------------------------------------------------------------------------------------
def q2_on_device(what, trace_call, summary_call, alpha):
    """Q2: the moments through the summary call (the trace-summary kernel in the loop), the
    product moment and R-hat through the trace call."""
    X, y = pl.q2_data()
    targets = pl.checked(pl.targets_2d, X, y, alpha)
    s = summary_call(y, X, alpha)
    assert not s["flags"].any()
    M = s["nsamp"]
    st = {}
    for j in range(2):
        st.update(pl.moment_stats_from_summary(s["chain_mean"][:, j], s["chain_var"][:, j], M,
                                               f"beta{j}", targets))
    g = trace_call(y, X, alpha)
    assert_converged(g["beta"], what)
    st["beta0beta1"] = pl.q2_stats(g["beta"], targets)["beta0beta1"]
    return pl.judge(what, st, targets, pl.Q2_NAMES)


@pytest.mark.parametrize("alpha", [0.5, 0.8])
def test_small_batch_q2(gpu_lib, alpha):
    bb = gpu_lib

    def call(fn):
        def run(y, X, a):
            bb.set_seed(SEED + 10)
            return fn(y, X, nsamp=M_BATCH, nchains=K_BATCH, alpha=a)
        return run

    assert_batch_kernel(bb, *pl.q2_data(), K_BATCH, threads=512, true_alpha=alpha)
    q2_on_device(f"small batch Q2 alpha={alpha}", call(bb.bridge_reg_stb_chains),
                 call(bb.bridge_reg_stb_chains_summary), alpha)


@pytest.mark.parametrize("n,shape,scale", pl.Q3_CASES, ids=pl.Q3_IDS)
def test_small_batch_q3(gpu_lib, n, shape, scale):
    """sig2 alone unknown at small n, through the summary call: beta, its variance and sig2."""
    bb = gpu_lib
    x, y, tau, alpha = pl.q3_data(n)
    targets = pl.checked(pl.targets_sig2_1d, x, y, tau, alpha, shape, scale)
    assert_batch_kernel(bb, x[:, None], y, K_BATCH, threads=512, true_alpha=alpha, true_tau=tau,
                        sig2_shape=shape, sig2_scale=scale)
    bb.set_seed(SEED + 11)
    s = bb.bridge_reg_stb_chains_summary(y, x[:, None], nsamp=M_BATCH, nchains=K_BATCH,
                                         alpha=alpha, tau_true=tau, sig2_shape=shape,
                                         sig2_scale=scale)
    assert not s["flags"].any()
    print(f"Q3 n={n}: split R-hat of beta (summary call) = {s['rhat'][0]:.4f}")
    assert s["rhat"][0] <= pl.RHAT_MAX
    st = pl.moment_stats_from_summary(s["chain_mean"][:, 0], s["chain_var"][:, 0], M_BATCH,
                                      "beta", targets)
    st["sig2"] = s["chain_mean"][:, 1]
    pl.judge(f"small batch Q3 n={n} IG({shape}, {scale})", st, targets, pl.Q3_NAMES)


def test_small_batch_s1(gpu_lib):
    X, y, g = small_traces(gpu_lib)
    assert_converged(g["beta"], "small batch S1 60x6")
    pl.stein_verdicts("small batch S1 60x6", g["beta"], linear_bs(X, y), (0, 1),
                      cond_fn=conditional_bs(X, y, g))


@pytest.mark.parametrize("n,p", [(100, 13), (150, 32)], ids=["32lanes_100x13", "16lanes_150x32"])
def test_narrow_lane_instances_s1(gpu_lib, n, p):
    bb = gpu_lib
    X, y, _ = synthetic_problem(n, p)
    assert_batch_kernel(bb, X, y, 64, threads=512)
    bb.set_seed(SEED + 12)
    g = bb.bridge_reg_stb_chains(y, X, nsamp=1000, nchains=64)
    assert_converged(g["beta"], f"small batch S1 {n}x{p}")
    pl.stein_verdicts(f"small batch S1 {n}x{p}", g["beta"], linear_bs(X, y), signal_swap(X),
                      cond_fn=conditional_bs(X, y, g))


# ---------------------------------------------------------------------------------------
# packed batch (key 21, two workgroups per CU)
# ---------------------------------------------------------------------------------------
def test_packed_batch(gpu_lib):
    bb = gpu_lib
    K = 2 * bb.compute_units()
    with tuning(bb, k21=1):
        X, y = pl.q2_data()
        b = bb.ChainBatch(bb.EngineConfig(n=20, p=2, seed=SEED), K, X, y)
        try:
            assert b.threads() == 256 and b.resident_per_cu() == 2
        finally:
            b.close()

        def call(fn):
            def run(y, X, a):
                bb.set_seed(SEED + 13)
                return fn(y, X, nsamp=M_BATCH, nchains=K, alpha=a)
            return run

        q2_on_device("packed batch Q2", call(bb.bridge_reg_stb_chains),
                     call(bb.bridge_reg_stb_chains_summary), 0.5)
        X, y, _ = synthetic_problem(100, 20)
        bb.set_seed(SEED + 14)
        g = bb.bridge_reg_stb_chains(y, X, nsamp=200, nchains=K)
    assert_converged(g["beta"], "packed batch S1 100x20")
    pl.stein_verdicts("packed batch S1 100x20", g["beta"], linear_bs(X, y), signal_swap(X),
                      second=False, cond_fn=conditional_bs(X, y, g))


# ---------------------------------------------------------------------------------------
# alpha sampled: the fused kernels (key 26) and the general path
# ---------------------------------------------------------------------------------------
def q1_judge(what, sampler, alpha_b, beta, alpha, resolution=pl.RESOLUTION, must_miss=True):
    """The chain against Beta(pair) d(alpha)^2 under the pair its sampling phase passes, and
    against the target it must miss: the model's own posterior (no d^2) on P(alpha > 0.9) under
    the uniform prior, the other pair's target on E alpha under alpha_b = 3."""
    x, y, sig2, tau = pl.q1_data()
    assert np.all((alpha > 0) & (alpha <= 1))
    pair = pl.q1_pair(sampler, 1.0, alpha_b)
    right = pl.checked(pl.targets_alpha_1d, x, y, sig2, tau, *pair, 2)
    pl.judge(f"{what} Beta{pair} d^2", pl.q1_stats(beta, alpha, right), right, pl.Q1_NAMES,
             resolution)
    if alpha_b == 1.0:
        wrong, name = pl.checked(pl.targets_alpha_1d, x, y, sig2, tau, 1.0, 1.0, 0), \
            "p_alpha_gt_0.9"
    else:
        other = pl.q1_pair("ortho" if sampler == "stable" else "stable", 1.0, alpha_b)
        wrong, name = pl.checked(pl.targets_alpha_1d, x, y, sig2, tau, *other, 2), "alpha"
    z, _ = pl.z_of(pl.q1_stats(beta, alpha, wrong)[name], wrong[name].value)
    print(f"{what}: against the target it must miss, {name}: exact {wrong[name].value:.5f}, "
          f"z = {z:+.2f}")
    if must_miss:
        assert abs(z) > pl.Z_SCALAR, (what, name, z)


@pytest.mark.parametrize("ortho", [False, True], ids=["dense", "ortho"])
@pytest.mark.parametrize("alpha_b", [1.0, 3.0], ids=["uniform", "b3"])
def test_fused_alpha_batch_q1(gpu_lib, ortho, alpha_b):
    """k_small_chains_mh: 256 chains x 2000 sweeps."""
    g = alpha_traces(gpu_lib, ortho, alpha_b)
    assert_converged(g["beta"], "fused alpha batch")
    q1_judge(f"fused alpha batch {'ortho' if ortho else 'dense'}",
             "ortho" if ortho else "stable", alpha_b, g["beta"][..., 0], g["alpha"])


def sequential_stb(bb, seed, K, y, X, **kw):
    bb.set_seed(seed)
    out = [bb.bridge_reg_stb(y, X, **kw) for _ in range(K)]
    assert bb.get_rng_state() == (seed, K)
    return {k: np.stack([o[k] for o in out]) for k in ("beta", "alpha", "tau", "sig2")}


@pytest.mark.parametrize("ortho", [False, True], ids=["dense", "ortho"])
@pytest.mark.parametrize("alpha_b", [1.0, 3.0], ids=["uniform", "b3"])
def test_fused_alpha_single_chain_q1(gpu_lib, ortho, alpha_b):
    """k_small_chain_mh: 16 calls of 8000 sweeps, each cut into 4 batches of 2000 (the alpha
    chain's autocorrelation time is about 50 sweeps): 64 batches, 128 000 sweeps."""
    bb = gpu_lib
    x, y, sig2, tau = pl.q1_data()
    with tuning(bb, k26=1):
        g = sequential_stb(bb, SEED + 20, 16, y, x[:, None], nsamp=8000, alpha=0.0, alpha_a=1.0,
                           alpha_b=alpha_b, sig2_true=sig2, tau_true=tau, ortho=ortho)
    assert_converged(g["beta"], "fused alpha single chain")
    q1_judge(f"fused alpha single chain {'ortho' if ortho else 'dense'}",
             "ortho" if ortho else "stable", alpha_b, pl.batches(g["beta"][..., 0], 4),
             pl.batches(g["alpha"], 4))


def test_general_path_alpha_q1(gpu_lib):
    """k_alpha_mh (key 26 off): 8 chains of 8000 sweeps one after another, each cut into 8
    batches of 1000.  64 000 sweeps resolve less than the batch kernels' 512 000: the resolution
    bound is 0.03 sqrt(512 000 / 64 000) = 0.085 posterior sd.  The miss of the uncorrected
    target is asserted like everywhere else."""
    bb = gpu_lib
    x, y, sig2, tau = pl.q1_data()
    with tuning(bb, k26=0):
        g = sequential_stb(bb, SEED + 21, 8, y, x[:, None], nsamp=8000, alpha=0.0,
                           sig2_true=sig2, tau_true=tau)
    assert_converged(g["beta"], "general path alpha")
    q1_judge("general path alpha", "stable", 1.0, pl.batches(g["beta"][..., 0], 8),
             pl.batches(g["alpha"], 8), scaled_resolution(8 * 8000))


# ---------------------------------------------------------------------------------------
# wide batch (key 25), the general p <= n path, Woodbury p > n
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(150, 33), (200, 64), (200, 65), (300, 128)],
                         ids=["150x33", "200x64", "200x65", "300x128"])
def test_wide_batch_s1(gpu_lib, n, p):
    """First order for every j; second order for the 16 rows j with the largest off-diagonal
    |G_jk|."""
    X, y, g = wide_traces(gpu_lib, n, p)
    assert_converged(g["beta"], f"wide batch S1 {n}x{p}")
    pl.stein_verdicts(f"wide batch S1 {n}x{p}", g["beta"], linear_bs(X, y), signal_swap(X),
                      rows=pl.rows_largest_offdiag(X, 16), cond_fn=conditional_bs(X, y, g))
    if (n, p) != (150, 33):
        del _traces[("wide", n, p)]


def test_general_cholesky_path_s1(gpu_lib):
    """120 x 40 on one engine (the 256-padded Cholesky): 4 calls of 3000 sweeps, each cut into
    16 batches of 187."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(120, 40)
    with tuning(bb, k25=0):
        g = sequential_stb(bb, SEED + 30, 4, y, X, nsamp=3000)
    assert_converged(g["beta"], "general path S1 120x40")
    assert_batches_long("general path S1 120x40", g["beta"], 16)
    pl.stein_verdicts("general path S1 120x40", pl.batches(g["beta"], 16), linear_bs(X, y),
                      signal_swap(X), cond_fn=conditional_bs(X, y, g, 16))


def test_woodbury_path_s1(gpu_lib):
    """60 x 250, first order, sig2 known (with p > n and the Jeffreys prior the posterior has
    a degenerate mode at sig2 -> 0; see test_long_free_running_wide_chain_statistics): 6 calls
    of 3000 sweeps, each cut into 8 batches of 375 (the autocorrelation time is measured on the
    five signal columns and the next 27)."""
    bb = gpu_lib
    X, y, _ = synthetic_problem(60, 250, seed=11)
    g = sequential_stb(bb, SEED + 31, 6, y, X, nsamp=3000, sig2_true=1.0)
    assert_converged(g["beta"], "Woodbury S1 60x250")
    assert_batches_long("Woodbury S1 60x250", g["beta"], 8, np.arange(32))
    pl.stein_verdicts("Woodbury S1 60x250", pl.batches(g["beta"], 8),
                      linear_bs(X, y, sig2=np.float64(1.0)), signal_swap(X), second=False)


# ---------------------------------------------------------------------------------------
# triangle batch
# ---------------------------------------------------------------------------------------
def test_tri_batch_s1(gpu_lib):
    X, y, g = tri_traces(gpu_lib)
    assert_converged(g["beta"], "tri batch S1 100x13")
    pl.stein_verdicts("tri batch S1 100x13", g["beta"], linear_bs(X, y), signal_swap(X),
                      cond_fn=conditional_bs(X, y, g))


@pytest.mark.parametrize("alpha", [0.5, 0.8])
def test_tri_batch_q2(gpu_lib, alpha):
    bb = gpu_lib

    def call(fn):
        def run(y, X, a):
            bb.set_seed(SEED + 40)
            return fn(y, X, nsamp=4000, nchains=K_BATCH, alpha=a)
        return run

    assert_batch_kernel(bb, *pl.q2_data(), K_BATCH, method=4, true_alpha=alpha)
    q2_on_device(f"tri batch Q2 alpha={alpha}", call(bb.bridge_reg_tri_chains),
                 call(bb.bridge_reg_tri_chains_summary), alpha)


@pytest.mark.parametrize("ortho", [False, True], ids=["general", "ortho"])
@pytest.mark.parametrize("alpha_b", [1.0, 3.0], ids=["uniform", "b3"])
def test_tri_q1(gpu_lib, ortho, alpha_b):
    """The triangle chain with alpha sampled: k_tri_chains refuses alpha unknown, so the batch
    call runs one chain per call through the single-chain triangle path.  8 chains of 12 000
    sweeps, each cut into 8 batches of 1500.  Under alpha_a = 1, alpha_b = 3 the chain must
    match Beta(1, 3) d^2, the pair (alpha_a, alpha_b), and miss Beta(3, 3) d^2."""
    bb = gpu_lib
    x, y, sig2, tau = pl.q1_data()
    bb.set_seed(SEED + 41)
    g = bb.bridge_reg_tri_chains(y, x[:, None], nsamp=12000, nchains=8, alpha=0.0, alpha_a=1.0,
                                 alpha_b=alpha_b, sig2_true=sig2, tau_true=tau, ortho=ortho)
    assert_converged(g["beta"], "tri Q1")
    q1_judge(f"tri Q1 {'ortho' if ortho else 'general'}", "tri", alpha_b,
             pl.batches(g["beta"][..., 0], 8), pl.batches(g["alpha"], 8))


# ---------------------------------------------------------------------------------------
# logistic
# ---------------------------------------------------------------------------------------
@pytest.mark.slow
def test_logistic_s1(gpu_lib):
    """The logistic engine at 200 x 5: 96 calls of 5000 sweeps, one chain each.

    The slow test of this file (about 50 s), and the power condition does not let it be shorter.
    200 Bernoulli observations leave beta a posterior sd near 20 % of its size, so a scale error
    of 2^-8 is a shift of 0.02 sd.  The family's max |z| of the scaled traces against its bound
    5.52 was measured as 2.9 at 8 x 5000, 4.8 at 56 x 5000 and 5.64 at these 96 x 5000 sweeps on
    the device, 3.6 at 64 000, 5.7 at 256 000 and 7.5 at 320 000 on the oracle, and the engine,
    one chain per call, draws about 10 000 sweeps a second."""
    from tests.test_logit_gpu import logit_problem

    bb = gpu_lib
    X, y, _ = logit_problem(200, 5, seed=3)
    K = 96
    bb.set_seed(SEED + 50)
    beta = np.stack([bb.bridge_reg_logit(y, X, nsamp=5000, burn=100)["beta"] for _ in range(K)])
    assert bb.get_rng_state() == (SEED + 50, K)
    assert_converged(beta, "logistic S1 200x5")
    pl.stein_verdicts("logistic S1 200x5", beta, lambda b, c: pl.bs_logit(b, X, y, 0.5),
                      pl.most_correlated(X))


# ---------------------------------------------------------------------------------------
# cross-chain independence of the four batch kernels
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["small", "fused_alpha", "wide", "tri"])
def test_neighbouring_chains_are_independent(gpu_lib, kernel):
    bb = gpu_lib
    beta = {"small": lambda: small_traces(bb)[2]["beta"],
            "fused_alpha": lambda: alpha_traces(bb, False, 1.0)["beta"],
            "wide": lambda: wide_traces(bb, 150, 33)[2]["beta"],
            "tri": lambda: tri_traces(bb)[2]["beta"]}[kernel]()
    zs = pl.neighbour_z(beta)
    print(f"{kernel}: z of the neighbour correlation at shifts -2..2: "
          + ", ".join(f"{s:+d}: {z:+.2f}" for s, z in zs.items()))
    for s, z in zs.items():
        assert abs(z) <= pl.Z_SCALAR, (kernel, s, z)
