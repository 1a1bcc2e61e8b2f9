"""Exact posterior laws of the bridge models, and the statistics that hold a chain to them.

A helper module (like tests/wide_cases.py, not collected).  Nothing here imports ``oracle`` or
``bayesbridge_amd``: the targets are plain numpy / scipy in fp64 and share no code with what
they judge.  A sampler test elsewhere in the suite says "the device draws what the oracle draws";
a test built on this module says "what is drawn follows the model's posterior".

The model (BridgeRegression.cpp:436-575, with nu = tau^-alpha):
    y | beta, sig2 ~ N(X beta, sig2 I)
    p(beta_j | tau, alpha) = alpha / (2 tau Gamma(1/alpha)) exp(-|beta_j / tau|^alpha)
    sig2 ~ IG(sig2_shape, sig2_scale)   (0, 0: the Jeffreys prior 1 / sig2)
    nu ~ Ga(nu_shape, rate nu_rate)
    alpha ~ Beta(a, b)
The prior of beta does not scale with sig2.  The marginalisations are analytic:
    tau unknown:   prod_j p(beta_j) -> (nu_rate + sum_j |beta_j|^alpha)^-(nu_shape + p / alpha)
    sig2 unknown:  the likelihood   -> (sig2_scale + RSS(beta) / 2)^-(sig2_shape + n / 2)
The logistic bridge has y_i ~ Bernoulli(sigmoid(x_i' beta)) and no sig2.

alpha sampled.  The reference's Metropolis-Hastings step (BridgeRegression.cpp:478-503) proposes
from U(max(0, a - 0.1), min(1, a + 0.1)) and adds log(d_old) - log(d_new) to the log acceptance
ratio, d(a) = min(1, a + 0.1) - max(0, a - 0.1), d_new the width of the window round the current
value and d_old of the one round the proposal.  The Hastings correction of that proposal is the
opposite sign; with the sign as it is, the step is exactly invariant for pi(alpha | .) d(alpha)^2
(detailed balance: pi(a) d(a)^2 / d(a) min(1, pi(a') d(a') / (pi(a) d(a))) is symmetric in a,
a').  The project reproduces the reference, so the target of a chain that samples alpha carries
the factor d(alpha)^2 (``dpow = 2``); ``dpow = 0`` is the model's own posterior, which such a
chain must miss.  (a, b) is the pair the sampling phase passes: (alpha_b, alpha_b) in the
stable non-orthogonal MCMC loop, (alpha_a, alpha_b) in the stable orthogonal loop and in the
triangle chain.

alpha and tau both unknown have NO target here: the reference's tau step draws nu = tau^-alpha
from a Gamma conditional that treats nu as independent of alpha a priori, while its alpha step
holds tau (not nu) fixed.  The two conditionals do not come from one joint density, so the
chain's stationary law has no closed form to integrate.

Quadrature.  Composite Simpson on tensor grids.  Every beta axis has a node at 0 with an even
index, so no panel straddles the cusp of |beta|^alpha; the alpha axis has even-indexed nodes at
0.1 and 0.9, the kinks of d(alpha).  The p = 2 grid is uniform in u with beta = u^3, which makes
|beta|^alpha = |u|^(3 alpha) C^1 at that node (Simpson in beta itself converges only like
h^(1 + alpha) there).  ``checked`` evaluates a target twice, the second time with twice the
range and half the spacing, and refuses it unless every value moves by less than 1e-4 of the
statistic's posterior sd.  (Heavy tails need the range: with the Jeffreys sig2 prior at n = 8, a
grid of +-6 likelihood sds cuts the t tails and puts a correct chain 5 s.e. off.)

Integration-by-parts (Stein) identities, for any p and design.  With s = grad_beta log pi(beta |
y) and pi vanishing at infinity,
    first order:   E[1 + beta_j s_j] = 0                               for every j,
    second order:  E[beta_k (1 + delta_jk) + beta_j beta_k s_j] = 0    for every j, k.
beta_j s_j involves |beta_j|^alpha, not |beta_j|^(alpha - 1), so every term has finite variance
for alpha in (0, 1).  ``bs_linear`` / ``bs_logit`` return beta_j s_j with tau and sig2
marginalised, or plugged in from the trace where given (the conditional form, which separates
the lambda / beta steps from the scalar steps).  The identities see the design, the beta map and
the scale of beta; they are nearly blind to the hyper-priors when the data dominate, which is
what the small-n quadrature targets are for.

Verdicts, for K independent chains with fixed keys (deterministic, no retry).  A per-chain
statistic g_c (a chain mean) gives z = mean_c g_c / (sd_c g_c / sqrt K), or with a target,
(mean_c g_c - target) / (...).  The error is the between-chain spread: no ESS estimate is
involved.  A scalar target passes with |z| <= 5; a family of m identities passes with
max |z| <= z_m, the two-sided normal quantile of 1e-6 / m (about 6 at m = 1e4).  z is Student-t
with K - 1 degrees of freedom, not normal: at K = 64 its two-sided tail at 5 is 5e-6 against the
normal 6e-7, and at z_m for m = 36 it is 6e-7 against 3e-8 per identity -- small against the
margins the conditions below demand.  A pass means something only if the test also asserts
    resolution:   s.e. <= 0.03 posterior sd of the statistic, for every quadrature target;
    power:        the same traces times 1 + 2^-8, and the same traces with two correlated columns
                  swapped, fail the same verdict;
    convergence:  split R-hat of beta over the chains <= 1.01.
"""
import math
from collections import namedtuple

import numpy as np
from scipy import special, stats

Z_SCALAR = 5.0
RESOLUTION = 0.03
RHAT_MAX = 1.01
POWER_SCALE = 1.0 + 2.0 ** -8
QUAD_TOL = 1e-4

Target = namedtuple("Target", "value sd")  # E f and sd f under the posterior


# ---------------------------------------------------------------------------------------
# the cases (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------
def q1_data():
    """Q1: the data of test_gibbs_chain_matches_exact_posterior (n = 6, p = 1); returns
    (x, y, sig2, tau)."""
    rng = np.random.default_rng(42)
    x = rng.standard_normal(6)
    y = 0.4 * x + rng.standard_normal(6)
    return x, y, 1.0, 0.5


def q2_data():
    """Q2: n = 20, two columns with correlation about 0.8."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 2))
    X[:, 1] = 0.8 * X[:, 0] + 0.6 * X[:, 1]
    y = X @ np.array([0.5, 0.0]) + rng.standard_normal(20)
    return np.asfortranarray(X), y


Q3_CASES = [(6, 2.0, 1.0), (12, 0.0, 0.0)]  # n, sig2_shape, sig2_scale
Q3_IDS = ["proper_n6", "jeffreys_n12"]


def q3_data(n):
    """Q3: p = 1; returns (x, y, tau, alpha)."""
    rng = np.random.default_rng(42)
    x = rng.standard_normal(n)
    y = 0.4 * x + rng.standard_normal(n)
    return x, y, 0.5, 0.5


def s1_problem(n, p, seed=7):
    """S1: columns 0 and 1 correlated (about 0.8), three signals of different size."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    X[:, 1] = 0.8 * X[:, 0] + 0.6 * X[:, 1]
    b = np.zeros(p)
    b[[0, 2, 4]] = [1.5, -1.0, 0.5]
    y = X @ b + rng.standard_normal(n)
    return np.asfortranarray(X), y


Q1_NAMES = ("beta", "alpha", "var_alpha", "p_alpha_gt_0.9")
Q2_NAMES = ("beta0", "beta1", "var_beta0", "var_beta1", "beta0beta1")
Q3_NAMES = ("beta", "var_beta", "sig2")


def q1_pair(sampler, alpha_a, alpha_b):
    """The Beta pair the sampling phase of a chain passes to the alpha step."""
    return (alpha_b, alpha_b) if sampler == "stable" else (alpha_a, alpha_b)


def q1_stats(beta, alpha, targets):
    """beta, alpha (K, M)."""
    st = moment_stats(beta, "beta", targets)
    st.update(moment_stats(alpha, "alpha", targets))
    st["p_alpha_gt_0.9"] = (alpha > 0.9).mean(axis=1)
    return st


def q2_stats(beta, targets):
    """beta (K, M, 2)."""
    st = {"beta0beta1": (beta[..., 0] * beta[..., 1]).mean(axis=1)}
    for j in range(2):
        st.update(moment_stats(beta[..., j], f"beta{j}", targets))
    return st


# ---------------------------------------------------------------------------------------
# quadrature
# ---------------------------------------------------------------------------------------
def _axis(lo, hi, h):
    """Nodes k h from below lo to above hi, k = 0 at an even index, an even number of panels;
    returns (nodes, Simpson weights)."""
    kl = 2 * int(math.floor(lo / h / 2.0))
    kh = 2 * int(math.ceil(hi / h / 2.0))
    kl, kh = min(kl, 0), max(kh, 0)
    x = np.arange(kl, kh + 1) * h
    return x, _simpson(x.shape[0], h)


def _simpson(nodes, h):
    assert nodes % 2 == 1 and nodes >= 3
    w = np.ones(nodes)
    w[1:-1:2] = 4.0
    w[2:-1:2] = 2.0
    return w * (h / 3.0)


def _moment_targets(name, m):
    """Targets of x and of (x - E x)^2 from the raw moments m[1..4] of x."""
    mu = m[1]
    var = m[2] - mu * mu
    mu4 = m[4] - 4 * mu * m[3] + 6 * mu * mu * m[2] - 3 * mu ** 4
    return {name: Target(mu, math.sqrt(var)),
            f"var_{name}": Target(var, math.sqrt(max(mu4 - var * var, 0.0)))}


def checked(fn, *args, **kw):
    """fn(*args, refine=0) against refine=1 (twice the range, half the spacing): every value
    within QUAD_TOL of the statistic's posterior sd, or the target is refused.  Returns the
    refined targets."""
    coarse, fine = fn(*args, refine=0, **kw), fn(*args, refine=1, **kw)
    for k, t in fine.items():
        assert abs(coarse[k].value - t.value) <= QUAD_TOL * t.sd, (k, coarse[k], t)
        assert abs(coarse[k].sd - t.sd) <= 1e-3 * t.sd, (k, coarse[k], t)
    return fine


def alpha_window(a, ep=0.1):
    """d(alpha): the width of the MH proposal window round alpha."""
    return np.minimum(1.0, a + ep) - np.maximum(0.0, a - ep)


def targets_alpha_1d(x, y, sig2, tau, a, b, dpow, refine=0):
    """p = 1, tau and sig2 known, alpha sampled: p(beta, alpha | y) d(alpha)^dpow on a beta x
    alpha grid.  Targets: beta, var_beta, alpha, var_alpha, p_alpha_gt_0.9."""
    xx, xy = float(x @ x), float(x @ y)
    bhat, sd = xy / xx, math.sqrt(sig2 / xx)
    half, h = 12.0 * sd * 2 ** refine, sd / 100.0 / 2 ** refine
    na = 400 * 2 ** refine  # a multiple of 20: 0.1 and 0.9 are even-indexed nodes
    bg, wb = _axis(bhat - half, bhat + half, h)
    ag = np.arange(na + 1) / na
    wa = _simpson(na + 1, 1.0 / na)
    loglik = -0.5 * (xx * bg * bg - 2.0 * xy * bg) / sig2
    loglik -= loglik.max()
    labs = np.log(np.abs(bg / tau), where=bg != 0, out=np.full_like(bg, -np.inf))
    mb = np.zeros((5, na + 1))  # raw moments of beta at each alpha, times the alpha density
    for i in range(1, na + 1):  # alpha = 0 has density 0
        al = ag[i]
        lp = math.log(al) - special.gammaln(1.0 / al) + (a - 1.0) * math.log(al)
        if al < 1.0:
            lp += (b - 1.0) * math.log1p(-al)
        elif b != 1.0:
            continue  # the Beta density is 0 at alpha = 1 for b > 1
        lp += dpow * math.log(alpha_window(al))
        w = np.exp(loglik - np.exp(al * labs) + lp) * wb
        pw = np.ones_like(bg)
        for r in range(5):
            mb[r, i] = w @ pw
            pw = pw * bg
    Z = wa @ mb[0]
    out = _moment_targets("beta", [wa @ mb[r] / Z for r in range(5)])
    out.update(_moment_targets("alpha", [wa @ (mb[0] * ag ** r) / Z for r in range(5)]))
    k9 = (9 * na) // 10
    pt = float(_simpson(na + 1 - k9, 1.0 / na) @ mb[0][k9:]) / Z  # [0.9, 1]: na / 10 panels
    out["p_alpha_gt_0.9"] = Target(pt, math.sqrt(pt * (1.0 - pt)))
    return out


def _log_marginal_lik(rss, n, sig2_shape, sig2_scale, sig2):
    if sig2 is None:
        return -(sig2_shape + 0.5 * n) * np.log(sig2_scale + 0.5 * rss)
    return -0.5 * rss / sig2


def targets_sig2_1d(x, y, tau, alpha, sig2_shape, sig2_scale, refine=0):
    """p = 1, tau and alpha known, sig2 unknown.  Targets: beta, var_beta, sig2 (through
    sig2 | beta ~ IG(sig2_shape + n / 2, sig2_scale + RSS / 2); needs shape + n / 2 > 2)."""
    n = x.shape[0]
    xx, xy, yy = float(x @ x), float(x @ y), float(y @ y)
    bhat = xy / xx
    sd = math.sqrt(max(yy - xy * xy / xx, 1e-300) / max(n - 1, 1) / xx)
    half, h = 40.0 * sd * 2 ** refine + abs(bhat), sd / 200.0 / 2 ** refine
    bg, wb = _axis(bhat - half, bhat + half, h)
    rss = yy - 2.0 * xy * bg + xx * bg * bg
    lw = _log_marginal_lik(rss, n, sig2_shape, sig2_scale, None) - np.abs(bg / tau) ** alpha
    w = np.exp(lw - lw.max()) * wb
    Z = w.sum()
    out = _moment_targets("beta", [w @ bg ** r / Z for r in range(5)])
    sh, sc = sig2_shape + 0.5 * n, sig2_scale + 0.5 * rss
    e1 = w @ (sc / (sh - 1.0)) / Z
    e2 = w @ (sc * sc / ((sh - 1.0) * (sh - 2.0))) / Z
    out["sig2"] = Target(e1, math.sqrt(e2 - e1 * e1))
    return out


def targets_2d(X, y, alpha, sig2_shape=0.0, sig2_scale=0.0, nu_shape=2.0, nu_rate=2.0,
               refine=0):
    """p = 2, alpha known, tau and sig2 unknown (both marginalised).  Targets: beta0, beta1,
    var_beta0, var_beta1, beta0beta1."""
    n = X.shape[0]
    G, c, yy = X.T @ X, X.T @ y, float(y @ y)
    bhat = np.linalg.solve(G, c)
    s2 = (yy - c @ bhat) / (n - 2)
    sd = np.sqrt(s2 * np.diag(np.linalg.inv(G)))
    # beta = u^3 on a uniform u grid: |beta|^alpha = |u|^(3 alpha) is then C^1 at the node 0,
    # where Simpson in beta itself converges only like h^(1 + alpha)
    axes = []
    for j in range(2):
        half = (16.0 * sd[j] + abs(bhat[j])) * 2 ** refine
        hu = half ** (1.0 / 3.0) / (300.0 * 2 ** refine)
        u, wu = _axis(-half ** (1.0 / 3.0), half ** (1.0 / 3.0), hu)
        axes.append((u ** 3, wu * 3.0 * u * u))
    (b0, w0), (b1, w1) = axes
    B0, B1 = b0[:, None], b1[None, :]
    rss = yy - 2.0 * (c[0] * B0 + c[1] * B1) + G[0, 0] * B0 * B0 + 2.0 * G[0, 1] * B0 * B1 + \
        G[1, 1] * B1 * B1
    lw = _log_marginal_lik(rss, n, sig2_shape, sig2_scale, None)
    lw = lw - (nu_shape + 2.0 / alpha) * np.log(nu_rate + np.abs(B0) ** alpha + np.abs(B1) ** alpha)
    W = np.exp(lw - lw.max()) * w0[:, None] * w1[None, :]
    Z = W.sum()
    m0, m1 = W.sum(axis=1) / Z, W.sum(axis=0) / Z
    out = {}
    for name, g, m in (("beta0", b0, m0), ("beta1", b1, m1)):
        out.update(_moment_targets(name, [m @ g ** r for r in range(5)]))
    e11 = b0 @ (W @ b1) / Z
    e22 = (b0 * b0) @ (W @ (b1 * b1)) / Z
    out["beta0beta1"] = Target(e11, math.sqrt(e22 - e11 * e11))
    return out


# ---------------------------------------------------------------------------------------
# integration by parts
# ---------------------------------------------------------------------------------------
def _prior_bs(beta, alpha, nu_shape, nu_rate, tau):
    """-beta_j d/dbeta_j log prior, tau marginalised (tau None) or given ((...,) broadcast)."""
    p = beta.shape[-1]
    ab = np.abs(beta) ** alpha
    if tau is None:
        return (nu_shape + p / alpha) * alpha * ab / (nu_rate + ab.sum(axis=-1, keepdims=True))
    return alpha * ab / np.asarray(tau, dtype=np.float64)[..., None] ** alpha


def bs_linear(beta, X, y, alpha, sig2_shape=0.0, sig2_scale=0.0, nu_shape=2.0, nu_rate=2.0,
              sig2=None, tau=None):
    """beta_j s_j of the linear bridge posterior for beta (..., p); sig2 / tau None:
    marginalised, else the trace (...) to condition on."""
    n = X.shape[0]
    G, c, yy = X.T @ X, X.T @ y, float(y @ y)
    Gb = beta @ G
    xr = c - Gb  # x_j'(y - X beta)
    rss = yy - 2.0 * (beta @ c) + (beta * Gb).sum(axis=-1)
    if sig2 is None:
        lik = (sig2_shape + 0.5 * n) / (sig2_scale + 0.5 * rss)
    else:
        lik = 1.0 / np.asarray(sig2, dtype=np.float64)
    return beta * xr * lik[..., None] - _prior_bs(beta, alpha, nu_shape, nu_rate, tau)


def bs_logit(beta, X, y, alpha, nu_shape=2.0, nu_rate=2.0, tau=None):
    """beta_j s_j of the logistic bridge posterior: s_j = x_j'(y - sigmoid(X beta)) - prior."""
    xr = (y - special.expit(beta @ X.T)) @ X
    return beta * xr - _prior_bs(beta, alpha, nu_shape, nu_rate, tau)


def stein_stats(beta, bs_fn, rows=None):
    """Per-chain means of the identities for traces beta (K, M, p): first (K, p) of
    1 + beta_j s_j, second (K, len(rows), p) of beta_k (1 + delta_jk) + beta_j beta_k s_j for
    j in rows (None: every j).  One chain at a time: K x M x p^2 is never formed."""
    K, M, p = beta.shape
    rows = np.arange(p) if rows is None else np.asarray(rows)
    first = np.empty((K, p))
    second = np.empty((K, rows.shape[0], p))
    for c in range(K):
        b = beta[c]
        g = 1.0 + bs_fn(b, c)  # (M, p)
        first[c] = g.mean(axis=0)
        second[c] = g[:, rows].T @ b / M
        second[c, np.arange(rows.shape[0]), rows] += b[:, rows].mean(axis=0)
    return first, second


def z_of(stat, target=0.0):
    """z of per-chain statistics (K, ...) against a target, and the s.e."""
    stat = np.asarray(stat, dtype=np.float64)
    K = stat.shape[0]
    se = stat.std(axis=0, ddof=1) / math.sqrt(K)
    return (stat.mean(axis=0) - target) / se, se


def z_family(m):
    """The bound on max |z| over m identities: the two-sided normal quantile of 1e-6 / m."""
    return float(stats.norm.isf(0.5e-6 / m))


def family_max_z(*stats_):
    """(max |z|, bound) over every entry of the given per-chain statistic arrays."""
    zs = np.concatenate([np.abs(z_of(s)[0]).ravel() for s in stats_])
    return float(zs.max()), z_family(zs.shape[0])


def judge(what, stats_, targets, names, resolution=RESOLUTION):
    """Each named target: the figures printed, then s.e. <= resolution x posterior sd and
    |z| <= 5 asserted.  stats_[name] is the per-chain statistic (K,).  Returns {name: z}."""
    zs, ses = {}, {}
    for name in names:
        t = targets[name]
        z, se = z_of(stats_[name], t.value)
        zs[name], ses[name] = float(z), float(se)
        print(f"{what} {name}: chains {np.mean(stats_[name]):.5f} +- {se:.5f}, exact "
              f"{t.value:.5f}, z = {z:+.2f}, s.e. / sd = {se / t.sd:.4f}")
    for name in names:
        assert ses[name] <= resolution * targets[name].sd, (what, name, ses[name])
        assert abs(zs[name]) <= Z_SCALAR, (what, name, zs[name])
    return zs


def moment_stats(x, name, targets):
    """Per-chain means of x (K, M) and of (x - E x)^2, E x the exact mean."""
    return {name: x.mean(axis=1), f"var_{name}": ((x - targets[name].value) ** 2).mean(axis=1)}


def moment_stats_from_summary(mean_c, var_c, M, name, targets):
    """moment_stats from each chain's mean and unbiased variance of M draws."""
    return {name: mean_c,
            f"var_{name}": central_sq_from_moments(mean_c, var_c, M, targets[name].value)}


def stein_verdicts(what, beta, bs_fn, swap, rows=None, second=True, cond_fn=None,
                   power=("scaled", "swapped")):
    """The verdict on traces beta (K, M, p), and the power conditions on the same traces: times
    1 + 2^-8, and with the columns ``swap`` exchanged, the same verdict must fail (``power``:
    the conditions asserted; both are printed).  ``second`` False: the first-order family alone.
    cond_fn: beta_j s_j of the conditional form (tau and sig2 from the trace), printed when the
    verdict fails.  Returns (max |z|, bound)."""
    out = {}
    for name, b in (("as drawn", beta), ("scaled", beta * POWER_SCALE),
                    ("swapped", swap_columns(beta, *swap))):
        first, sec = stein_stats(b, bs_fn, rows)
        out[name] = family_max_z(first, sec) if second else family_max_z(first)
        print(f"{what} {name}: max |z| first order {np.abs(z_of(first)[0]).max():.2f}, second "
              f"order {np.abs(z_of(sec)[0]).max():.2f}{'' if second else ' (not judged)'}, "
              f"bound {out[name][1]:.2f}")
    z, bound = out["as drawn"]
    if z > bound and cond_fn is not None:
        first, sec = stein_stats(beta, cond_fn, rows)
        print(f"{what} conditional on the traced tau, sig2: max |z| first order "
              f"{np.abs(z_of(first)[0]).max():.2f}, second order "
              f"{np.abs(z_of(sec)[0]).max():.2f}")
    assert z <= bound, (what, z, bound)
    for name in power:
        assert out[name][0] > out[name][1], (what, name, out[name])
    return z, bound


def batches(x, nb):
    """(K, M, ...) -> (K nb, M // nb, ...): each chain cut into nb consecutive batches, for the
    paths that run few chains (the between-batch spread then stands in for the between-chain
    one; batches must be long against the autocorrelation time)."""
    K, M = x.shape[:2]
    m = M // nb
    return x[:, : nb * m].reshape((K * nb, m) + x.shape[2:])


def central_sq_from_moments(mean_c, var_c, M, mu):
    """Per-chain mean of (x - mu)^2 from the chain's mean and unbiased variance of M draws."""
    return var_c * (M - 1.0) / M + (mean_c - mu) ** 2


def swap_columns(beta, j, k):
    out = beta.copy()
    out[..., [j, k]] = beta[..., [k, j]]
    return out


def most_correlated(X, among=None):
    """The pair j < k (among the first ``among`` columns) with the largest |x_j'x_k|."""
    G = np.abs(X.T @ X)
    q = G.shape[0] if among is None else among
    G = np.triu(G[:q, :q], 1)
    j, k = np.unravel_index(np.argmax(G), G.shape)
    return int(j), int(k)


def rows_largest_offdiag(X, count=16):
    """At most ``count`` rows j holding the largest off-diagonal |G_jk|, ascending."""
    G = np.abs(X.T @ X)
    np.fill_diagonal(G, 0.0)
    return np.sort(np.argsort(-G.max(axis=1), kind="stable")[:count])


def neighbour_z(beta, shifts=(-2, -1, 0, 1, 2)):
    """Cross-chain independence: for neighbouring chains c, c + 1 the correlation over sweeps of
    beta_j[c, t] with beta_j[c + 1, t + s], averaged over j; per shift s the mean over the K - 1
    pairs against the between-pair s.e.  Returns {s: z}."""
    K, M, p = beta.shape
    xc = beta - beta.mean(axis=1, keepdims=True)
    xc = xc / np.sqrt((xc * xc).sum(axis=1, keepdims=True))
    out = {}
    for s in shifts:
        a = xc[:-1, max(0, -s): M - max(0, s)]
        b = xc[1:, max(0, s): M - max(0, -s)]
        r = (a * b).sum(axis=1).mean(axis=1)  # (K - 1,)
        out[s] = float(z_of(r)[0])
    return out
