"""CPU tests: the oracle's chains against the exact posterior laws of tests/posterior_law.py.

Every other sampler test pins a kernel to the oracle; these pin the oracle to the model, with a
reference that shares no code with it: quadrature of the posterior (Q1 alpha sampled, Q2 p = 2
with tau and sig2 unknown, Q3 sig2 alone unknown at small n) and the integration-by-parts
identities for designs where quadrature is impossible (S1).

One long chain per case stands in for the K independent chains of the device tests: it is cut
into K = 64 consecutive batches whose means are the per-chain statistics (batches of 500 and more
sweeps against autocorrelation times of at most about 50, the alpha chain's), and into 8 segments
for split R-hat.  Keys are fixed, so every figure printed here is reproducible.
"""
import numpy as np
import pytest

import oracle
from bayesbridge_amd.diagnostics import rhat
from oracle import gibbs
from tests import posterior_law as pl
from tests.test_triangle_cpu import _basis

K = 64
SEED = 0x1A77


def chains(x, k=K):
    """(M, ...) -> (k, M // k, ...): consecutive batches of one chain."""
    x = np.asarray(x)
    m = x.shape[0] // k
    return x[: k * m].reshape((k, m) + x.shape[1:])


def assert_converged(beta, what):
    r = np.max(rhat(chains(beta.reshape(beta.shape[0], -1), 8)))
    print(f"{what}: split R-hat of beta over 8 segments = {r:.4f}")
    assert r <= pl.RHAT_MAX, (what, r)


# ---------------------------------------------------------------------------------------
# Q1: alpha sampled
# ---------------------------------------------------------------------------------------
Q1_SWEEPS = 64000


def q1_chain(sampler, alpha_b):
    x, y, sig2, tau = pl.q1_data()
    X = x[:, None]
    kw = dict(burn=500, alpha=0.0, true_sig2=sig2, true_tau=tau, alpha_a=1.0, alpha_b=alpha_b,
              seed=SEED + 1, stream=0)
    if sampler == "tri":
        o = gibbs.bridge_regression_tri(y, X, Q1_SWEEPS, _basis(X, y), **kw)
        return o["beta"][:, 0], o["alpha"]
    o = gibbs.bridge_regression_stable(y, X, Q1_SWEEPS, ortho=sampler == "ortho", **kw)
    return o["beta"][0], o["alpha"]


@pytest.mark.parametrize("sampler", ["stable", "ortho", "tri"])
@pytest.mark.parametrize("alpha_b", [1.0, 3.0], ids=["uniform", "b3"])
def test_q1_sampled_alpha(sampler, alpha_b):
    """The chain's (beta, alpha) law is the posterior times d(alpha)^2 under the prior pair its
    sampling phase passes: (alpha_b, alpha_b) for the stable non-orthogonal loop, (alpha_a,
    alpha_b) for the orthogonal loop and the triangle chain.  It must MISS the model's own
    posterior (no d^2) on P(alpha > 0.9) under the uniform prior, and the other pair's target on
    E alpha under alpha_b = 3: neither the inverted Hastings term nor the prior quirk can go
    away unnoticed."""
    x, y, sig2, tau = pl.q1_data()
    beta, alpha = q1_chain(sampler, alpha_b)
    assert np.all((alpha > 0) & (alpha <= 1))
    assert_converged(beta[:, None], f"Q1 {sampler}")
    pair = pl.q1_pair(sampler, 1.0, alpha_b)
    right = pl.checked(pl.targets_alpha_1d, x, y, sig2, tau, *pair, 2)
    pl.judge(f"Q1 {sampler} Beta{pair} d^2", pl.q1_stats(chains(beta), chains(alpha), right),
             right, pl.Q1_NAMES)
    if alpha_b == 1.0:
        wrong, name = pl.checked(pl.targets_alpha_1d, x, y, sig2, tau, 1.0, 1.0, 0), \
            "p_alpha_gt_0.9"
    else:
        other = (1.0, alpha_b) if sampler == "stable" else (alpha_b, alpha_b)
        wrong, name = pl.checked(pl.targets_alpha_1d, x, y, sig2, tau, *other, 2), "alpha"
    z, _ = pl.z_of(pl.q1_stats(chains(beta), chains(alpha), wrong)[name], wrong[name].value)
    print(f"Q1 {sampler}: against the target it must miss, {name}: exact {wrong[name].value:.5f}, "
          f"z = {z:+.2f}")
    assert abs(z) > pl.Z_SCALAR, (sampler, name, z)


# ---------------------------------------------------------------------------------------
# Q2: p = 2, tau and sig2 unknown
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.5, 0.8])
@pytest.mark.parametrize("sampler", ["stable", "tri"])
def test_q2_two_coefficients(sampler, alpha):
    X, y = pl.q2_data()
    assert abs(np.corrcoef(X.T)[0, 1]) > 0.7
    if sampler == "stable":
        beta = oracle.cpu_chain(y, X, 64000, burn=500, alpha=alpha, seed=SEED + 2)["beta"].T
    else:
        beta = gibbs.bridge_regression_tri(y, X, 64000, _basis(X, y), burn=500, alpha=alpha,
                                           seed=SEED + 2)["beta"]
    assert_converged(beta, f"Q2 {sampler} {alpha}")
    targets = pl.checked(pl.targets_2d, X, y, alpha)
    pl.judge(f"Q2 {sampler} alpha={alpha}", pl.q2_stats(chains(beta), targets), targets,
             pl.Q2_NAMES)


# ---------------------------------------------------------------------------------------
# Q3: sig2 alone unknown, small n
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape,scale", pl.Q3_CASES, ids=pl.Q3_IDS)
def test_q3_sig2_unknown(n, shape, scale):
    """Where the sig2 step's shape and scale matter: at n = 6 the prior's (2, 1) is as heavy as
    the data's (n / 2, RSS / 2)."""
    x, y, tau, alpha = pl.q3_data(n)
    o = gibbs.bridge_regression_stable(y, x[:, None], 32000, burn=500, alpha=alpha,
                                       true_tau=tau, sig2_shape=shape, sig2_scale=scale,
                                       seed=SEED + 3)
    assert_converged(o["beta"].T, f"Q3 n={n}")
    targets = pl.checked(pl.targets_sig2_1d, x, y, tau, alpha, shape, scale)
    st = pl.moment_stats(chains(o["beta"][0]), "beta", targets)
    st["sig2"] = chains(o["sig2"]).mean(axis=1)
    pl.judge(f"Q3 n={n} IG({shape}, {scale})", st, targets, pl.Q3_NAMES)


# ---------------------------------------------------------------------------------------
# S1: integration by parts
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(60, 6), (100, 20)])
def test_s1_stable(n, p):
    X, y = pl.s1_problem(n, p)
    beta = oracle.cpu_chain(y, X, 64000, burn=500, alpha=0.5, seed=SEED + 4)["beta"].T
    assert_converged(beta, f"S1 stable {n}x{p}")
    pl.stein_verdicts(f"S1 stable {n}x{p}", chains(beta),
                      lambda b, c: pl.bs_linear(b, X, y, 0.5), (0, 1))


def test_s1_triangle():
    X, y = pl.s1_problem(60, 6)
    beta = gibbs.bridge_regression_tri(y, X, 64000, _basis(X, y), burn=500, alpha=0.5,
                                       seed=SEED + 5)["beta"]
    assert_converged(beta, "S1 tri 60x6")
    pl.stein_verdicts("S1 tri 60x6", chains(beta), lambda b, c: pl.bs_linear(b, X, y, 0.5),
                      (0, 1))


def test_s1_logistic():
    from tests.test_logit_gpu import logit_problem

    X, y, _ = logit_problem(200, 5, seed=3)
    beta = oracle.cpu_logit_chain(y, X, 320000, burn=500, alpha=0.5, seed=SEED + 6)["beta"].T
    assert_converged(beta, "S1 logit 200x5")
    pl.stein_verdicts("S1 logit 200x5", chains(beta), lambda b, c: pl.bs_logit(b, X, y, 0.5),
                      pl.most_correlated(X))


def test_s1_sees_an_off_diagonal_error_in_the_beta_map():
    """Mutation: the stable sweep driven with G[0, 1] scaled by 0.9 in gibbs.beta_step_chol
    (which reads the upper triangle).  The identities must reject its chain."""
    X, y = pl.s1_problem(60, 6)
    n, p = X.shape
    G, c = X.T @ X, X.T @ y
    G[0, 1] *= 0.9
    seed, M = SEED + 7, 16000
    beta = np.zeros((M, p))
    b = np.linalg.solve(X.T @ X, c)
    for t in range(1, M + 200):
        tau = oracle.tau_from_sum(oracle.sum_abs_pow(b, 0.5), p, 0.5, 2.0, 2.0, seed, 0, t)
        r = y - X @ b
        sig2 = oracle.sig2_from_rss(float(r @ r), n, 0.0, 0.0, seed, 0, t)
        lam = oracle.sample_lambda(b, 0.5, tau, seed, 0, t)
        b = gibbs.beta_step_chol(G, c, lam, sig2, tau,
                                 oracle.normals(p, seed, 0, t, oracle.KIND_BETA_Z))
        if t >= 200:
            beta[t - 200] = b
    first, sec = pl.stein_stats(chains(beta), lambda bb, ch: pl.bs_linear(bb, X, y, 0.5))
    z, bound = pl.family_max_z(first, sec)
    print(f"mutated beta map: max |z| = {z:.1f}, bound {bound:.2f}")
    assert z > bound, (z, bound)
