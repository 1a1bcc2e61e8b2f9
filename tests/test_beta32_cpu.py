"""The fp32 beta pass of a certified near-identity sweep, restated in numpy.

beta_j = u_j + D_j g_j / sig needs g = X'w for the Chebyshev solution w = x_K = sum_k d_k.  The
solve's fp64 passes already form X'd_k for every increment but the last, so g is that banked
sum plus fl32(X)'w_s for the small rest w_s (d_{K-1}; the correction c of a mixed-plan sweep),
and X beta = X u + sig (b - w) follows from M w = b.  The device takes the pass when its bound
on |w_s| / |w| is at most 2^-26 (bb_kernels.h kBeta32Tol).  Checked here, over designs with D
spread over ten decades and eps from 1e-12 to 1e-2: the dots agree with X'w within the fp32
copy's share 2^-50 |x_j| |w| plus the fp64 dot's own worst-case rounding, X beta agrees with
the product, and the rule refuses increments beyond the bound."""
import numpy as np
import pytest

U32 = 2.0 ** -24
TOL = 2.0 ** -56       # kNidTol: the solve's certificate
B32TOL = 2.0 ** -26    # kBeta32Tol
N, P = 96, 300


def cheb_const(eps):
    theta, delta = 1.0 + 0.5 * eps, 0.5 * eps
    return theta, delta, theta / delta


def cheb_bound_at(eps, k):
    """sqrt(1 + eps) / T_k(sigma1) by the recurrence (bb_kernels.h cheb_bound_at)."""
    s1 = cheb_const(eps)[2]
    tm1, tk = 1.0, s1
    for _ in range(1, k):
        tm1, tk = tk, 2.0 * s1 * tk - tm1
    return np.sqrt(1.0 + eps) / tk


def cheb_iterations(eps, kmax=64, tol=TOL):
    for k in range(1, kmax + 1):
        if cheb_bound_at(eps, k) <= tol:
            return k
    return 0


def beta32_flag(eps, K, k2=0, err1=np.inf):
    """nid_finish's rule for NidState::b32 (without the cost gate)."""
    if K < 1:
        return False
    if k2 > 0:
        bound = err1
    elif K >= 2 and eps > 0:
        bound = cheb_bound_at(eps, K) + cheb_bound_at(eps, K - 1)
    else:
        return False
    return bound * (1.0 + 1e-6) <= B32TOL


def chebyshev(apply_e, rhs, eps, K):
    """K Chebyshev iterates on I + E from x_0 = 0 (k_cheb_init / k_cheb_step): the increments."""
    theta, delta, s1 = cheb_const(eps)
    r = rhs.copy()
    d = r / theta
    ds = [d.copy()]
    rho = 1.0 / s1
    for _ in range(1, K):
        r = r - (d + apply_e(d))
        rho1 = 1.0 / (2.0 * s1 - rho)
        d = rho1 * rho * d + (2.0 * rho1 / delta) * r
        rho = rho1
        ds.append(d.copy())
    return ds


def problem(eps_target, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, P))
    X -= X.mean(axis=0)
    y = X[:, :5] @ rng.uniform(1, 3, 5) + rng.standard_normal(N)
    sig2 = 0.7
    D = 10.0 ** rng.uniform(-10.0, 0.0, P)
    cn = (X * X).sum(axis=0)
    D *= eps_target * sig2 / float(D @ cn)      # tr(X D X') / sig2 = eps_target
    u = np.sqrt(D) * rng.standard_normal(P)
    sig = np.sqrt(sig2)
    b = y / sig - (X @ u / sig + rng.standard_normal(N))
    return X, y, D, u, sig2, b


def check(X, y, D, u, sig2, b, w, g):
    """The dots against X'w and X beta against the product, for a sweep whose flag holds."""
    sig = np.sqrt(sig2)
    Xl, wl = X.astype(np.longdouble), w.astype(np.longdouble)
    ref = np.asarray(Xl.T @ wl, dtype=np.longdouble)
    xn = np.sqrt((X * X).sum(axis=0))
    lim = (2.0 ** -50 + N * 2.0 ** -53) * xn * np.linalg.norm(w)
    err = np.abs(np.asarray(g, dtype=np.longdouble) - ref).astype(np.float64)
    assert np.all(err <= lim), float(np.max(err / lim))
    beta = u + D * g / sig
    xb = X @ u + sig * (b - w)
    assert np.max(np.abs(xb - X @ beta)) <= 1e-13 * np.linalg.norm(y)


EPS = [1e-12, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2]


@pytest.mark.parametrize("eps", EPS)
def test_fp64_plan_banked_dots_and_xbeta(eps):
    X, y, D, u, sig2, b = problem(eps, seed=int(-np.log10(eps)))
    X32 = X.astype(np.float32).astype(np.float64)
    K = cheb_iterations(eps)
    assert K >= 2
    ds = chebyshev(lambda v: X @ (D * (X.T @ v)) / sig2, b, eps, K)
    w = np.sum(ds, axis=0)
    # the certificate itself: the solve's residual is at rounding level
    assert np.linalg.norm(b - (w + X @ (D * (X.T @ w)) / sig2)) <= 1e-14 * np.linalg.norm(b)
    # a certified fp64 solve always passes: t_{K-1} <= 2 sigma1 t_K, and t_K <= 2^-56
    assert beta32_flag(eps, K)
    assert np.linalg.norm(ds[-1]) <= B32TOL * np.linalg.norm(w)
    g = np.zeros(P)
    for d in ds[:-1]:       # the dots the product passes formed, banked in order
        g = g + X.T @ d
    g = g + X32.T @ ds[-1]  # the last increment against the fp32 copy, arithmetic in fp64
    check(X, y, D, u, sig2, b, w, g)


def mixed_plan(eps, tr, need_flag):
    """(K1, K2, eta, e2, err1): the cheapest K1 whose first solve is (is not) within the fp32
    pass's bound, and the least K2 completing the certificate (nid_plan_mixed's inequality)."""
    eta = (2.0 * U32 * np.sqrt(tr * eps) + U32 * U32 * tr) * (1.0 + 1e-6)
    e2 = eps + eta
    ac = np.arccosh(cheb_const(e2)[2])
    with np.errstate(over="ignore"):  # T_k overflows to inf: t_k = 0, as on the device
        tk = np.sqrt(1.0 + e2) / np.cosh(np.arange(65) * ac) * (1.0 + 1e-12)
    t = lambda k: float(tk[k])
    for k1 in range(1, 65):
        err1 = eta + t(k1) * (1.0 + eta)
        if err1 >= 1.0 or (err1 * (1.0 + 1e-6) <= B32TOL) != need_flag:
            continue
        for k2 in range(1, 65):
            if (eta + t(k2) * (1.0 + eta)) * err1 <= TOL:
                return k1, k2, eta, e2, err1
    return None


@pytest.mark.parametrize("eps", EPS)
def test_mixed_plan_banked_dots_and_xbeta(eps):
    X, y, D, u, sig2, b = problem(eps, seed=100 + int(-np.log10(eps)))
    X32 = X.astype(np.float32).astype(np.float64)
    plan = mixed_plan(eps, eps, need_flag=True)
    assert plan is not None
    K1, K2, eta, e2, err1 = plan
    assert beta32_flag(eps, K1, K2, err1)
    e32 = lambda v: X32 @ (D * (X32.T @ v)) / sig2
    x0 = np.sum(chebyshev(e32, b, e2, K1), axis=0)
    g = X.T @ x0                                    # the fp64 residual pass's dots
    r = b - (x0 + X @ (D * g) / sig2)
    c = np.zeros(N)
    for d in chebyshev(e32, r, e2, K2):             # the correction, accumulated
        c = c + d
    w = x0 + c
    assert np.linalg.norm(c) <= B32TOL * np.linalg.norm(w)
    check(X, y, D, u, sig2, b, w, g + X32.T @ c)


def test_flag_is_off_beyond_the_bound():
    # K = 1 banks nothing; the factor (K = 0) has no solve
    assert not beta32_flag(1e-10, 1) and not beta32_flag(1e-10, 0)
    # K = 2 is certified up to eps ~ 1.05e-8 (t_2 ~ eps^2 / 8), where t_1 ~ eps / 2 is in bound
    assert cheb_iterations(1.0e-8) == 2 and beta32_flag(1.0e-8, 2)
    assert cheb_iterations(1.1e-8) == 3
    # two iterates beyond that (not a certified solve either): d_1 is too large
    assert not beta32_flag(3.2e-8, 2) and not beta32_flag(1e-6, 2)
    # mixed plans whose first solve is stopped early: the correction is too large.  They
    # exist only while 2^-26 (eta + ..) <= 2^-56, i.e. eta < 2^-30: the certificate
    # (eta + t_K2 (1 + eta)) err1 <= 2^-56 forces err1 <= 2^-26 beyond eps ~ 1e-5.
    for eps in (1e-4, 1e-3, 1e-2):
        assert mixed_plan(eps, eps, need_flag=False) is None
    for eps in (1e-6, 1e-5):
        plan = mixed_plan(eps, eps, need_flag=False)
        assert plan is not None
        K1, K2, _, _, err1 = plan
        assert err1 * (1.0 + 1e-6) > B32TOL and not beta32_flag(eps, K1, K2, err1)
    # and one whose eta alone is past the bound, whatever K1
    eps = 0.3
    eta = 2.0 * U32 * eps
    assert eta > B32TOL and not beta32_flag(eps, 20, 3, eta)
