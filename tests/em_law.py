"""Exact and long-double references for the bridge EM (BR::EM behind ``.C("bridge_EM")``),
independent of oracle/em.py: plain numpy, nothing of the checker imported.

1. ``hadamard_case`` / ``em_orthogonal``: on a +-1 design with X'X = n I and an integer y,
   X'X and X'y are exact in fp64 in any summation order and the EM decouples into the scalar
   recursion beta_j <- b_j / (n + c2 c1 |beta_j|^(alpha - 2)) with BR::EM's drop rule
   (lam < lambda_max), distance and stopping rule.  The recursion runs in long double.
2. ``m_step_system`` / ``cw_residual`` / ``objective``: on a general design, the system a
   maximisation step must have solved, rebuilt in long double from the previous iterate,
   the componentwise residual of a candidate solution and the penalised objective.
3. The designs and grids the CPU and the GPU tests share.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg as sla

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# ------------------------------------------------------------------------------------------
# 1. +-1 designs: the whole EM, exactly
# ------------------------------------------------------------------------------------------
HAD_SHAPES = [(64, 1), (64, 63), (64, 64), (128, 65), (128, 127), (128, 128), (256, 129),
              (256, 192), (256, 193), (256, 256), (512, 257)]
HAD_ALPHAS = [0.1, 0.5, 0.9, 1.0]
HAD_RATIOS = np.exp(np.array([-20.0, -6.0, -2.0, -0.5, 0.0, 1.0, 3.0, 8.0, 20.0]))
HAD_MAX_ITER = [1, 3, 30]
HAD_TOL = 1e-9
HAD_SEED = 20240917
# Device bound per non-zero coefficient on these designs: max(64 eps, ORACLE_FACTOR x the fp64
# checker's own error on the same case).  64 eps: about ten rounded operations over three
# iterations with the log's error doubled by |alpha - 2| <= 2.  The factor allows for the
# device's sqrt-and-two-divisions and ocml exp / log against LAPACK and libm; the recursion's
# amplification near a coefficient about to be dropped (the checker's error reaches 9041 eps
# at 256 x 193) is common to both sides.  Measured on an MI355X the device's error was at
# most 1.19 x the checker's wherever it exceeded the floor, so the factor is 4, not 8.
ORACLE_FACTOR = 4


@functools.lru_cache(maxsize=None)
def hadamard_case(n, p, seed=HAD_SEED):
    """(X, y): the first p columns of the Sylvester Hadamard matrix of order n and an integer
    y = X k + e, k a few integer coefficients and e integers in [-40, 40].  |X'y| < 2^53 by
    far, so X'y is exact in fp64 however it is summed."""
    rng = np.random.default_rng([seed, n, p])
    X = sla.hadamard(n)[:, :p].astype(np.float64)
    k = np.zeros(p)
    nz = rng.choice(p, size=min(p, max(1, p // 8)), replace=False)
    k[nz] = rng.integers(1, 6, nz.size) * rng.choice([-1, 1], nz.size)
    y = X @ k + rng.integers(-40, 41, n).astype(np.float64)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _lam(beta, alpha, ratio):
    """c1 |beta|^(alpha - 2) in long double, c1 = alpha ratio^(2 - alpha); inf at beta = 0."""
    a, t = LD(alpha), LD(ratio)
    c1 = a * np.exp((2 - a) * np.log(t))
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return c1 * np.exp((a - 2) * np.log(np.fabs(np.asarray(beta, dtype=LD))))


def em_orthogonal(b, n, ratio, alpha, lambda_max, tol, max_iter):
    """BR::EM on X'X = n I, X'y = b (exact integers), in long double.

    Returns (beta (long double), solves, margin): solves is p plus the active counts of the
    maximisation steps, or the iteration count when every coefficient was dropped; margin is
    the smallest |lam - lambda_max| / lambda_max any expectation step met."""
    b = np.asarray(b, dtype=LD)
    p = b.size
    nn, lmax, c2 = LD(n), LD(lambda_max), np.exp(-2 * np.log(LD(ratio)))
    beta = b / nn
    active = np.ones(p, dtype=bool)
    solves, it, dist, margin = p, 0, LD(tol) + 1, np.inf
    while dist > LD(tol) and it < max_iter:
        lam = _lam(beta, alpha, ratio)
        with np.errstate(invalid="ignore"):
            m = np.fabs(lam[active] - lmax) / lmax
            keep = active & (lam < lmax)
        if m.size:
            margin = min(margin, float(np.min(m)))
        if not keep.any():
            return np.zeros(p, dtype=LD), it, margin
        active = keep
        old = beta
        beta = np.where(active, b / (nn + c2 * np.where(active, lam, 0)), 0)
        solves += int(active.sum())
        d = np.where(active, beta - old, 0)
        dist = np.sqrt(np.sum(d * d))
        it += 1
    return np.where(active, beta, 0), solves, margin


_HAD_TABLES = {}


def hadamard_table(n, p, oracle_em):
    """Every case of the +-1 design (n, p), computed once and shared: {(alpha, max_iter):
    [row per ratio of HAD_RATIOS]}, a row being dict(ratio, lambda_max, beta (long double),
    solves, margin, o_beta, o_solves, o_err) with o_* what `oracle_em` (the fp64 checker's
    bridge_em, passed in: this module does not import it) returns and its worst relative
    error per non-zero coefficient against the long-double recursion."""
    if (n, p) in _HAD_TABLES:
        return _HAD_TABLES[(n, p)]
    X, y = hadamard_case(n, p)
    b = X.T @ y
    tab = {}
    for alpha in HAD_ALPHAS:
        for mi in HAD_MAX_ITER:
            rows = []
            for ratio in HAD_RATIOS:
                lmax = ratio / HAD_TOL
                beta, solves, margin = em_orthogonal(b, n, ratio, alpha, lmax, HAD_TOL, mi)
                ob, os_ = oracle_em(y, X, ratio, alpha, lmax, HAD_TOL, mi)
                same = np.array_equal(ob == 0, beta == 0)
                rows.append(dict(ratio=ratio, lambda_max=lmax, beta=beta, solves=solves,
                                 margin=margin, o_beta=ob, o_solves=os_, o_same_zeros=same,
                                 o_err=rel_err(ob, beta) if same else np.inf))
            tab[(alpha, mi)] = rows
    _HAD_TABLES[(n, p)] = tab
    return tab


def em_orthogonal_mp(b, n, ratio, alpha, lambda_max, tol, max_iter, digits=40):
    """The same recursion in mpmath at `digits` digits (lists of mpf); (beta, solves)."""
    import mpmath as mp

    with mp.workdps(digits):
        f = lambda v: mp.mpf(float(v))  # noqa: E731  (every input is an fp64 value)
        a, t, lmax, nn, tl = f(alpha), f(ratio), f(lambda_max), f(n), f(tol)
        c1 = a * mp.exp((2 - a) * mp.log(t))
        c2 = mp.exp(-2 * mp.log(t))
        bb = [f(v) for v in b]
        beta = [v / nn for v in bb]
        act = list(range(len(bb)))
        solves, it, dist = len(bb), 0, tl + 1
        while dist > tl and it < max_iter:
            lam = {j: (c1 * mp.exp((a - 2) * mp.log(abs(beta[j]))) if beta[j] != 0 else mp.inf)
                   for j in act}
            act = [j for j in act if lam[j] < lmax]
            if not act:
                return [mp.mpf(0)] * len(bb), it
            d2 = mp.mpf(0)
            for j in act:
                new = bb[j] / (nn + c2 * lam[j])
                d2 += (new - beta[j]) ** 2
                beta[j] = new
            solves += len(act)
            dist = mp.sqrt(d2)
            it += 1
        out = [mp.mpf(0)] * len(bb)
        for j in act:
            out[j] = beta[j]
        return out, solves


def rel_err_mp(x, ref, digits=40):
    """max_j |x_j - ref_j| / |ref_j| of a long double vector against a list of mpf, evaluated
    at `digits` digits (a long double enters as the exact sum of two fp64 values)."""
    import mpmath as mp

    with mp.workdps(digits):
        worst = mp.mpf(0)
        for v, r in zip(np.asarray(x, dtype=LD), ref):
            if r == 0:
                if v != 0:
                    return np.inf
                continue
            hi = float(v)
            worst = max(worst, abs(mp.mpf(hi) + mp.mpf(float(v - LD(hi))) - r) / abs(r))
        return float(worst)


def rel_err(x, ref):
    """max_j |x_j - ref_j| / |ref_j| over ref_j != 0, in long double; 0 when none."""
    ref = np.asarray(ref, dtype=LD)
    nz = ref != 0
    if not nz.any():
        return 0.0
    return float(np.max(np.fabs(np.asarray(x, dtype=LD)[nz] - ref[nz]) / np.fabs(ref[nz])))


# ------------------------------------------------------------------------------------------
# 2. General designs: one maximisation step, in long double
# ------------------------------------------------------------------------------------------
GEN_SHAPES = [(100, 20), (200, 65), (300, 129), (300, 192)]
GEN_DESIGNS = ["iid", "ar1", "scaled"]
GEN_ALPHAS = [0.5, 1.0]
GEN_RATIOS = np.exp(np.array([-3.0, 0.0, 4.0]))
GEN_TOL = 1e-9
GEN_STEPS = 6


@functools.lru_cache(maxsize=None)
def general_case(kind, n, p, seed=11):
    """(X, y) for kind 'iid' (Gaussian), 'ar1' (columns AR(1), rho = 0.99) or 'scaled' (iid
    columns times e^U, U uniform on log[1e-3, 1e3]); y = X beta0 + noise, beta0 chosen so the
    signal per column is O(1) whatever the column's scale."""
    rng = np.random.default_rng([seed, GEN_DESIGNS.index(kind), n, p])
    Z = rng.standard_normal((n, p))
    if kind == "ar1":
        rho = 0.99
        X = np.empty_like(Z)
        X[:, 0] = Z[:, 0]
        for j in range(1, p):
            X[:, j] = rho * X[:, j - 1] + np.sqrt(1 - rho * rho) * Z[:, j]
    elif kind == "scaled":
        X = Z * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), p))
    else:
        X = Z
    k = max(3, p // 10)
    b0 = np.zeros(p)
    b0[:k] = rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 3, k)
    y = (X / np.sqrt((X * X).mean(axis=0))) @ b0 + rng.standard_normal(n)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def general_gram(kind, n, p):
    """(X'X, X'y) of general_case(kind, n, p), formed in long double from X and y."""
    X, y = general_case(kind, n, p)
    Xl = X.astype(LD)
    return Xl.T @ Xl, Xl.T @ y.astype(LD)


def gram_ld(X, y):
    Xl = np.asarray(X, dtype=LD)
    return Xl.T @ Xl, Xl.T @ np.asarray(y, dtype=LD)


def m_step_system(G, b, prev, ratio, alpha, lambda_max):
    """The system the maximisation step after the fp64 iterate `prev` must solve, in long
    double from G = X'X and b = X'y: (active index set, A, rhs) with the active set the
    non-zeros of prev whose lam < lambda_max and A = G_aa + c2 diag(lam(prev_a))."""
    lam = _lam(prev, alpha, ratio)
    with np.errstate(invalid="ignore"):
        act = np.flatnonzero((np.asarray(prev) != 0) & (lam < LD(lambda_max)))
    c2 = np.exp(-2 * np.log(LD(ratio)))
    A = G[np.ix_(act, act)].copy()
    A[np.arange(act.size), np.arange(act.size)] += c2 * lam[act]
    return act, A, b[act]


def cw_residual(A, rhs, x):
    """Componentwise backward error max_i |A x - rhs|_i / (|A| |x| + |rhs|)_i, long double."""
    x = np.asarray(x, dtype=LD)
    return float(np.max(np.fabs(A @ x - rhs) / (np.fabs(A) @ np.fabs(x) + np.fabs(rhs))))


def cho_residual(A, rhs):
    """cw_residual of scipy's fp64 Cholesky solve of the same system (rounded to fp64)."""
    A64, r64 = np.asarray(A, dtype=np.float64), np.asarray(rhs, dtype=np.float64)
    x = sla.cho_solve(sla.cho_factor(A64, lower=False), r64)
    return cw_residual(A, rhs, x)


def objective(X, y, beta, ratio, alpha):
    """1/2 |y - X beta|^2 + sum_j |beta_j / ratio|^alpha in long double (0^alpha = 0)."""
    bl = np.asarray(beta, dtype=LD)
    r = np.asarray(y, dtype=LD) - np.asarray(X, dtype=LD) @ bl
    nz = bl != 0
    pen = np.sum(np.exp(LD(alpha) * np.log(np.fabs(bl[nz]) / LD(ratio))))
    return r @ r / 2 + pen


def check_steps(X, y, G, b, its, ratio, alpha, lambda_max):
    """The maximisation-step law over consecutive iterates its = [(beta_k, solves_k), ...]
    (beta_k what a run with max_iter = k returns).  For every pair whose solve count grew (a
    pair whose count did not grow has converged: no step was taken, nothing to check):
      - the non-zeros of beta_k are exactly the non-zeros of beta_{k-1} with lam < lambda_max;
      - the componentwise residual of beta_k on the long-double system is at most
        max(8 eps, 4 x that of scipy's fp64 Cholesky solve of the same system);
      - with the active set unchanged, the objective does not increase by more than 4 eps
        relative (the MM property; across a drop it may, and is not asserted).
    Returns dict(pairs, res, cho, obj): the number of pairs checked and the worst residual,
    the worst Cholesky residual (both in eps) and the largest relative objective increase."""
    st = dict(pairs=0, res=0.0, cho=0.0, obj=-np.inf)
    for (pb, ps), (nb, ns) in zip(its[:-1], its[1:]):
        if ns <= ps:
            continue
        act, A, rhs = m_step_system(G, b, pb, ratio, alpha, lambda_max)
        assert np.array_equal(np.flatnonzero(nb), act), "active set"
        assert ns - ps == act.size, "solve count"
        res, cho = cw_residual(A, rhs, nb[act]), cho_residual(A, rhs)
        assert res <= max(8 * EPS, 4 * cho), (res / EPS, cho / EPS)
        st["pairs"] += 1
        st["res"], st["cho"] = max(st["res"], res / EPS), max(st["cho"], cho / EPS)
        if np.array_equal(pb != 0, nb != 0):
            o0, o1 = objective(X, y, pb, ratio, alpha), objective(X, y, nb, ratio, alpha)
            inc = float((o1 - o0) / np.fabs(o0))
            assert inc <= 4 * EPS, ("objective", inc / EPS)
            st["obj"] = max(st["obj"], inc)
    return st


def ridge_ld(G, b, ratio):
    """alpha = 2: (X'X + 2 ratio^-2 I) beta = X'y; returns (A, rhs) in long double."""
    A = G.copy()
    A[np.arange(b.size), np.arange(b.size)] += 2 * np.exp(-2 * np.log(LD(ratio)))
    return A, b


# ------------------------------------------------------------------------------------------
# 4. Conjugate gradients
# ------------------------------------------------------------------------------------------
# name -> design, parameters and the iterates k whose maximisation step is checked (the
# step from iterate k - 1 to k; both come from the device, so k >= 2).  lambda_max is chosen
# so the near-zero coefficients are dropped at once: kept, their c2 lam ~ |beta|^(alpha - 2)
# diagonal makes A so ill-conditioned that every CG solve runs to its cap of p_active
# iterations and the stopping rule is never the reason it ends.
CG_CASES = {
    # p_pad = 1280 unknowns on 1024 threads: every loop of k_em_cg strides
    "p1025": dict(design=("big",), ratio=1.0, alpha=0.5, tol=1e-6, lambda_max=100.0,
                  ks=(2, 3, 4, 5)),
    # the design and parameters of test_bridge_em_cg_matches_oracle
    "p40": dict(design=(250, 40, 3), ratio=0.2, alpha=0.5, tol=1e-10, lambda_max=0.2 / 1e-9,
                ks=(9, 10, 19)),
    "p300": dict(design=(700, 300, 3300), ratio=0.2, alpha=0.5, tol=1e-8, lambda_max=50.0,
                 ks=(2, 3, 4, 5)),
}
CG_BIG = dict(n=1400, p=1025)


def cg_design(name):
    d = CG_CASES[name]["design"]
    return cg_big_case() if d[0] == "big" else cg_case(*d)


@functools.lru_cache(maxsize=None)
def cg_big_case(seed=5):
    """X = Q diag(s): Q the orthonormal factor of a 1400 x 1025 Gaussian matrix, s in [1, 2],
    so X'X has condition number <= 4 and every CG solve takes a few tens of iterations."""
    rng = np.random.default_rng(seed)
    n, p = CG_BIG["n"], CG_BIG["p"]
    Q, _ = np.linalg.qr(rng.standard_normal((n, p)))
    X = Q * rng.uniform(1.0, 2.0, p)
    b0 = np.zeros(p)
    b0[:100] = rng.choice([-1.0, 1.0], 100) * rng.uniform(0.5, 3, 100)
    y = X @ b0 + 0.1 * rng.standard_normal(n)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def cg_case(n, p, seed):
    """The iid Gaussian case of tests/test_gpu_parity.py::_em_case, restated."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    b = np.zeros(p)
    k = max(3, p // 10)
    b[:k] = rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 3, k)
    y = X @ b + rng.standard_normal(n)
    return X, y


def cg_step_residual(X, y, prev, new, ratio, alpha, lambda_max):
    """(active set, |A new_a - X_a'y|_2) for the maximisation step after `prev`, long double,
    by matrix-vector products only: A v = X_a'(X_a v) + c2 lam v."""
    lam = _lam(prev, alpha, ratio)
    with np.errstate(invalid="ignore"):
        act = np.flatnonzero((np.asarray(prev) != 0) & (lam < LD(lambda_max)))
    c2 = np.exp(-2 * np.log(LD(ratio)))
    Xa = np.asarray(X, dtype=LD)[:, act]
    v = np.asarray(new, dtype=LD)[act]
    r = Xa.T @ (Xa @ v) + c2 * lam[act] * v - Xa.T @ np.asarray(y, dtype=LD)
    return act, float(np.sqrt(r @ r))
