"""The residual-certified mixed plan on the CPU (tests/nid_resid_plan.py restates
bb_nid.hip's nid_plan_resid and k_nid_k2 on top of oracle.gibbs).

The solves run in extended precision (numpy longdouble: 64 significant bits on x86, rounding
~1e-19 per operation), so the comparison with the exact solution sees the certificate's 2^-56
itself and not fp64 rounding.  The exact solution is numpy's direct fp64 solve refined three times
with extended-precision residuals (cond(M) <= 1.1: each refinement gains ~15 digits)."""
import numpy as np
import pytest

from oracle import gibbs
from tests import nid_resid_plan as rp

LD = np.longdouble
# the longdouble arithmetic's own rounding over a solve of <= 64 iterates on n <= 300 rows (where
# longdouble is plain fp64 the slack grows with its eps and the tests see fp64 rounding instead)
LD_SLACK = 4096 * float(np.finfo(LD).eps)


def _system(n, p, eps_target, seed):
    """X (n x p), D over 10 decades, sig2 = 1, scaled so that lambda_max(E) = eps_target / 15
    (the thresholded bound is 15-23 times lambda_max on the C3 chain) -> dict of operators."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    D = 10.0 ** rng.uniform(-10.0, 0.0, p)
    E = (X * D) @ X.T
    lmax = float(np.linalg.eigvalsh(E)[-1])
    D *= (eps_target / 15.0) / lmax
    X32 = X.astype(np.float32).astype(np.float64)
    El = (X.astype(LD) * D.astype(LD)) @ X.astype(LD).T
    E32l = (X32.astype(LD) * D.astype(LD)) @ X32.astype(LD).T
    lmax = float(np.linalg.eigvalsh(El.astype(np.float64))[-1])
    tr = float(np.trace(El)) * (1.0 + 1e-6)
    b = rng.standard_normal(n).astype(LD)
    M64 = np.eye(n) + El.astype(np.float64)
    w = np.linalg.solve(M64, b.astype(np.float64)).astype(LD)
    for _ in range(3):
        res = b - (w + El @ w)
        w = w + np.linalg.solve(M64, res.astype(np.float64)).astype(LD)
    return dict(n=n, eps=eps_target, tr=tr, lmax=lmax, b=b, w=w,
                E=lambda t: El @ t, E32=lambda t: E32l @ t)


def _rel(a, b):
    d = a - b
    return float(np.sqrt(d @ d) / np.sqrt(b @ b))


CASES = [(64, 200, 1e-8, 1), (100, 400, 1e-6, 2), (150, 300, 1e-4, 3), (200, 500, 1e-3, 4),
         (300, 700, 1e-2, 5), (128, 256, 1e-1, 6)]


@pytest.mark.parametrize("n,p,eps,seed", CASES)
def test_residual_certificate_whatever_the_first_interval(n, p, eps, seed):
    """Random PSD E, eps from 1e-8 to 1e-1, first-solve intervals that are right (1.05
    lambda_max), 10x and 1000x too small: whenever a K2 is returned the solve is within
    4 x 2^-56 of the exact solution (plus the extended arithmetic's own rounding); a redo
    reproduces gibbs.woodbury_solve_mixed (or the fp64 plan) on the a-priori plan exactly."""
    s = _system(n, p, eps, seed)
    kcap = 64
    K1a, K2a, eta, e2 = gibbs.nid_plan_mixed(eps, s["tr"], kcap, np.inf)
    fallback = (K1a, K2a) if K2a else (gibbs.cheb_iterations(eps, kcap), 0)
    assert fallback[0] > 0
    seen = set()
    for shrink in (1.0, 10.0, 1000.0):
        eps1 = min(e2, 1.05 * s["lmax"] / shrink)
        K1, _ = rp.plan_first(eta, e2, eps1, kcap, any_cost=True)
        if K1 == 0:      # no first solve qualifies (eta too large): the a-priori plan stands
            continue
        w, K2, ratio = rp.solve_resid(s["E"], s["E32"], s["b"], eps, eta, e2, eps1, K1, kcap,
                                      fallback)
        seen.add(K2 > 0)
        if K2:
            assert ratio < 1.0
            assert _rel(w, s["w"]) <= 4.0 * rp.TOL + LD_SLACK, (shrink, K1, K2, ratio)
        elif fallback[1]:
            ref = gibbs.woodbury_solve_mixed(s["E"], s["E32"], s["b"], e2, *fallback)
            assert np.array_equal(w, ref)
        else:
            ref = gibbs.woodbury_solve_cheb(s["E"], s["b"], eps, fallback[0])
            assert np.array_equal(w, ref)
    # err2 >= eta and rho^ >= eta: no (K1, K2) is even predicted once eta^2 > 2^-56 (eps = 1e-1)
    assert seen or eta * eta > rp.TOL, "no first solve ran"


def test_wrong_guess_is_redone_or_pays_with_iterates():
    """An interval 1000x too small at eps = 1e-2 leaves a residual that eta^2 > 2^-56 cannot
    correct: the certificate refuses it (K2 = 0, the redo), never a wrong w; at eps = 1e-6 the
    same wrong guess is absorbed by a larger K2 than the right interval needs."""
    s = _system(200, 500, 1e-2, 4)
    _, _, eta, e2 = gibbs.nid_plan_mixed(1e-2, s["tr"], 64, np.inf)
    eps1 = 1.05 * s["lmax"] / 1000.0
    K1, _ = rp.plan_first(eta, e2, eps1, 64, any_cost=True)
    assert K1 > 0
    _, K2, ratio = rp.solve_resid(s["E"], s["E32"], s["b"], 1e-2, eta, e2, eps1, K1, 64,
                                  (gibbs.cheb_iterations(1e-2, 64), 0))
    assert K2 == 0 and ratio * eta > rp.TOL
    s = _system(100, 400, 1e-6, 2)
    _, _, eta, e2 = gibbs.nid_plan_mixed(1e-6, s["tr"], 64, np.inf)
    k2 = []
    for shrink in (1.0, 1000.0):
        eps1 = 1.05 * s["lmax"] / shrink
        K1, _ = rp.plan_first(eta, e2, eps1, 64, any_cost=True)
        w, K2, _ = rp.solve_resid(s["E"], s["E32"], s["b"], 1e-6, eta, e2, eps1, K1, 64, (2, 2))
        assert K2 > 0 and _rel(w, s["w"]) <= 4.0 * rp.TOL + LD_SLACK
        k2.append((K1, K2))
    assert sum(k2[1]) >= sum(k2[0]) - 1, k2


@pytest.mark.parametrize("n,p,eps,seed", CASES[:5])
def test_ratio_within_a_priori_bound_on_the_certified_interval(n, p, eps, seed):
    """With eps1 = eps + eta the first solve has the a-priori bound |w - x0| <= err1 |w|, err1 =
    eta + t_K1(e2)(1 + eta), so |r| = |M (w - x0)| <= (1 + eps) err1 |b|: the measured
    |r| / |b| -- the certificate's ratio without its own (1 + eps)(1 + 1e-6) factor -- never
    exceeds (1 + eps) err1, for every K1 up to the plan's."""
    s = _system(n, p, eps, seed)
    eta = rp.eta_of(eps, s["tr"])
    e2 = eps + eta
    t = rp.cheb_t(e2, 12)
    for K1 in range(1, 9):
        err1 = eta + t[K1] * (1.0 + eta)
        x0 = gibbs.woodbury_solve_cheb(s["E32"], s["b"], e2, K1)
        r = s["b"] - (x0 + s["E"](x0))
        _, ratio = rp.certify_k2(np.sqrt(r @ r), np.sqrt(s["b"] @ s["b"]), eps, eta, e2, 64)
        raw = ratio / ((1.0 + eps) * (1.0 + 1e-6))
        assert raw <= (1.0 + eps) * err1 + LD_SLACK, (K1, raw, err1)


def test_key_zero_is_the_a_priori_plan():
    """bb_set_tuning key 29 = 0: gibbs.nid_plan_mixed's plan unchanged, over eps from 1e-9 to
    1e-1 and both cost regimes; key 1 always replaces an a-priori mixed plan (eps1 <= e2: the
    same plan qualifies) and never predicts more products; key 2 takes the plan wherever a first
    solve qualifies.  (Lambda / sum |x_j|^2 = 1e-3 and tr = 16 eps put
    eps1 at 0.128 eps, the C3 chain's proportions.)"""
    changed = 0
    for eps in 10.0 ** np.arange(-9.0, -0.5, 0.5):
        tr = 16.0 * eps
        for kcap, cost64 in ((16, np.inf), (16, 5 * 1.05), (64, 7 * 1.05)):
            K1, K2, eta, e2 = gibbs.nid_plan_mixed(eps, tr, kcap, cost64)
            off = rp.plan(eps, tr, kcap, cost64, 0, lam_x=0.1, sum_cn=100.0)
            assert (off["K1"], off["K2"], off["eta"], off["e2"]) == (K1, K2, eta, e2)
            assert not off["resid"] and off["eps1"] == e2
            on = rp.plan(eps, tr, kcap, cost64, 1, lam_x=0.1, sum_cn=100.0)
            assert on["fallback"] == (K1, K2)
            if on["resid"]:
                assert on["eps1"] <= e2
                changed += on["K1"] - 1 + on["K2"] - 1 < K1 - 1 + K2 - 1
            if K2:
                assert on["resid"] and on["K1"] - 1 + on["K2"] - 1 <= K1 - 1 + K2 - 1
                assert rp.plan(eps, tr, kcap, cost64, 2, lam_x=0.1, sum_cn=100.0)["resid"]
    assert changed > 0
