"""The residual-certified mixed plan (bb_nid.hip nid_plan_resid, k_nid_k2)
restated on top of oracle.gibbs: the first solve of the mixed plan on a guessed interval
[1, 1 + eps1], the correction's K2 chosen from the norm of the fp64 residual, and the redo on the
a-priori plan when the residual certifies nothing.  Works in whatever floating type the operators
and the right-hand side carry (the CPU tests run it in extended precision to see the certificate
itself rather than fp64 rounding)."""
import numpy as np

from oracle import gibbs

TOL = gibbs.NID_TOL
B32TOL = 2.0 ** -26
PHI = 8.0


def cheb_t(e, kmax):
    """t[K] = sqrt(1 + e) / cosh(K acosh sigma1) (1 + 1e-12), K = 1..kmax, on [1, 1 + e]."""
    sigma1 = (1.0 + 0.5 * e) / (0.5 * e)
    ac = np.arccosh(sigma1)
    with np.errstate(over="ignore"):
        return [np.inf] + [np.sqrt(1.0 + e) / np.cosh(k * ac) * (1.0 + 1e-12)
                           for k in range(1, kmax + 1)]


def eta_of(eps, tr):
    return (2.0 * gibbs.U32 * np.sqrt(tr * eps) + gibbs.U32 ** 2 * tr) * (1.0 + 1e-6)


def guess_interval(eps, tr, lam_x, sum_cn, phi=PHI):
    """eps1 = min(e2, phi tr(E) Lambda / sum |x_j|^2): lambda_max(E) for equal D_j, times phi."""
    e2 = eps + eta_of(eps, tr)
    if lam_x > 0.0 and np.isfinite(lam_x) and sum_cn > 0.0:
        return min(e2, phi * tr * lam_x / sum_cn)
    return e2


def plan_first(eta, e2, eps1, kcap, limit=np.inf, c64=1.0, c32=gibbs.COST32,
               cstep=gibbs.COST_STEP, bsave=0.0, any_cost=False):
    """nid_plan_resid: the cheapest (K1, predicted K2) of cost <= limit, else (0, 0)."""
    if not e2 < 1e300 or not eps1 > 0.0 or kcap < 1:
        return 0, 0
    kmax = min(kcap, 64)
    t1, t2 = cheb_t(eps1, kmax), cheb_t(e2, kmax)
    step32, step64 = c32 + cstep, c64 + cstep
    cap = (kcap - 1) * step64
    best, K1, K2 = np.inf, 0, 0
    for k1 in range(1, kmax + 1):
        rho = eta + t1[k1] * (1.0 + eta)
        if not rho < 1.0:
            continue
        need = TOL / rho
        k2 = next((k for k in range(1, kmax + 1) if eta + t2[k] * (1.0 + eta) <= need), 0)
        if not k2:
            continue
        cost = (k1 - 1) * step32 + step64 + (k2 - 1) * step32
        if not cost < cap * (1.0 - 1e-9):
            continue
        if rho * (1.0 + 1e-6) <= B32TOL:
            cost -= bsave
        if not any_cost and not cost <= limit:
            continue
        if cost < best:
            best, K1, K2 = cost, k1, k2
    return K1, K2


def plan(eps, tr, kcap, cost_fp64, key, lam_x=0.0, sum_cn=0.0, **costs):
    """The decision under bb_set_tuning key 29 = key: dict(K1, K2, eta, e2, eps1, resid,
    fallback).  key 0 is gibbs.nid_plan_mixed unchanged (K2 = 0: the fp64 plan, of cost_fp64,
    or the factor); otherwise that plan is the fallback and the residual-certified plan replaces
    it where it is no dearer than the a-priori mixed plan or cheaper than the fp64 plan (key 1),
    or wherever a first solve qualifies (key >= 2, phi = 8 / 16^(key - 2))."""
    K1, K2, eta, e2 = gibbs.nid_plan_mixed(eps, tr, kcap, cost_fp64, **costs)
    out = dict(K1=K1, K2=K2, eta=eta, e2=e2, eps1=e2, resid=False, fallback=(K1, K2))
    if key == 0 or (K2 == 0 and not cost_fp64 < np.inf):
        return out
    c64, c32 = costs.get("c64", 1.0), costs.get("c32", gibbs.COST32)
    cstep = costs.get("cstep", gibbs.COST_STEP)
    limit = (((K1 - 1 + K2 - 1) * (c32 + cstep) + c64 + cstep) * (1.0 + 1e-9) if K2
             else cost_fp64 * (1.0 - 1e-9))
    eps1 = guess_interval(eps, tr, lam_x, sum_cn, PHI / 16.0 ** max(key - 2, 0))
    k1, k2 = plan_first(eta, e2, eps1, kcap, limit, c64, c32, cstep, any_cost=key >= 2)
    if k2:
        out.update(K1=k1, K2=k2, eps1=eps1, resid=True)
    return out


def certify_k2(rnorm, bnorm, eps, eta, e2, kcap):
    """k_nid_k2: ratio = |r| (1 + eps)(1 + 1e-6) / |b| and the least K2 <= kcap with
    err2(K2) ratio <= 2^-56, err2 = eta + t_K2(e2)(1 + eta); K2 = 0: no certificate (a redo)."""
    ratio = 0.0 if rnorm == 0.0 else float(rnorm) * (1.0 + eps) * (1.0 + 1e-6) / float(bnorm)
    if not ratio < 1.0:
        return 0, ratio
    kmax = min(kcap, 64)
    t = cheb_t(e2, kmax)
    for k in range(1, kmax + 1):
        if (eta + t[k] * (1.0 + eta)) * ratio <= TOL:
            return k, ratio
    return 0, ratio


def solve_resid(apply_E, apply_E32, rhs, eps, eta, e2, eps1, K1, kcap, fallback):
    """The sweep's solve: (w, K2, ratio); K2 = 0 is the redo, gibbs.woodbury_solve_mixed on the
    a-priori plan `fallback` = (K1, K2) (K2 = 0 there: the fp64 plan's K1 iterates on eps)."""
    x0 = gibbs.woodbury_solve_cheb(apply_E32, rhs, eps1, K1)
    r = rhs - (x0 + apply_E(x0))
    K2, ratio = certify_k2(np.sqrt(r @ r), np.sqrt(rhs @ rhs), eps, eta, e2, kcap)
    if K2:
        return x0 + gibbs.woodbury_solve_cheb(apply_E32, r, e2, K2), K2, ratio
    f1, f2 = fallback
    if f2:
        return gibbs.woodbury_solve_mixed(apply_E, apply_E32, rhs, e2, f1, f2), 0, ratio
    return gibbs.woodbury_solve_cheb(apply_E, rhs, eps, f1), 0, ratio
