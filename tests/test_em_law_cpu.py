"""The references of tests/em_law.py against each other and against oracle/em.py, on the CPU:
the fp64 checker against the exact long-double recursion on every +-1 case the GPU test runs,
the long-double recursion against 40-digit arithmetic, the maximisation-step law and the CG
stopping law on the checker's own iterates, and the conditions the GPU cases rely on."""
import numpy as np
import pytest

from tests import em_law as L
from oracle import em


@pytest.mark.parametrize("n,p", L.HAD_SHAPES)
def test_oracle_matches_exact_recursion(n, p):
    """oracle.em.bridge_em on X'X = n I against the exact recursion in long double: the same
    zero pattern and solve count on every case, none left out, which is safe because no
    expectation step of any case comes within 1e-9 (relative) of lambda_max.  Its relative
    error per coefficient is printed: the device bound is L.ORACLE_FACTOR times it, per case."""
    tab = L.hadamard_table(n, p, em.bridge_em)
    worst, margin = 0.0, np.inf
    for (alpha, mi), rows in tab.items():
        for r in rows:
            assert r["margin"] >= 1e-9, (alpha, mi, r["ratio"], r["margin"])
            assert r["o_solves"] == r["solves"], (alpha, mi, r["ratio"])
            assert r["o_same_zeros"], (alpha, mi, r["ratio"])
            worst, margin = max(worst, r["o_err"]), min(margin, r["margin"])
    print(f"em_law {n}x{p}: oracle worst rel err {worst / L.EPS:.1f} eps, "
          f"smallest margin {margin:.2e}")
    assert worst < 1e-9     # the bound of the existing parity tests, far above what is seen


@pytest.mark.parametrize("n,p", [(64, 63), (128, 65)])
def test_long_double_recursion_against_mpmath(n, p):
    """The long-double recursion against the same recursion at 40 digits: same zero pattern
    and solve count, and an error at most 1/1000 of the bound the device is held to on that
    case with the long-double value as the reference, max(64 eps, 4 x the checker's error):
    the reference's own error then moves no verdict by more than a thousandth of the bound.
    (Long double carries 11 more bits than fp64, so its error is about 1/2048 of an fp64
    run's under the same amplification.)"""
    pytest.importorskip("mpmath")
    X, y = L.hadamard_case(n, p)
    b = X.T @ y
    tab = L.hadamard_table(n, p, em.bridge_em)
    eps_ld = float(np.finfo(L.LD).eps)
    worst = 0.0
    for (alpha, mi), rows in tab.items():
        for r in rows:
            mb, ms = L.em_orthogonal_mp(b, n, r["ratio"], alpha, r["lambda_max"], L.HAD_TOL, mi)
            assert ms == r["solves"]
            e = L.rel_err_mp(r["beta"], mb)
            worst = max(worst, e)
            bound = max(64 * L.EPS, L.ORACLE_FACTOR * r["o_err"])
            assert e <= bound / 1000, (alpha, mi, r["ratio"], e)
    print(f"em_law {n}x{p}: long double against 40 digits, worst {worst / eps_ld:.1f} ld eps")


@pytest.mark.parametrize("n,p", L.GEN_SHAPES)
@pytest.mark.parametrize("kind", L.GEN_DESIGNS)
def test_step_law_holds_for_the_oracle(kind, n, p):
    """The maximisation-step law the device is held to, on the checker's own iterates: the
    active set, the componentwise residual against scipy's Cholesky on the same system, and
    the objective's descent between iterates with one active set."""
    X, y = L.general_case(kind, n, p)
    G, b = L.general_gram(kind, n, p)
    for alpha in L.GEN_ALPHAS:
        for ratio in L.GEN_RATIOS:
            lmax = ratio / L.GEN_TOL
            its = [em.bridge_em(y, X, ratio, alpha, lmax, L.GEN_TOL, k)
                   for k in range(L.GEN_STEPS + 1)]
            st = L.check_steps(X, y, G, b, its, ratio, alpha, lmax)
            assert st["pairs"] > 0


def test_ridge_closed_form_oracle():
    """alpha = 2: lam is the constant 2, every step solves (X'X + 2 ratio^-2 I) beta = X'y,
    the second iteration moves nothing and the solve count is 3 p."""
    X, y = L.general_case("iid", 100, 20)
    G, b = L.general_gram("iid", 100, 20)
    beta, solves = em.bridge_em(y, X, 0.7, 2.0, 0.7 / 1e-9, 1e-9, 30)
    assert solves == 60
    A, rhs = L.ridge_ld(G, b, 0.7)
    assert L.cw_residual(A, rhs, beta) <= max(8 * L.EPS, 4 * L.cho_residual(A, rhs))


@pytest.mark.parametrize("name", list(L.CG_CASES))
def test_cg_cases_stop_by_their_rule(name):
    """What the GPU's CG test relies on, on the checker: every checked step of every case
    ends before its cap of p_active iterations, so the stopping rule is what ended it, and
    then |A beta_k - X_a'y| <= tol (1 + 1e-6) in long double; the p = 1025 case costs at most
    300 CG iterations in all."""
    c = L.CG_CASES[name]
    X, y = L.cg_design(name)
    args = (c["ratio"], c["alpha"], c["lambda_max"], c["tol"])
    runs = {k: em.bridge_em(y, X, *args, k, use_cg=True)
            for k in sorted({k - 1 for k in c["ks"]} | set(c["ks"]))}
    if name == "p1025":
        assert runs[max(c["ks"])][1] - X.shape[1] <= 300
    for k in c["ks"]:
        (pb, ps), (nb, ns) = runs[k - 1], runs[k]
        act, res = L.cg_step_residual(X, y, pb, nb, c["ratio"], c["alpha"], c["lambda_max"])
        assert np.array_equal(np.flatnonzero(nb), act)
        assert 0 < ns - ps < act.size, (k, ns - ps, act.size)
        assert res <= c["tol"] * (1 + 1e-6), (k, res)


def test_em_scratch_budget_hook_is_declared():
    import bayesbridge_amd as bb

    assert "bb_set_em_scratch_budget" in bb.EXPORTED_SYMBOLS
    assert callable(bb.set_em_scratch_budget)
