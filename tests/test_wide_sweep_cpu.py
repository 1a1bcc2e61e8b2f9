"""CPU tests of the references that judge the wide fused sweep (tests/wide_cases.py): the case
builders do what they say, the extended-precision beta | rest draw is exact where exactness is
possible, and on every (design, state) pair of tests/test_wide_sweep_gpu.py the fp64 oracle sits
at least ten times inside the textbook bound of a Cholesky solve.  No GPU.

e_oracle = |beta_step_chol - ext_beta_step| / |ext_beta_step| must not exceed
3 p u kappa_s / 10, with u = 2^-53 and kappa_s the 2-norm condition of A scaled to unit diagonal.
The ill-conditioning of the shrunk state is diagonal scaling, which Cholesky does not feel, so
the reference alone meets the condition and the kernel's bar (32 e_oracle, at least p u) stays
far tighter than p u cond(A).
"""
import numpy as np
import pytest

from tests import wide_cases as wc


def test_interaction_design_construction():
    for q, p in ((10, 64), (13, 103)):
        assert wc.interaction_columns(q) == p
        X = wc.interaction_design(120, q, 3)
        assert X.shape == (120, p)
        assert np.max(np.abs(X.mean(axis=0))) < 1e-15
        assert np.max(np.abs(np.linalg.norm(X, axis=0) - 1.0)) < 1e-14
        assert len(np.unique(np.round(X[:, 0], 12))) == 2      # the binary column
        assert len(np.unique(np.round(X[:, 1], 12))) > 100
    # the family is what the wide kernel exists for and the Gaussian designs are not: G is far
    # from n I
    for n, q in ((442, 10), (506, 13)):
        X = wc.interaction_design(n, q, 3)
        assert 1e4 < np.linalg.cond(X.T @ X) < 1e7
    # truncation takes the first p columns of the smallest design that has them
    Xa = wc.interaction_problem(150, 49)[0]
    assert np.array_equal(Xa, wc.interaction_design(150, 10, 20240501)[:, :49])
    assert wc.interaction_problem(150, 128)[0].shape == (150, 128)


def test_states():
    rng = np.random.default_rng(0)
    b = np.r_[np.full(5, 2.0), np.zeros(59)]
    beta, tau, sig2 = wc.state_shrunk(64, b, rng)
    assert np.array_equal(beta[:5], b[:5]) and (tau, sig2) == (1e-3, 1.0)
    assert np.all((beta[5:] >= 1e-9) & (beta[5:] <= 1e-3))
    beta, tau, sig2 = wc.state_zero(64, b, rng)
    assert np.sum(beta == 0.0) == 2 and beta[63] == 0.0 and (tau, sig2) == (1.0, 1.0)


def test_ext_beta_step_exact_on_integers():
    """A = U'U with a small-integer U, integer m and x: every intermediate of the Cholesky and
    of the three solves is an integer, so the draw must come back exactly."""
    rng = np.random.default_rng(4)
    p = 23
    Ui = np.triu(rng.integers(-3, 4, size=(p, p))).astype(np.float64)
    Ui[np.diag_indices(p)] = rng.integers(1, 5, size=p)
    A = Ui.T @ Ui
    lam = rng.integers(1, 4, size=p).astype(np.float64)
    sig2, tau = 4.0, 2.0                      # lambda sig2 / tau^2 = lambda, sqrt(sig2) = 2
    G = A - np.diag(lam)
    m = rng.integers(-5, 6, size=p).astype(np.float64)
    x = rng.integers(-5, 6, size=p).astype(np.float64)
    beta = wc.ext_beta_step(G, A @ m, lam, sig2, tau, Ui @ x)
    assert beta.dtype == np.longdouble
    assert np.array_equal(beta, m + 2.0 * x)


def test_ext_beta_step_beyond_fp64():
    """np.longdouble must carry more than fp64 here (64-bit mantissa on x86): the residual of
    the extended draw's mean against a longdouble system is far below fp64 roundoff."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    X, y, _ = wc.interaction_problem(120, 64)
    G, c = wc.ext_gram(X, y)
    lam = np.ones(64)
    m = wc.ext_beta_step(G, c, lam, 1.0, 1.0, np.zeros(64))
    A = G + np.diag(lam.astype(np.longdouble))
    r = A @ m - c
    assert float(np.sqrt(r @ r) / np.sqrt(c @ c)) < 1e-17


def test_ext_beta_step_refuses_indefinite():
    with pytest.raises(np.linalg.LinAlgError):
        wc.ext_beta_step(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2), np.zeros(2), 1.0, 1.0,
                         np.zeros(2))


def test_case_list_covers_the_tiling():
    ps = {c.p for c in wc.CHOL_CASES}
    assert ps == {33, 48, 49, 63, 64, 65, 95, 96, 97, 103, 113, 127, 128}
    ids = [wc.case_id(c) for c in wc.CHOL_CASES + wc.ORTHO_CASES]
    assert len(set(ids)) == len(ids)
    assert all(c.p <= c.n for c in wc.CHOL_CASES)
    for p in (49, 64, 97, 103, 128):
        mine = [c for c in wc.CHOL_CASES if c.p == p and c.design == "int"]
        assert {c.n for c in mine} == {150, p + 1}
        assert {"benign", "shrunk"} <= {c.state for c in mine}


@pytest.mark.parametrize("c", wc.CHOL_CASES + wc.BATCH_CASES, ids=wc.case_id)
def test_oracle_inside_cholesky_bound(c):
    r = wc.reference(c)
    print(f"{wc.case_id(c)}: e_oracle {r.e_oracle:.2e} kappa_s {r.kappa_s:.2e} "
          f"lambda {r.lam.min():.1e} .. {r.lam.max():.1e} tau {r.tau:.2e}")
    assert np.all(np.isfinite(r.lam)) and np.all(r.lam > 0)      # h = 0 included (state zero)
    assert np.all(np.isfinite(r.beta_oracle))
    assert r.e_oracle <= 3 * c.p * wc.U * r.kappa_s / 10, (r.e_oracle, r.kappa_s)
    if c.true_tau:
        assert r.tau == c.true_tau
    if c.true_sig2:
        assert r.sig2 == c.true_sig2


def test_shrunk_state_spans_twelve_decades():
    """What the shrunk state is for: on an interaction design the diagonal lambda sig2 / tau^2
    spans about twelve decades and cond(A) is ten decades past cond of the scaled matrix."""
    c = next(c for c in wc.CHOL_CASES if (c.design, c.n, c.p, c.state) == ("int", 150, 103,
                                                                          "shrunk"))
    r = wc.reference(c)
    assert r.lam.max() / r.lam.min() > 1e10
    A = r.X.T @ r.X + np.diag(r.lam * r.sig2 / r.tau ** 2)
    assert np.linalg.cond(A) > 1e8 * r.kappa_s


@pytest.mark.parametrize("c", wc.ORTHO_CASES, ids=wc.case_id)
def test_ortho_reference_is_the_cholesky_draw(c):
    """On an orthogonal design the elementwise draw is the Cholesky draw: the two references
    agree, so the orthogonal cases are judged by the same arithmetic as the others."""
    r = wc.reference(c)
    G, cv = wc.ext_gram(r.X, r.y)
    ext = wc.ext_beta_step(G, cv, r.lam, r.sig2, r.tau, r.z)
    assert wc.ext_rel_err(r.beta_oracle, ext) < 1e-13
