"""The device's bridge EM (bridge_EM / trace.beta: k_em_batch<64>, k_em_batch<128>,
k_em_batch_tiled, k_em_form, k_em_cg and their host loops) against the references of
tests/em_law.py, which do not restate oracle/em.py:

1. +-1 designs with X'X = n I: the whole EM against its exact scalar recursion in long double,
   at every shape edge of the three batch kernels and across the persistent Cholesky's padding.
2. General designs (iid, AR(1) 0.99, columns scaled over six decades): each maximisation step
   against the long-double system it must have solved, and the objective's descent;
   alpha = 2 against the ridge solution.
3. The chunk loop of bridge_em_batch, forced by the scratch budget hook.
4. Conjugate gradients past 1024 unknowns, and CG's stopping rule as a law.
5. Failure and special-value paths: a zero column, a NaN in y, a coefficient that is exactly 0.

Every test prints the figures it measured (pytest -s) before it asserts.
"""
import ctypes

import numpy as np
import pytest

from tests import em_law as L

pytestmark = pytest.mark.gpu

def _oracle_em():
    from oracle import em

    return em.bridge_em


def _check_rows(rows, beta, solves, tag):
    """Device rows against the table's: zero pattern, solve count, error bound.  Prints the
    worst device error and the worst device / checker error ratio over the rows where that
    ratio decides (a device error above the 64 eps floor) and over all rows."""
    worst, ratio, above = 0.0, 0.0, 0.0
    for r, bd, sd in zip(rows, beta, solves):
        ref = r["beta"]
        err = L.rel_err(bd, ref) if np.array_equal(bd == 0, ref == 0) else np.inf
        worst = max(worst, err / L.EPS)
        if r["o_err"] > 0:
            ratio = max(ratio, err / r["o_err"])
            if err > 64 * L.EPS:
                above = max(above, err / r["o_err"])
        r["_dev"] = (int(sd), err)
    print(f"em_law {tag}: device worst {worst:.1f} eps, device/checker ratio {above:.2f} above "
          f"the floor, {ratio:.2f} over all")
    for r, bd in zip(rows, beta):
        sd, err = r["_dev"]
        assert np.array_equal(bd == 0, r["beta"] == 0), (tag, r["ratio"])
        assert sd == r["solves"], (tag, r["ratio"], sd, r["solves"])
        assert err <= max(64 * L.EPS, L.ORACLE_FACTOR * r["o_err"]), (
            tag, r["ratio"], err / L.EPS, r["o_err"] / L.EPS)


# ------------------------------------------------------------------------------------------
# 1. The whole EM, exactly
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", L.HAD_SHAPES)
def test_batch_against_exact_recursion(gpu_lib, n, p):
    """bridge_em_batch, nine ratios from e^-20 to e^20 in one launch per (alpha, max_iter), on
    the first p columns of a Hadamard matrix: k_em_batch<64> for p <= 64 (p = 1, 63, 64),
    k_em_batch<128> to 128 (65: one live lane in the second wave; 127, 128),
    k_em_batch_tiled above (129, 193, 257: one live row in the last tile; 192, 256: no
    identity padding).  Same zero pattern and solve count as the exact recursion, every
    non-zero coefficient within max(64 eps, 4 x the fp64 checker's error on that case)."""
    bb = gpu_lib
    X, y = L.hadamard_case(n, p)
    tab = L.hadamard_table(n, p, _oracle_em())
    for (alpha, mi), rows in tab.items():
        beta, solves = bb.bridge_em_batch(y, X, L.HAD_RATIOS, alpha=alpha,
                                          lambda_max=L.HAD_RATIOS / L.HAD_TOL, tol=L.HAD_TOL,
                                          max_iter=mi)
        _check_rows(rows, beta, solves, f"batch {n}x{p} alpha={alpha} max_iter={mi}")


@pytest.mark.parametrize("alpha", L.HAD_ALPHAS)
@pytest.mark.parametrize("n,p", [(64, 1), (64, 63), (256, 256), (512, 257)])
def test_single_against_exact_recursion(gpu_lib, n, p, alpha):
    """The .C entry (k_em_form, the persistent Cholesky, the host's expectation step) on the
    same cases: p = 256 fills the Cholesky's padding exactly, p = 257 pads to 512."""
    bb = gpu_lib
    X, y = L.hadamard_case(n, p)
    tab = L.hadamard_table(n, p, _oracle_em())
    for mi in L.HAD_MAX_ITER:
        rows = tab[(alpha, mi)]
        out = [bb.bridge_em(y, X, alpha=alpha, ratio=r["ratio"], lambda_max=r["lambda_max"],
                            tol=L.HAD_TOL, max_iter=mi, ret_solves=True) for r in rows]
        _check_rows(rows, [o["beta"] for o in out], [o["num.solves"] for o in out],
                    f"single {n}x{p} alpha={alpha} max_iter={mi}")


# ------------------------------------------------------------------------------------------
# 2. General designs: every maximisation step
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", L.GEN_SHAPES)
@pytest.mark.parametrize("kind", L.GEN_DESIGNS)
def test_batch_steps_against_long_double(gpu_lib, kind, n, p):
    """bridge_em_batch with max_iter = 0 .. 6 returns the iterates; each step that was taken
    is held to L.check_steps: its active set, its componentwise residual on the long-double
    system within max(8 eps, 4 x scipy's Cholesky on the same system), and the objective's
    descent between iterates with one active set."""
    bb = gpu_lib
    X, y = L.general_case(kind, n, p)
    G, b = L.general_gram(kind, n, p)
    lmax = L.GEN_RATIOS / L.GEN_TOL
    agg = dict(pairs=0, res=0.0, cho=0.0, obj=-np.inf)
    for alpha in L.GEN_ALPHAS:
        runs = [bb.bridge_em_batch(y, X, L.GEN_RATIOS, alpha=alpha, lambda_max=lmax,
                                   tol=L.GEN_TOL, max_iter=k) for k in range(L.GEN_STEPS + 1)]
        for i, ratio in enumerate(L.GEN_RATIOS):
            its = [(bk[i], int(sk[i])) for bk, sk in runs]
            assert its[0][1] == p
            st = L.check_steps(X, y, G, b, its, ratio, alpha, lmax[i])
            agg = {k: (agg[k] + st[k] if k == "pairs" else max(agg[k], st[k])) for k in agg}
    print(f"em_law steps batch {kind} {n}x{p}: {agg['pairs']} steps, residual {agg['res']:.2f} "
          f"eps (scipy Cholesky {agg['cho']:.2f}), objective increase {agg['obj'] / L.EPS:.2f} eps")
    assert agg["pairs"] > 0


@pytest.mark.parametrize("n,p", L.GEN_SHAPES[:2])
@pytest.mark.parametrize("kind", L.GEN_DESIGNS)
def test_single_steps_against_long_double(gpu_lib, kind, n, p):
    """The same law for the .C entry with direct solves, max_iter = 1 .. 6."""
    bb = gpu_lib
    X, y = L.general_case(kind, n, p)
    G, b = L.general_gram(kind, n, p)
    agg = dict(pairs=0, res=0.0, cho=0.0, obj=-np.inf)
    for alpha in L.GEN_ALPHAS:
        for ratio in L.GEN_RATIOS:
            lmax = ratio / L.GEN_TOL
            its = []
            for k in range(1, L.GEN_STEPS + 1):
                o = bb.bridge_em(y, X, alpha=alpha, ratio=ratio, lambda_max=lmax, tol=L.GEN_TOL,
                                 max_iter=k, ret_solves=True)
                its.append((o["beta"], o["num.solves"]))
            st = L.check_steps(X, y, G, b, its, ratio, alpha, lmax)
            agg = {k: (agg[k] + st[k] if k == "pairs" else max(agg[k], st[k])) for k in agg}
    print(f"em_law steps single {kind} {n}x{p}: {agg['pairs']} steps, residual "
          f"{agg['res']:.2f} eps (scipy Cholesky {agg['cho']:.2f}), objective increase "
          f"{agg['obj'] / L.EPS:.2f} eps")
    assert agg["pairs"] > 0


@pytest.mark.parametrize("path,n,p", [("batch", 100, 20), ("batch", 200, 65),
                                      ("batch", 300, 129), ("single", 100, 20)])
def test_ridge_closed_form(gpu_lib, path, n, p):
    """alpha = 2: lam is the constant 2, every maximisation step solves
    (X'X + 2 ratio^-2 I) beta = X'y, the second iteration moves nothing (distance 0) and the
    solve count is 3 p; the estimate meets the residual bound on the long-double ridge system."""
    bb = gpu_lib
    X, y = L.general_case("ar1", n, p)
    G, b = L.general_gram("ar1", n, p)
    ratios = np.array([0.3, 2.0])
    if path == "batch":
        beta, solves = bb.bridge_em_batch(y, X, ratios, alpha=2.0, lambda_max=ratios / 1e-9,
                                          tol=1e-9, max_iter=30)
    else:
        out = [bb.bridge_em(y, X, alpha=2.0, ratio=r, lambda_max=r / 1e-9, tol=1e-9,
                            max_iter=30, ret_solves=True) for r in ratios]
        beta, solves = [o["beta"] for o in out], [o["num.solves"] for o in out]
    for ratio, bd, sd in zip(ratios, beta, solves):
        A, rhs = L.ridge_ld(G, b, ratio)
        res, cho = L.cw_residual(A, rhs, bd), L.cho_residual(A, rhs)
        print(f"em_law ridge {path} {n}x{p} ratio={ratio}: residual {res / L.EPS:.2f} eps "
              f"(scipy Cholesky {cho / L.EPS:.2f}), solves {sd}")
        assert sd == 3 * p
        assert res <= max(8 * L.EPS, 4 * cho)


# ------------------------------------------------------------------------------------------
# 3. The chunk loop
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [129, 192])
def test_chunked_grid_same_bits(gpu_lib, p):
    """Seven ratios in chunks of 1, 2, 3 (a ragged last chunk) and 7, forced by the scratch
    budget hook: ratio r0 + blockIdx.x with scratch indexed by blockIdx.x gives the same
    beta and solves, bit for bit, as the default budget."""
    bb = gpu_lib
    X, y = L.general_case("iid", 300, p)
    ratios = np.exp(np.linspace(-3.0, 4.0, 7))
    args = dict(alpha=0.5, lambda_max=ratios / 1e-9, tol=1e-9, max_iter=30)
    per = 192 * 192 * 8      # a ratio's scratch: round_up(p, 64)^2 doubles
    ref_b, ref_s = bb.bridge_em_batch(y, X, ratios, **args)
    assert len(set(ref_s.tolist())) > 1 and ref_b.any(axis=1).all()
    try:
        for chunk in (1, 2, 3, 7):
            bb.set_em_scratch_budget(chunk * per + per // 2)
            bc, sc = bb.bridge_em_batch(y, X, ratios, **args)
            assert np.array_equal(sc, ref_s), chunk
            assert np.array_equal(bc, ref_b), chunk
    finally:
        bb.set_em_scratch_budget(0)
    b2, s2 = bb.bridge_em_batch(y, X, ratios, **args)
    assert np.array_equal(b2, ref_b) and np.array_equal(s2, ref_s)


# ------------------------------------------------------------------------------------------
# 4. Conjugate gradients
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.CG_CASES))
def test_cg_stopping_rule(gpu_lib, name):
    """k_em_cg's law, no checker needed: a maximisation step that took fewer than p_active
    iterations ended by its stopping rule, so |A beta_k - X_a'y|_2 <= tol (1 + 1e-6) on the
    system rebuilt in long double from beta_{k-1}.  p1025 runs 1280 unknowns on 1024 threads.
    The active sets equal the checker's."""
    bb = gpu_lib
    c = L.CG_CASES[name]
    X, y = L.cg_design(name)
    kw = dict(alpha=c["alpha"], ratio=c["ratio"], lambda_max=c["lambda_max"], tol=c["tol"],
              use_cg=True, ret_solves=True)
    runs = {k: bb.bridge_em(y, X, max_iter=k, **kw)
            for k in sorted({k - 1 for k in c["ks"]} | set(c["ks"]))}
    checked = 0
    for k in c["ks"]:
        pb, ps = runs[k - 1]["beta"], runs[k - 1]["num.solves"]
        nb, ns = runs[k]["beta"], runs[k]["num.solves"]
        act, res = L.cg_step_residual(X, y, pb, nb, c["ratio"], c["alpha"], c["lambda_max"])
        print(f"em_law cg {name} step {k}: {ns - ps} iterations on {act.size} unknowns, "
              f"residual / tol = {res / c['tol']:.4f}")
        assert np.array_equal(np.flatnonzero(nb), act), k
        assert 0 < ns - ps <= act.size, k
        if ns - ps < act.size:
            assert res <= c["tol"] * (1 + 1e-6), (k, res)
            checked += 1
    assert checked > 0
    kmax = max(c["ks"])
    ob, _ = _oracle_em()(y, X, c["ratio"], c["alpha"], c["lambda_max"], c["tol"], kmax,
                         use_cg=True)
    assert np.array_equal(runs[kmax]["beta"] == 0, ob == 0)


# ------------------------------------------------------------------------------------------
# 5. Failure and special values
# ------------------------------------------------------------------------------------------
EDGE_SHAPES = [("batch", 100, 20), ("batch", 200, 65), ("batch", 300, 129), ("single", 100, 20)]
EDGE_RATIOS = np.array([0.2, 1.0, 5.0])


def _run(bb, path, y, X, ratios, alpha=0.5, tol=1e-9, max_iter=30):
    """(beta rows, solves) of the ratios through bridge_em_batch or, one by one, bridge_em."""
    if path == "batch":
        return bb.bridge_em_batch(y, X, ratios, alpha=alpha, lambda_max=ratios / tol, tol=tol,
                                  max_iter=max_iter)
    out = [bb.bridge_em(y, X, alpha=alpha, ratio=r, lambda_max=r / tol, tol=tol,
                        max_iter=max_iter, ret_solves=True) for r in ratios]
    return np.array([o["beta"] for o in out]), np.array([o["num.solves"] for o in out])


@pytest.mark.parametrize("path,n,p", EDGE_SHAPES)
def test_zero_column_is_not_positive_definite(gpu_lib, capfd, path, n, p):
    """A design with one all-zero column: G_jj is exactly 0 and the pivot test fires.  Every
    ratio returns solves = -1 and a zero row, the call itself succeeds, the .C entry prints
    "Aborting EM.", and the next call with a good design gives the bits it gave before."""
    bb = gpu_lib
    X, y = L.general_case("iid", n, p)
    before = _run(bb, path, y, X, EDGE_RATIOS)
    assert (before[1] > 0).all()
    Xz = X.copy()
    Xz[:, p // 2] = 0.0
    ctypes.CDLL(None).fflush(None)
    capfd.readouterr()
    beta, solves = _run(bb, path, y, Xz, EDGE_RATIOS)
    ctypes.CDLL(None).fflush(None)
    printed = capfd.readouterr().out
    assert np.array_equal(solves, np.full(EDGE_RATIOS.size, -1))
    assert not np.asarray(beta).any()
    if path == "single":
        assert printed.count("Aborting EM.") == EDGE_RATIOS.size
    after = _run(bb, path, y, X, EDGE_RATIOS)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


@pytest.mark.parametrize("path,n,p", EDGE_SHAPES)
def test_nan_in_y_drops_every_coefficient(gpu_lib, path, n, p):
    """A NaN in y makes X'y, the first solve and every lam NaN; `lam < lambda_max` is false,
    so every coefficient is dropped at the first expectation step: solves = 0 (the iteration
    count), beta = 0, as BR::EM's early return does."""
    bb = gpu_lib
    X, y = L.general_case("iid", n, p)
    yn = y.copy()
    yn[n // 3] = np.nan
    beta, solves = _run(bb, path, yn, X, EDGE_RATIOS)
    assert np.array_equal(solves, np.zeros(EDGE_RATIOS.size, dtype=solves.dtype))
    assert np.array_equal(beta, np.zeros((EDGE_RATIOS.size, p)))


@pytest.mark.parametrize("path,n,p", [("batch", 64, 20), ("batch", 128, 65),
                                      ("batch", 256, 129), ("single", 64, 20)])
def test_exactly_zero_coefficient_is_dropped(gpu_lib, path, n, p):
    """A +-1 design with X_j'y = 0 exactly: the first solve gives beta_j = 0, log 0 = -inf,
    lam = +inf, and j is dropped at the first expectation step; the rest follows the exact
    recursion (zero pattern, solve count, error bound as in section 1)."""
    bb = gpu_lib
    X, y0 = L.hadamard_case(n, p)
    j = p // 3
    y = n * y0 - X[:, j] * (X[:, j] @ y0)      # integers; X_j'y = 0, X_i'y = n X_i'y0
    b = X.T @ y
    assert b[j] == 0 and np.count_nonzero(b) == p - 1
    oracle = _oracle_em()
    for alpha in (0.5, 1.0):
        rows = []
        for ratio in EDGE_RATIOS:
            lmax = ratio / 1e-9
            ref, s, margin = L.em_orthogonal(b, n, ratio, alpha, lmax, 1e-9, 30)
            assert margin >= 1e-9 and ref[j] == 0
            ob, _ = oracle(y, X, ratio, alpha, lmax, 1e-9, 30)
            assert np.array_equal(ob == 0, ref == 0)
            rows.append(dict(ratio=ratio, beta=ref, solves=s, o_err=L.rel_err(ob, ref)))
        beta, solves = _run(bb, path, y, X, EDGE_RATIOS, alpha=alpha)
        _check_rows(rows, beta, solves, f"zero b_j {path} {n}x{p} alpha={alpha}")
