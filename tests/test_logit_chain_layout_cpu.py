"""CPU tests of what tests/test_logit_chain_edges_gpu.py stands on (tests/logit_chain_cases.py):
the LDS budget and limits the cases were chosen under are the headers', each case lands on the
layout it is there for, the long double beta | rest step agrees with the oracle's fp64 one, and
the oracle's chain does not notice zero rows appended to a design, which is what lets the GPU
test compare a resident X with a staged one bit for bit."""
import os
import re

import numpy as np
import pytest

import oracle
from oracle import gibbs
from tests import logit_chain_cases as lc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "bayesbridge_amd", "csrc")


def header_constant(header, name):
    """The integer value of `constexpr <type> name = <product of integers>;` in a header."""
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9][0-9\s*]*);" % name, f.read())
    assert m, (header, name)
    v = 1
    for factor in m.group(1).split("*"):
        v *= int(factor)
    return v


def test_constants_match_the_headers():
    assert header_constant("bb_small_body.h", "kSmallXLds") == lc.LDS_BUDGET
    assert header_constant("bb_kernels.h", "kLogitChainMaxN") == lc.MAX_N
    assert header_constant("bb_kernels.h", "kSmallChainMaxP") == lc.MAX_P
    # the rule layout() restates, as text: the budget less omega over the odd-stride row, and
    # the multiple of 4
    with open(os.path.join(CSRC, "bb_logit_chain.hip")) as f:
        src = f.read()
    assert "const size_t row = (size_t)(p | 1) * sizeof(double);" in src
    assert "const size_t fit = (kSmallXLds - om) / row;" in src
    assert "*rows_lds = fit >= (size_t)n ? n : (int)(fit & ~(size_t)3);" in src
    assert "return inst[(mh ? 3 : 0) + (p <= 8 ? 0 : p <= 16 ? 1 : 2)];" in src


def test_edge_problem_is_the_suites_problem():
    from tests.test_logit_gpu import logit_problem

    for n, p in ((50, 5), (83, 13), (150, 32), (60, 3)):
        X, y = lc.edge_problem(n, p)
        Xs, ys, _ = logit_problem(n, p, n + p)
        assert np.array_equal(X, Xs) and np.array_equal(y, ys)
        assert X.flags.f_contiguous
    for n, p in ((1, 1), (2, 2), (4096, 1), (4096, 2)):
        X, y = lc.edge_problem(n, p)
        assert X.shape == (n, p) and y.shape == (n,)
        assert np.all((y == 0) | (y == 1))
    assert 0 < lc.edge_problem(4096, 1)[1].sum() < 4096


@pytest.mark.parametrize("case", list(lc.TEACHER_FORCED), ids=lc.case_id)
def test_case_hits_its_layout(case):
    assert lc.layout(*case) == lc.TEACHER_FORCED[case]


def test_layouts_the_cases_are_there_for():
    """The issue's table, spelled out once more and independently of the helper's tuples."""
    resident = [(421, 32), (796, 16), (1433, 9), (4096, 1)]
    staged = {(422, 32): (420, 2), (1000, 32): (404, 404, 192), (797, 17): (796, 1),
              (799, 16): (796, 3), (1434, 8): (1432, 2), (1435, 9): (1432, 3),
              (4096, 2): (3412, 684)}
    for n, p in resident:
        assert lc.layout(n, p)[:2] == (n, (n,)), (n, p)
        # and one more row would not fit
        if n < lc.MAX_N:
            assert lc.layout(n + 1, p)[0] < n + 1, (n, p)
    assert 421 % 4 == 1
    for (n, p), chunks in staged.items():
        rows, got, _ = lc.layout(n, p)
        assert got == chunks and rows == chunks[0] and rows % 4 == 0, (n, p)
    for (n, p), (rows, count, last) in {(4096, 32): (308, 14, 92), (4095, 32): (308, 14, 91),
                                        (4093, 20): (484, 9, 221)}.items():
        r, chunks, lanes = lc.layout(n, p)
        assert (r, len(chunks), chunks[-1]) == (rows, count, last) and lanes == 16
        assert all(c == rows for c in chunks[:-1]) and sum(chunks) == n
    assert 91 % 4 == 3 and 221 % 4 == 1
    # every instance boundary is among the teacher-forced cases, staged and resident
    lanes = {(lc.layout(*c)[2], len(lc.layout(*c)[1]) > 1) for c in lc.TEACHER_FORCED}
    assert lanes == {(L, s) for L in (64, 32, 16) for s in (False, True)}
    assert {p for _, p in lc.TEACHER_FORCED} >= {1, 2, 8, 9, 16, 17, 32}
    # last chunks of 1, 2 and 3 rows
    assert {lc.layout(*c)[1][-1] for c in lc.TEACHER_FORCED} >= {1, 2, 3}
    for c in lc.WHOLE_KNOWN + lc.WHOLE_SAMPLED:
        assert c in lc.TEACHER_FORCED
    assert [lc.layout(*c)[2] for c in lc.WHOLE_SAMPLED[:3]] == [64, 32, 16]
    assert all(len(lc.layout(*c)[1]) > 1 for c in lc.WHOLE_SAMPLED)


def test_padded_cases_straddle_a_seam():
    for (n, p), (small, padded) in lc.PADDED.items():
        assert n % 4 == 0
        assert lc.layout(n, p) == small and small[:2] == (n, (n,))
        assert lc.layout(lc.PAD_N, p) == padded
        rows = padded[0]
        assert rows < n and n % rows != 0, (n, p)  # a seam inside the real rows
    assert [v[1][0] for v in lc.PADDED.values()] == [308, 600, 600, 1136]
    assert {v[0][2] for v in lc.PADDED.values()} == {64, 32, 16}


@pytest.mark.parametrize("n,p", [(32, 32), (5, 5), (2, 2), (1, 1), (1000, 32), (4095, 32),
                                 (799, 16)], ids=lambda v: str(v))
def test_beta_longdouble_agrees_with_the_oracle(n, p):
    """The oracle's fp64 beta (LAPACK) against beta_longdouble on the oracle's own omega, lambda
    and tau over 12 sweeps, at the bar of 1e-13 relative L2.  Measured: at most 9.9e-16 over
    these designs (1000 x 32)."""
    X, y = lc.edge_problem(n, p)
    seed, stream = lc.SEED + 81, 2
    o = gibbs.bridge_regression_logit(y, X, 12, burn=0, seed=seed, stream=stream,
                                      record_state=True)
    assert len(o["states"]) == 12
    worst = 0.0
    for t, tau, lam, om, beta, _ in o["states"]:
        z = oracle.normals(p, seed, stream, t, gibbs.KIND_BETA_Z)
        ref = lc.beta_longdouble(X, y, om, lam, tau, z)
        assert ref.dtype == lc.LD
        worst = max(worst, lc.rel_l2(beta, ref))
        # the numpy fp64 yardstick of the GPU test is an evaluation of the same step
        assert lc.rel_l2(lc.beta_fp64(X, y, om, lam, tau, z), ref) <= 1e-13
    print(f"{n}x{p}: oracle beta against long double, worst rel L2 {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("kw", [{}, lc.ALPHA_SAMPLED], ids=["alpha_known", "alpha_sampled"])
def test_oracle_chain_ignores_appended_zero_rows(kw):
    """The premise of the resident-against-staged GPU test, on the oracle alone: omega's counters
    are per row, z's per coefficient, and nothing else in the sweep depends on n.  Measured over
    50 sweeps of the 420 x 32 dyadic design against its 4096-row padding, at the bar of 1e-9
    elementwise on beta: beta within 2.1e-14, lambda within 7.8e-12 relative, the sampled
    alpha equal (numpy's sums over 420 and over 4096 rows block differently, hence not 0)."""
    n, p = 420, 32
    X, y = lc.dyadic_problem(n, p)
    Xp, yp = lc.dyadic_problem(n, p, lc.PAD_N)
    assert np.array_equal(X * 1024.0, np.round(X * 1024.0))
    assert Xp.shape == (lc.PAD_N, p) and np.array_equal(Xp[:n], X) and not Xp[n:].any()
    assert np.array_equal(yp[:n], y) and not yp[n:].any()
    c, cp = X.T @ (y - 0.5), Xp.T @ (yp - 0.5)
    assert np.array_equal(c, cp)
    assert np.array_equal(c, np.asarray(X, dtype=lc.LD).T @ (np.asarray(y, dtype=lc.LD) - 0.5))
    run = dict(nsamp=50, burn=0, seed=lc.SEED + 82, stream=1, **kw)
    a = lc.oracle_chain((lc.dyadic_problem, n, p), **run)
    b = lc.oracle_chain((lc.dyadic_problem, n, p, lc.PAD_N), **run)
    d_beta = np.max(np.abs(a["beta"] - b["beta"]))
    d_lam = np.max(np.abs(a["lambda"] - b["lambda"]) / a["lambda"])
    d_alpha = np.max(np.abs(a["alpha"] - b["alpha"]))
    print(f"padded oracle chain: beta {d_beta:.2e}, lambda {d_lam:.2e}, alpha {d_alpha:.2e}")
    assert d_beta <= 1e-9
    if kw:
        assert len(np.unique(a["alpha"])) > 5
