"""Cases and references shared by tests/test_logit_chain_layout_cpu.py and
tests/test_logit_chain_edges_gpu.py: the shapes at which the logistic chain batch
(bb_logit_chain.hip k_logit_chains) changes how it holds X or which instance runs, and a
beta | rest step in np.longdouble that judges both the kernel and the fp64 oracle.

layout() restates logit_chain_shm and logit_chain_instance.  The library has no accessor for
rows_lds; tests/test_logit_chain_layout_cpu.py reads the constants below out of the headers, so
a change of the LDS budget fails there and the cases get chosen again.

A design and an oracle chain are computed once per process and their arrays are read-only.
"""
import collections

import numpy as np

from oracle import gibbs

SEED = 0xB4E5B41D6E      # tests/test_logit_gpu.py SEED
LDS_BUDGET = 112 * 1024  # kSmallXLds (bb_small_body.h)
MAX_N = 4096             # kLogitChainMaxN (bb_kernels.h)
MAX_P = 32               # kSmallChainMaxP (bb_kernels.h)
LD = np.longdouble
ALPHA_SAMPLED = dict(alpha=0.0, alpha_a=2.0, alpha_b=3.0)


def layout(n, p):
    """(rows_lds, chunk sizes, lanes per coefficient of the lambda draw) of an n x p launch:
    X is resident (one chunk of n rows) when omega and X at the odd stride p | 1 fit the budget,
    else staged in chunks of as many rows as fit beside omega, a multiple of 4."""
    assert 1 <= p <= MAX_P and p <= n <= MAX_N
    fit = (LDS_BUDGET - 8 * n) // (8 * (p | 1))
    rows = n if fit >= n else fit & ~3
    chunks = tuple(min(rows, n - r0) for r0 in range(0, n, rows))
    return rows, chunks, 64 if p <= 8 else 32 if p <= 16 else 16


# ---------------------------------------------------------------------------------------
# the case tables: (n, p) -> (rows_lds, chunks, lanes) as worked out by hand from the rule
# ---------------------------------------------------------------------------------------
def _staged(n, rows, lanes):
    full, last = divmod(n, rows)
    return rows, (rows,) * full + ((last,) if last else ()), lanes


def _resident(n, lanes):
    return n, (n,), lanes


TEACHER_FORCED = collections.OrderedDict([
    ((1, 1), _resident(1, 64)),          # p = 1: one entry, one lane; n = p
    ((2, 2), _resident(2, 64)),          # the tail loop alone, n = p
    ((5, 5), _resident(5, 64)),          # n = p, n % 4 = 1
    ((32, 32), _resident(32, 16)),       # n = p at the limit; 16 threads own a second entry
    ((33, 32), _resident(33, 16)),       # n = p + 1, n % 4 = 1
    ((83, 13), _resident(83, 32)),       # n % 4 = 3, resident
    ((421, 32), _resident(421, 16)),     # the last resident n at p = 32, n % 4 = 1
    ((422, 32), _staged(422, 420, 16)),  # the first staged n at p = 32: chunks 420 + 2
    ((796, 16), _resident(796, 32)),     # the last resident n at stride 17, p = 16: 32 lanes
    ((797, 17), _staged(797, 796, 16)),  # p = 17: 16 lanes; chunks 796 + 1
    ((799, 16), _staged(799, 796, 32)),  # chunks 796 + 3 under 32 lanes
    ((1433, 9), _resident(1433, 32)),    # the last resident n at stride 9, p = 9: 32 lanes
    ((1434, 8), _staged(1434, 1432, 64)),   # p = 8: 64 lanes; chunks 1432 + 2
    ((1435, 9), _staged(1435, 1432, 32)),   # chunks 1432 + 3
    ((1000, 32), _staged(1000, 404, 16)),   # the README's shape: 404 + 404 + 192
    ((4093, 20), _staged(4093, 484, 16)),   # 9 chunks, the last 221 (tail 1)
    ((4095, 32), _staged(4095, 308, 16)),   # 14 chunks, the last 91 (tail 3)
    ((4096, 32), _staged(4096, 308, 16)),   # the limit: 14 chunks, the last 92
    ((4096, 2), _staged(4096, 3412, 64)),   # p = 2 at the limit: 3412 + 684
    ((4096, 1), _resident(4096, 64)),       # p = 1 at the limit stays resident
])
WHOLE_KNOWN = [(1000, 32), (4096, 32), (4095, 32), (422, 32), (797, 17), (799, 16), (1434, 8),
               (4096, 2), (4096, 1)]
# the staged path under each of the three MH instances (64, 32, 16, 16 lanes)
WHOLE_SAMPLED = [(1434, 8), (799, 16), (797, 17), (1000, 32)]
# resident designs with n % 4 = 0 and what they become with zero rows up to PAD_N: the real
# rows straddle a seam of the staged chunks.  (796, 16) is the 32-lane instance, which
# (420, 32) and (796, 17), both 16-lane, and (1432, 8), 64-lane, leave out.
PAD_N = 4096
PADDED = collections.OrderedDict([
    ((420, 32), (_resident(420, 16), _staged(PAD_N, 308, 16))),
    ((796, 17), (_resident(796, 16), _staged(PAD_N, 600, 16))),
    ((796, 16), (_resident(796, 32), _staged(PAD_N, 600, 32))),
    ((1432, 8), (_resident(1432, 64), _staged(PAD_N, 1136, 64))),
])
CASES = dict(teacher_forced=TEACHER_FORCED, whole_known=WHOLE_KNOWN, whole_sampled=WHOLE_SAMPLED,
             padded=PADDED)


def case_id(case):
    return f"{case[0]}x{case[1]}"


# ---------------------------------------------------------------------------------------
# designs
# ---------------------------------------------------------------------------------------
_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def edge_problem(n, p):
    """tests/test_logit_gpu.py logit_problem(n, p, n + p) with k = min(p, max(3, p // 20))
    signal coefficients: the same bits as tests/test_logit_chains_gpu.py problem(n, p) for
    p >= 3, and defined for p = 1, 2.  Returns (X column-major, y)."""
    if ("edge", n, p) not in _cache:
        rng = np.random.default_rng(n + p)
        X = rng.standard_normal((n, p)) * 1.0
        b = np.zeros(p)
        k = min(p, max(3, p // 20))
        b[:k] = rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ b))).astype(np.float64)
        _cache["edge", n, p] = _frozen(np.asfortranarray(X), y)
    return _cache["edge", n, p]


def dyadic_problem(n, p, pad_to=None):
    """edge_problem(n, p) with X rounded to multiples of 2^-10, so that every partial sum of
    X'(y - 1/2) is exact: c is the same in any summation order.  pad_to: followed by zero rows
    with y = 0 up to that many rows."""
    key = ("dyadic", n, p, pad_to)
    if key not in _cache:
        X, y = edge_problem(n, p)
        X = np.round(X * 1024.0) / 1024.0 + 0.0  # + 0.0: no negative zeros
        if pad_to is not None:
            X = np.vstack([X, np.zeros((pad_to - n, p))])
            y = np.concatenate([y, np.zeros(pad_to - n)])
        _cache[key] = _frozen(np.asfortranarray(X), y.copy())
    return _cache[key]


def oracle_chain(design, nsamp, burn, seed, stream, **kw):
    """gibbs.bridge_regression_logit of design = (maker, *args), e.g. (edge_problem, n, p)."""
    key = ("chain", design[0].__name__) + tuple(design[1:]) + (
        nsamp, burn, seed, stream, tuple(sorted(kw.items())))
    if key not in _cache:
        X, y = design[0](*design[1:])
        o = gibbs.bridge_regression_logit(y, X, nsamp, burn=burn, seed=seed, stream=stream, **kw)
        _frozen(*[v for v in o.values() if isinstance(v, np.ndarray)])
        _cache[key] = o
    return _cache[key]


# ---------------------------------------------------------------------------------------
# beta | rest
# ---------------------------------------------------------------------------------------
def beta_longdouble(X, y, omega, lam, tau, z):
    """The beta | rest step of the logistic sweep in np.longdouble (64-bit mantissa on x86):
    A = X' diag(omega) X + diag(lam / tau^2), c = X'(y - 1/2), A = U'U by a hand-written upper
    Cholesky, U'v = c, U m = v, U x = z, beta = m + x.  Plain loops over p <= 32; no code shared
    with gibbs.beta_step_chol, the engine or the kernel."""
    Xl = np.asarray(X, dtype=LD)
    n, p = Xl.shape
    om, lam, z = (np.asarray(v, dtype=LD) for v in (omega, lam, z))
    tau = LD(tau)
    A = (Xl.T * om) @ Xl
    for j in range(p):
        A[j, j] += lam[j] / (tau * tau)
    c = Xl.T @ (np.asarray(y, dtype=LD) - LD(0.5))
    U = np.zeros((p, p), dtype=LD)
    for k in range(p):
        d = A[k, k]
        for i in range(k):
            d -= U[i, k] * U[i, k]
        assert d > 0
        U[k, k] = np.sqrt(d)
        for j in range(k + 1, p):
            s = A[k, j]
            for i in range(k):
                s -= U[i, k] * U[i, j]
            U[k, j] = s / U[k, k]
    v = np.zeros(p, dtype=LD)
    for k in range(p):  # U'v = c
        s = c[k]
        for i in range(k):
            s -= U[i, k] * v[i]
        v[k] = s / U[k, k]
    m, x = np.zeros(p, dtype=LD), np.zeros(p, dtype=LD)
    for k in range(p - 1, -1, -1):  # U m = v, U x = z
        sm, sx = v[k], z[k]
        for j in range(k + 1, p):
            sm -= U[k, j] * m[j]
            sx -= U[k, j] * x[j]
        m[k] = sm / U[k, k]
        x[k] = sx / U[k, k]
    return m + x


def beta_fp64(X, y, omega, lam, tau, z):
    """The same step in fp64 by numpy's blocked sums and LAPACK: what a careful fp64 evaluation
    of these inputs gives, the yardstick of the device's error against beta_longdouble."""
    A = (X.T * omega) @ X + np.diag(lam / (tau * tau))
    c = X.T @ (y - 0.5)
    L = np.linalg.cholesky(A)
    m = np.linalg.solve(L.T, np.linalg.solve(L, c))
    return m + np.linalg.solve(L.T, z)


def rel_l2(a, ref):
    """Relative L2 error of an fp64 vector against a longdouble one, in longdouble."""
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.sqrt(np.sum((a - ref) ** 2) / np.sum(ref ** 2)))
