"""Case builders shared by tests/test_wide_sweep_cpu.py and tests/test_wide_sweep_gpu.py: the
designs, teacher-forced starting states and references of one sweep of the wide fused chain
(bb_wide.hip wide_chain_body, 32 < p <= 128).

Two references judge a beta | rest draw.  The oracle's beta_step_chol is the reference's
operations in fp64 (LAPACK).  ext_beta_step is the same draw as an explicit Cholesky and three
triangular solves in np.longdouble (64-bit mantissa on x86), from G = X'X and c = X'y formed in
np.longdouble too; it judges both the kernel and the fp64 oracle.

A reference is computed once per process (lru_cache) and its arrays are read-only.
"""
import functools
import types

import numpy as np

import oracle
from oracle import gibbs
from tests.conftest import synthetic_problem
from tests.test_gpu_parity import flips, rel_err  # noqa: F401  (re-exported to the two tests)

SEED = 0xB4E5B41D6E
WIDE_KEY = 25            # bb_set_tuning: wide fused chains
U = 2.0 ** -53           # fp64 unit roundoff
LD = np.longdouble
HYPER = dict(nu_shape=2.0, nu_rate=2.0, sig2_shape=0.0, sig2_scale=0.0)  # EngineConfig defaults
NSIGNAL = 5


# ---------------------------------------------------------------------------------------
# designs
# ---------------------------------------------------------------------------------------
def interaction_columns(q):
    """Columns of interaction_design(., q, .): q + q (q - 1) / 2 + q - 1."""
    return q + q * (q - 1) // 2 + q - 1


def interaction_design(n, q, seed):
    """The published protocol's interaction construction on synthetic data: q correlated base
    columns (pairwise correlation 0.9 through a shared factor, mean 1 so that products and
    squares are collinear with the main effects, as those of uncentred measurements are), the
    first made binary (+-1), then all q (q - 1) / 2 pairwise products and the q - 1 squares of
    the non-binary columns; every column centred and scaled to unit norm.  q = 10 gives 64
    columns, q = 13 gives 103; cond(G) is about 1e5 at 442 x 64 and 506 x 103."""
    rng = np.random.default_rng(seed)
    base = (np.sqrt(0.1) * rng.standard_normal((n, q)) + np.sqrt(0.9) * rng.standard_normal((n, 1))
            + 1.0)
    base[:, 0] = np.where(base[:, 0] > 1.0, 1.0, -1.0)
    cols = [base[:, j] for j in range(q)]
    cols += [base[:, i] * base[:, j] for i in range(q) for j in range(i + 1, q)]
    cols += [base[:, j] ** 2 for j in range(1, q)]
    X = np.stack(cols, axis=1)
    X -= X.mean(axis=0)
    X /= np.linalg.norm(X, axis=0)
    return np.asfortranarray(X)


def interaction_problem(n, p, seed=20240501):
    """The first p columns of the protocol's q = 10 or q = 13 design (q = 15 above 103), five
    signal coefficients (the first five columns) and unit noise: (X, y, b_true)."""
    q = next(q for q in (10, 13, 15) if interaction_columns(q) >= p)
    X = np.asfortranarray(interaction_design(n, q, seed)[:, :p])
    rng = np.random.default_rng(seed + 1)
    b = np.zeros(p)
    # columns have unit norm: sqrt(n) puts the signal where synthetic_problem's is
    b[:NSIGNAL] = np.sqrt(n) * rng.uniform(1, 3, NSIGNAL) * rng.choice([-1.0, 1.0], NSIGNAL)
    y = X @ b + rng.standard_normal(n)
    y -= y.mean()
    return X, y, b


def ortho_problem(n, p, seed=9):
    """An orthogonal n x p design, QR-based as test_wide_chains_gpu.ortho_wide_problem."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, p)))
    X = np.asfortranarray(Q * 4.0)
    b = np.r_[np.ones(NSIGNAL), np.zeros(p - NSIGNAL)]
    y = X @ b + rng.standard_normal(n)
    return X, y, b


DESIGNS = {"syn": lambda n, p: synthetic_problem(n, p), "int": interaction_problem,
           "ortho": ortho_problem}


# ---------------------------------------------------------------------------------------
# teacher-forced starting states: (p, b_true, rng) -> (beta, tau, sig2)
# ---------------------------------------------------------------------------------------
def state_benign(p, b_true, rng):
    return b_true + 0.05 * rng.standard_normal(p), 1.0, 1.0


def state_shrunk(p, b_true, rng):
    """Every coefficient off the signal columns 3 to 9 decades down: lambda sigma^2 / tau^2 then
    spans about twelve decades."""
    beta = 10.0 ** rng.uniform(-9.0, -3.0, p)
    sig = b_true != 0
    beta[sig] = b_true[sig]
    return beta, 1e-3, 1.0


def state_zero(p, b_true, rng):
    """Two coefficients exactly 0.0 (one of them the last): h = 0 in their lambda draws and
    exp(alpha log 0) in S_alpha."""
    beta, tau, sig2 = state_benign(p, b_true, rng)
    beta[[NSIGNAL + 2, p - 1]] = 0.0
    return beta, tau, sig2


STATES = {"benign": state_benign, "shrunk": state_shrunk, "zero": state_zero}


# ---------------------------------------------------------------------------------------
# the extended-precision reference
# ---------------------------------------------------------------------------------------
def ext_gram(X, y):
    """G = X'X and c = X'y in np.longdouble."""
    Xl = np.asarray(X, dtype=LD)
    return Xl.T @ Xl, Xl.T @ np.asarray(y, dtype=LD)


def ext_beta_step(G, c, lam, sig2, tau, z):
    """The reference's beta | rest draw (BridgeRegression.cpp:552-575) in np.longdouble:
    A = G + diag(lambda sig2 / tau^2) = U'U by an explicit row Cholesky, then
    beta = U^-1 U'^-1 c + sqrt(sig2) U^-1 z by three explicit triangular solves."""
    A = np.array(G, dtype=LD)
    c, lam, z = (np.asarray(v, dtype=LD) for v in (c, lam, z))
    sig2, tau = LD(sig2), LD(tau)
    p = A.shape[0]
    A[np.diag_indices(p)] += lam * sig2 / (tau * tau)
    Uf = np.zeros((p, p), dtype=LD)
    for k in range(p):
        d = A[k, k] - Uf[:k, k] @ Uf[:k, k]
        if not d > 0:
            raise np.linalg.LinAlgError(f"ext_beta_step: pivot {k} is not positive")
        Uf[k, k] = np.sqrt(d)
        Uf[k, k + 1:] = (A[k, k + 1:] - Uf[:k, k] @ Uf[:k, k + 1:]) / Uf[k, k]
    v = np.zeros(p, dtype=LD)
    for k in range(p):                      # U'v = c
        v[k] = (c[k] - Uf[:k, k] @ v[:k]) / Uf[k, k]
    m = np.zeros(p, dtype=LD)
    x = np.zeros(p, dtype=LD)
    for k in range(p - 1, -1, -1):          # U m = v, U x = z
        m[k] = (v[k] - Uf[k, k + 1:] @ m[k + 1:]) / Uf[k, k]
        x[k] = (z[k] - Uf[k, k + 1:] @ x[k + 1:]) / Uf[k, k]
    return m + np.sqrt(sig2) * x


def ext_rel_err(b, ref):
    """|b - ref| / |ref| (2-norms) with the difference taken in np.longdouble."""
    d = np.asarray(b, dtype=LD) - ref
    return float(np.sqrt(d @ d) / np.sqrt(ref @ ref))


def scaled_cond(G, lam, sig2, tau):
    """kappa_s: the 2-norm condition of A = G + diag(lambda sig2 / tau^2) scaled to unit
    diagonal -- what a Cholesky solve feels (it is blind to diagonal scaling)."""
    A = np.array(G, dtype=np.float64)
    A[np.diag_indices_from(A)] += lam * sig2 / (tau * tau)
    d = 1.0 / np.sqrt(np.diag(A))
    return float(np.linalg.cond(A * d[:, None] * d[None, :]))


# ---------------------------------------------------------------------------------------
# the cases: one sweep each
# ---------------------------------------------------------------------------------------
def case(design, n, p, state="benign", alpha=0.5, t=5, true_sig2=0.0, true_tau=0.0):
    return types.SimpleNamespace(design=design, n=n, p=p, state=state, alpha=alpha, t=t,
                                 true_sig2=true_sig2, true_tau=true_tau)


def case_id(c):
    s = f"{c.design}{c.n}x{c.p}-{c.state}"
    if c.alpha != 0.5:
        s += f"-a{c.alpha}"
    if c.t != 5:
        s += f"-t{c.t}"
    if c.true_sig2:
        s += "-sig2known"
    if c.true_tau:
        s += "-tauknown"
    return s


# The p values sit where the tiling of wide_chain_body changes.  MAXP = 64 in 256 threads (16 x 16
# blocks): 33 first above the small path, 48 a full block edge, 49 one past it, 63, 64.  MAXP = 128
# in 512 threads (16 x 32 blocks): 65 (the second lane entry of the backward solves holds one
# element), 95 / 96 / 97 round the TJ edge, 103, 113 (odd-ka pivots, kb = ka / 2), 127, 128.
# n: p + 1 (G close to singular), 150 (less than one pass of the residual loop), 257 and 513 (one
# row past a whole pass of the 256- and the 512-thread instance).
CHOL_CASES = [
    # ---- MAXP = 64 ----
    case("syn", 150, 33), case("syn", 34, 33, "shrunk"),
    case("syn", 257, 48), case("syn", 150, 48, "zero"),
    case("int", 150, 49), case("int", 50, 49, "shrunk"),
    case("syn", 150, 49, true_sig2=1.5), case("syn", 257, 49, true_tau=0.8),
    case("syn", 150, 63), case("syn", 257, 63, alpha=0.3), case("syn", 64, 63, alpha=0.9),
    case("syn", 257, 64, t=23),
    case("int", 150, 64, "shrunk"), case("int", 65, 64), case("int", 65, 64, "shrunk"),
    # ---- MAXP = 128 ----
    case("syn", 150, 65), case("syn", 66, 65, "shrunk"),
    case("syn", 513, 95), case("syn", 150, 96),
    case("int", 150, 97, "shrunk"), case("int", 98, 97),
    case("syn", 513, 97, true_sig2=1.5), case("syn", 150, 97, true_tau=0.8),
    case("int", 150, 103), case("int", 150, 103, "shrunk"), case("int", 104, 103, "shrunk"),
    case("syn", 513, 103, alpha=0.3), case("syn", 150, 103, alpha=0.9),
    case("syn", 150, 113, "zero"), case("syn", 114, 113),
    case("syn", 513, 127, "shrunk", t=23), case("syn", 128, 127),
    case("int", 150, 128), case("int", 129, 128, "shrunk"), case("syn", 513, 128),
]
ORTHO_CASES = [case("ortho", n, p, s) for n, p in ((200, 70), (150, 33), (160, 128))
               for s in ("benign", "shrunk")]
# k_wide_chains is the LOST = true instantiation: chain 1 of a batch of three forced to the
# shrunk state, one case per instance
BATCH_CASES = [case("int", 150, 103, "shrunk"), case("int", 150, 49, "shrunk", t=23)]
STREAM = 7        # of the single engines
BATCH_STREAM = 5  # of chain 0 of a batch: the forced chain 1 draws on BATCH_STREAM + 1


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**kw)


@functools.lru_cache(maxsize=None)
def _problem(design, n, p):
    X, y, b = DESIGNS[design](n, p)
    return _frozen(X=X, y=y, b_true=b)


@functools.lru_cache(maxsize=None)
def _reference(design, n, p, state, alpha, t, true_sig2, true_tau, stream):
    pr = _problem(design, n, p)
    X, y = pr.X, pr.y
    rng = np.random.default_rng(1000 * n + p)
    beta0, tau0, sig20 = STATES[state](p, pr.b_true, rng)
    # a known scalar is the chain's state, as engine_init_state leaves it
    tau0 = true_tau or tau0
    sig20 = true_sig2 or sig20
    tau, sig2 = tau0, sig20
    if not true_tau:
        tau = oracle.tau_from_sum(oracle.sum_abs_pow(beta0, alpha), p, alpha, HYPER["nu_shape"],
                                  HYPER["nu_rate"], SEED, stream, t)
    if not true_sig2:
        r = y - X @ beta0
        sig2 = oracle.sig2_from_rss(float(r @ r), n, HYPER["sig2_shape"], HYPER["sig2_scale"],
                                    SEED, stream, t)
    lam = oracle.sample_lambda(beta0, alpha, tau, SEED, stream, t)
    z = oracle.normals(p, SEED, stream, t, oracle.KIND_BETA_Z)
    G, c = X.T @ X, X.T @ y
    out = dict(X=X, y=y, beta0=beta0, tau0=tau0, sig20=sig20, tau=tau, sig2=sig2, lam=lam, z=z)
    if design == "ortho":
        out.update(beta_oracle=gibbs.beta_step_ortho(np.diag(G).copy(), c, lam, sig2, tau, z))
    else:
        Gx, cx = ext_gram(X, y)
        ext = ext_beta_step(Gx, cx, lam, sig2, tau, z)
        b = gibbs.beta_step_chol(G, c, lam, sig2, tau, z)
        out.update(beta_oracle=b, beta_ext=ext, e_oracle=ext_rel_err(b, ext),
                   kappa_s=scaled_cond(G, lam, sig2, tau))
    return _frozen(**out)


def reference(c, stream=STREAM):
    """One oracle sweep of case c from its teacher-forced state under the key (SEED, stream)
    and counter c.t: the state (X, y, beta0, tau0, sig20), the draws (tau, sig2, lam, z),
    beta_oracle (fp64) and, for a Cholesky case, beta_ext (np.longdouble), e_oracle, kappa_s."""
    return _reference(c.design, c.n, c.p, c.state, c.alpha, c.t, c.true_sig2, c.true_tau, stream)


def beta_bar(p, e_oracle):
    """The bar of the kernel's beta against ext_beta_step: 32 x the fp64 oracle's own error (a
    different but equally stable summation order: worst-case and random-walk accumulation over
    p <= 128 terms differ by about sqrt(p) ~ 11, doubled for the two solves), and no less than
    p u, one worst-case dot product of length p."""
    return max(32.0 * e_oracle, p * U)


def elementwise_err(b, ref, tau, lam):
    """max_j |b_j - ref_j| / (|ref_j| + sqrt(tau^2 / lambda_j)): the error of each coefficient on
    its own scale (as test_chain_wide_p_woodbury_teacher_forced), so that one wrong coefficient
    cannot hide in the norm."""
    ref = np.asarray(ref, dtype=LD)
    d = np.abs(np.asarray(b, dtype=LD) - ref)
    return float(np.max(d / (np.abs(ref) + np.sqrt(tau * tau / lam))))
