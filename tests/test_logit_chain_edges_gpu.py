"""GPU tests of the logistic chain batch (bb_logit_chain.hip k_logit_chains) at the shapes where
it changes how it holds X or which instance runs (tests/logit_chain_cases.py; the layouts are
pinned by tests/test_logit_chain_layout_cpu.py): X resident in LDS or staged through it in
chunks, last chunks of 1, 2 and 3 rows, n mod 4 in {1, 2, 3}, n = p, n = 4096, p at the
boundaries of the three lambda instances, each with alpha known and sampled.

Three references.  The oracle (oracle/gibbs.py) on the same Philox counters, at the bars of
tests/test_logit_chains_gpu.py.  beta_longdouble on the device's own omega, lambda and tau: the
beta | rest step alone, which is where the row sums are, held to 64 x the error of a numpy fp64
evaluation of the same inputs.  And the kernel against itself: a resident design against the
same rows followed by zero rows, which is staged, bit for bit.
"""
import numpy as np
import pytest

import oracle
from oracle import gibbs
from tests import logit_chain_cases as lc
from tests.test_gpu_parity import flips, rel_err
from tests.test_logit_chains_gpu import same_bits, single_chain

pytestmark = pytest.mark.gpu

SEED = lc.SEED
TRACES = ("beta", "lambda", "tau", "alpha")


def assert_batch(bb, X, y, K, **cfg):
    """tests/test_logit_chains_gpu.py assert_batch's rule for any design: the .C call runs the
    chains one after another where the batch refuses the design, so a ChainBatch of it must
    exist, hold K chains and have a resident kernel."""
    n, p = X.shape
    b = bb.ChainBatch(bb.EngineConfig(n=n, p=p, method=6, seed=SEED, **cfg), K, X, y)
    try:
        assert b.nchains == K and b.resident_per_cu() >= 1
        assert b.threads() == 512
    finally:
        b.close()


def batch_cfg(kw):
    """EngineConfig fields of a .C call's alpha arguments."""
    return dict(true_alpha=kw["alpha"], alpha_a=kw["alpha_a"], alpha_b=kw["alpha_b"]) if kw else {}


# ---------------------------------------------------------------------------------------
# a. teacher-forced single sweeps
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(lc.TEACHER_FORCED), ids=lc.case_id)
def test_teacher_forced_edge_sweeps(gpu_lib, case):
    """Five sweeps of chain 1 of 3, each from the oracle's previous state.

    Against the oracle: tau 1e-12, lambda 1e-11 with no flips, omega 1e-11, beta 1e-10 relative
    L2.  Against beta_longdouble on the device's own omega, lambda, tau: the device's relative
    L2 error is at most 64 x max(numpy fp64's on the same inputs, 2^-50).  The kernel adds up to
    n / 4 <= 1024 terms one after another per partial sum, a random walk of about 32 units;
    numpy's blocked sums carry O(1) units and LAPACK's blocked factor a further factor of 2.

    Measured (MI355X; worst of the five sweeps; relative L2 against long double of the device
    and of numpy fp64, then the device against the oracle):
        1x1      1.7e-16  1.7e-16  7.8e-16      799x16   3.1e-16  7.8e-16  6.1e-16
        2x2      1.0e-16  1.0e-16  6.2e-16      1433x9   3.4e-16  3.5e-16  4.9e-16
        5x5      2.4e-16  1.6e-16  5.6e-16      1434x8   5.0e-16  4.7e-16  6.3e-16
        32x32    3.7e-16  4.3e-16  7.9e-16      1435x9   4.7e-16  3.6e-16  6.1e-16
        33x32    7.7e-16  3.9e-16  7.6e-16      1000x32  5.3e-16  2.9e-16  8.1e-16
        83x13    3.0e-16  3.2e-16  7.2e-16      4093x20  6.1e-16  1.0e-15  1.2e-15
        421x32   3.2e-16  2.9e-16  8.0e-16      4095x32  8.5e-16  1.1e-15  1.2e-15
        422x32   3.4e-16  4.6e-16  9.8e-16      4096x32  5.0e-16  3.8e-16  8.4e-16
        796x16   5.2e-16  5.3e-16  7.1e-16      4096x2   7.7e-16  4.2e-16  1.1e-15
        797x17   2.8e-16  3.2e-16  5.5e-16      4096x1   7.7e-16  5.5e-16  9.2e-16
    The device is within 2 x numpy everywhere: the bar is 64 x max(that, 8.9e-16).

    The cases were also run against three deliberately wrong builds of the kernel: the last four
    rows of the first staged chunk skipped (every staged case failed here, and the whole-chain
    and resident-against-staged tests below), a tail row weighted with omega[q] for omega[r]
    (failed at every n % 4 != 0 whose last chunk has 4 rows or more), and the tail rows left
    out of a thread's second entry (failed at every p = 32 case with n % 4 != 0).
    """
    bb = gpu_lib
    n, p = case
    X, y = lc.edge_problem(n, p)
    seed, s0 = SEED + 83, 4
    o = gibbs.bridge_regression_logit(y, X, 6, burn=0, seed=seed, stream=s0 + 1,
                                      record_state=True)
    st = o["states"]
    assert len(st) == 6
    cfg = bb.EngineConfig(n=n, p=p, method=6, seed=seed, stream=s0)
    b, free = bb.ChainBatch(cfg, 3, X, y), bb.ChainBatch(cfg, 3, X, y)
    try:
        # a refused design would raise above; the batch holds its chains and its kernel fits
        assert b.nchains == 3 and b.resident_per_cu() >= 1 and b.threads() == 512
        for q in (b, free):
            q.init_state()
        worst_dev = worst_np = worst_or = 0.0
        for k in range(1, len(st)):
            t, tau, lam, om, beta, _ = st[k]
            _, tau0, _, _, beta0, alpha0 = st[k - 1]
            b.set_state(1, beta0, tau0, 1.0, alpha0)
            for q in (b, free):
                q.run(t, 1, first_slot=-1)
            s, og = b.state(1), b.omega(1)
            # 1. the project's bars, against the oracle
            assert abs(s["tau"] - tau) <= 1e-12 * tau, t
            assert flips(s["lambda"], lam) == 0, t
            assert np.max(np.abs(s["lambda"] - lam) / lam) <= 1e-11, t
            assert np.max(np.abs(og - om) / om) <= 1e-11, t
            e_or = rel_err(s["beta"], beta)
            assert e_or < 1e-10, (t, e_or)
            assert s["sig2"] == 1.0 and s["alpha"] == 0.5
            # 2. the beta step alone, on the device's own inputs
            z = oracle.normals(p, seed, s0 + 1, t, gibbs.KIND_BETA_Z)
            ref = lc.beta_longdouble(X, y, og, s["lambda"], s["tau"], z)
            e_dev = lc.rel_l2(s["beta"], ref)
            e_np = lc.rel_l2(lc.beta_fp64(X, y, og, s["lambda"], s["tau"], z), ref)
            print(f"{n}x{p} t={t}: device {e_dev:.2e}, numpy fp64 {e_np:.2e}, "
                  f"device against oracle {e_or:.2e}")
            assert e_dev <= 64 * max(e_np, 2.0 ** -50), (t, e_dev, e_np)
            worst_dev, worst_np, worst_or = (max(worst_dev, e_dev), max(worst_np, e_np),
                                             max(worst_or, e_or))
            for c in (0, 2):  # the forced chain's neighbours do not notice
                sc, sf = b.state(c), free.state(c)
                for key in TRACES:
                    assert np.array_equal(sc[key], sf[key]), (c, key, t)
                assert np.array_equal(b.omega(c), free.omega(c)), (c, t)
        print(f"{n}x{p} worst: device {worst_dev:.2e}, numpy fp64 {worst_np:.2e}, "
              f"oracle {worst_or:.2e}")
        for c in range(3):
            assert b.error_flags(c) == 0 and free.error_flags(c) == 0
    finally:
        b.close()
        free.close()


# ---------------------------------------------------------------------------------------
# b. whole chains against the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.WHOLE_KNOWN, ids=lc.case_id)
def test_whole_edge_chains_match_oracle(gpu_lib, case):
    """161 sweeps at the bars of test_logit_chains_gpu.py::test_whole_chains_match_oracle.  The
    numpy oracle and oracle.cpu_logit_chain, two CPU chains with different summation orders,
    differ at these shapes by at most 4.1e-12 on beta and 9.3e-15 on tau.  No n = p here: at
    32 x 32 those two drift apart by 5.9e-6 on beta, so the reference alone would break the
    bars; n = p and n = p + 1 are teacher-forced only.

    Measured (MI355X), worst over the nine shapes and both chains: tau 3.8e-14 (1000 x 32), beta
    1.3e-11 (799 x 16), posterior mean 9.7e-16, against bars of 1e-8, 1e-6 and 1e-8."""
    bb = gpu_lib
    n, p = case
    X, y = lc.edge_problem(n, p)
    K, M, B = 2, 120, 40
    seed = SEED + 84
    assert_batch(bb, X, y, K)
    bb.set_rng_state(seed, 0)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=M, nchains=K, burn=B)
    assert bb.get_rng_state() == (seed, K)
    assert g["beta"].shape == (K, M, p) and g["tau"].shape == (K, M)
    for c in range(K):
        o = lc.oracle_chain((lc.edge_problem, n, p), M, B, seed, c)
        d_tau = np.max(np.abs(g["tau"][c] - o["tau"]) / o["tau"])
        d_beta = np.max(np.abs(g["beta"][c].T - o["beta"]) / np.maximum(np.abs(o["beta"]), 1e-8))
        d_mean = rel_err(g["beta"][c].mean(axis=0), o["beta"].mean(axis=1))
        print(f"{n}x{p} chain {c}: tau {d_tau:.2e}, beta {d_beta:.2e}, mean {d_mean:.2e}")
        assert d_tau < 1e-8
        assert np.all(g["alpha"][c] == 0.5)
        assert d_beta < 1e-6
        assert d_mean < 1e-8
        assert flips(g["lambda"][c].T, o["lambda"]) == 0


@pytest.mark.parametrize("case", lc.WHOLE_SAMPLED, ids=lc.case_id)
def test_alpha_sampled_edge_chains_match_oracle(gpu_lib, case):
    """The staged path under each MH instance, at the bars of
    test_logit_chains_gpu.py::test_alpha_sampled_matches_oracle.  Measured (MI355X): the alpha
    traces equal the oracle's at all four shapes; posterior mean within 8.1e-16."""
    bb = gpu_lib
    n, p = case
    X, y = lc.edge_problem(n, p)
    K, M, B = 2, 120, 40
    seed = SEED + 85
    kw = lc.ALPHA_SAMPLED
    assert_batch(bb, X, y, K, **batch_cfg(kw))
    bb.set_rng_state(seed, 0)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=M, nchains=K, burn=B, **kw)
    assert bb.get_rng_state() == (seed, K)
    for c in range(K):
        o = lc.oracle_chain((lc.edge_problem, n, p), M, B, seed, c, **kw)
        d_alpha = np.max(np.abs(g["alpha"][c] - o["alpha"]))
        d_mean = rel_err(g["beta"][c].mean(axis=0), o["beta"].mean(axis=1))
        print(f"{n}x{p} chain {c}: alpha {d_alpha:.2e}, mean {d_mean:.2e}")
        assert d_alpha < 1e-9
        assert d_mean < 1e-8
        assert len(np.unique(o["alpha"])) > 5  # the MH step moves


# ---------------------------------------------------------------------------------------
# c. resident against staged, bit for bit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, lc.ALPHA_SAMPLED], ids=["alpha_known", "alpha_sampled"])
@pytest.mark.parametrize("case", list(lc.PADDED), ids=lc.case_id)
def test_resident_equals_staged_bit_for_bit(gpu_lib, case, kw):
    """bb_logit_chain.hip's header: the staged sum "takes the same rows in the same order as over
    a resident X".  A resident design with n % 4 = 0 against the same rows followed by zero rows
    with y = 0 up to 4096, which is staged with a chunk seam inside the real rows: a zero row
    adds +0.0 to a partial sum, real row r keeps its index and its r mod 4, omega's counters
    are per row, and n enters nothing else (no sigma^2; tau's shape is nu + p / alpha).  X is
    dyadic, so c = X'(y - 1/2) is exact in any order.  (With a ragged n the real tail rows would
    move from the tail loop to the main loop, across which the header promises nothing.)

    Measured (MI355X): beta, lambda, tau and alpha of both chains are equal bit for bit at all
    four designs (padded rows_lds 308, 600, 600, 1136), alpha known and sampled: the 64-, 32- and
    16-lane instances and their three MH twins.  The header's claim holds as written.
    """
    bb = gpu_lib
    n, p = case
    K, M, B = 2, 120, 40
    seed = SEED + 86
    out = []
    for pad_to in (None, lc.PAD_N):
        X, y = lc.dyadic_problem(n, p, pad_to)
        assert_batch(bb, X, y, K, **batch_cfg(kw))
        bb.set_rng_state(seed, 0)
        out.append(bb.bridge_reg_logit_chains(y, X, nsamp=M, nchains=K, burn=B, **kw))
        assert bb.get_rng_state() == (seed, K)
    small, padded = out
    for k in TRACES:
        assert np.all(np.isfinite(small[k])), k
        d = np.max(np.abs(small[k] - padded[k]))
        print(f"{n}x{p} resident against {lc.PAD_N}x{p} staged, {k}: max difference {d:.2e}")
    assert not np.array_equal(small["beta"][0], small["beta"][1])
    if kw:
        assert len(np.unique(small["alpha"])) > 5
    same_bits(small, padded, f"{n}x{p} padded to {lc.PAD_N}", TRACES)


# ---------------------------------------------------------------------------------------
# d. a staged chain does not depend on K; n above the limit
# ---------------------------------------------------------------------------------------
def test_staged_chain_is_bitwise_the_same_at_any_k(gpu_lib):
    bb = gpu_lib
    n, p, K = 1000, 32, 3
    X, y = lc.edge_problem(n, p)
    assert len(lc.layout(n, p)[1]) == 3
    seed = SEED + 87
    run = dict(nsamp=60, burn=45)
    assert_batch(bb, X, y, K)
    bb.set_rng_state(seed, 0)
    g = bb.bridge_reg_logit_chains(y, X, nchains=K, **run)
    assert bb.get_rng_state() == (seed, K)
    for c in range(K):
        one = single_chain(bb, y, X, seed, c, **run)
        same_bits({k: g[k][c] for k in one}, one, f"chain {c} of {K}")


def test_n_above_the_limit_runs_chain_after_chain(gpu_lib):
    """n = 4097: the batch refuses, and the .C call is two bridge_reg_logit calls."""
    bb = gpu_lib
    n, p = lc.MAX_N + 1, 3
    X, y = lc.edge_problem(n, p)
    with pytest.raises(RuntimeError, match="n <= 4096"):
        bb.ChainBatch(bb.EngineConfig(n=n, p=p, method=6), 2, X, y)
    bb.set_rng_state(SEED + 88, 0)
    g = bb.bridge_reg_logit_chains(y, X, nsamp=12, nchains=2, burn=6)
    assert bb.get_rng_state() == (SEED + 88, 2)
    bb.set_rng_state(SEED + 88, 0)
    for c in range(2):
        one = bb.bridge_reg_logit(y, X, nsamp=12, burn=6)
        same_bits({k: g[k][c] for k in TRACES}, one, f"chain {c}")
