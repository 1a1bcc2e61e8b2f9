"""GPU tests of the wide fused sweep (bb_wide.hip wide_chain_body, 32 < p <= 128, bb_set_tuning
key 25) against references outside the kernel, at the shapes where its tiling changes.

1. Teacher-forced single sweeps (tests/wide_cases.py CHOL_CASES, ORTHO_CASES): set_state, one
   sweep at counter t, state() against the oracle sweep on the same (seed, stream, t).  The bars
   are the project's teacher-forced ones (tests/test_gpu_parity.py): tau and sig2 1e-12
   relative, lambda 0 flips and 1e-11; beta is judged against the np.longdouble draw
   ext_beta_step by e_gpu <= max(32 e_oracle, p u), in the 2-norm and coefficient by coefficient
   on the scale |beta_j| + sqrt(tau^2 / lambda_j), and that bar never exceeds 3 p u kappa_s.
   An orthogonal design's beta is elementwise arithmetic (one sqrt, two divisions): 1e-13
   against beta_step_ortho.  Measured maxima are in DESIGN.md s6.4.
2. Two chain batches (k_wide_chains is the LOST = true instantiation) with chain 1 forced.
3. Free-running chains at partial shapes against gibbs.bridge_regression_stable, with
   compare_chain's whole-chain tolerances, over a sweep count that is no multiple of the
   16-sweep pre-draw block.
4. Launch-split invariance: a sweep's draws depend on its counter, not on where a launch or a
   pre-draw block began.

Every test sets the key through a restoring context and closes every handle in a finally.
"""
import numpy as np
import pytest

from oracle import gibbs
from tests import wide_cases as wc
from tests.conftest import synthetic_problem
from tests.test_chains_gpu import KEYS, compare_chain
from tests.test_wide_chains_gpu import wide_chains

pytestmark = pytest.mark.gpu


def engine_config(bb, c, stream, ortho=False, cap=1):
    return bb.EngineConfig(n=c.n, p=c.p, seed=wc.SEED, stream=stream, trace_capacity=cap,
                           true_alpha=c.alpha, true_sig2=c.true_sig2, true_tau=c.true_tau,
                           ortho=ortho)


def forced_sweep(bb, c, r, ortho=False):
    """One sweep of a fresh engine from the case's state: (state, error word)."""
    e = None
    with wide_chains(bb):
        try:
            e = bb.Engine(engine_config(bb, c, wc.STREAM, ortho), r.X, r.y)
            e.init_state()
            e.set_state(r.beta0, r.tau0, r.sig20, c.alpha)
            e.run(c.t, 1, first_slot=-1)
            return e.state(), e.error_flags()
        finally:
            if e is not None:
                e.close()


def check_scalars_and_lambda(c, r, s):
    assert s["alpha"] == c.alpha
    if c.true_tau:      # the known value comes back unchanged, the other is still drawn
        assert s["tau"] == c.true_tau
        assert s["sig2"] != r.sig20
    if c.true_sig2:
        assert s["sig2"] == c.true_sig2
        assert s["tau"] != r.tau0
    assert abs(s["tau"] - r.tau) <= 1e-12 * r.tau, (s["tau"], r.tau)
    assert abs(s["sig2"] - r.sig2) <= 1e-12 * r.sig2, (s["sig2"], r.sig2)
    assert np.all(np.isfinite(s["lambda"]))
    nf = wc.flips(s["lambda"], r.lam)
    assert nf == 0, f"{nf} lambda decision flips"
    assert np.max(np.abs(s["lambda"] - r.lam) / r.lam) < 1e-11


def check_beta_chol(c, r, beta, tag=""):
    e_gpu = wc.ext_rel_err(beta, r.beta_ext)
    el_gpu = wc.elementwise_err(beta, r.beta_ext, r.tau, r.lam)
    el_or = wc.elementwise_err(r.beta_oracle, r.beta_ext, r.tau, r.lam)
    bar = wc.beta_bar(c.p, r.e_oracle)
    print(f"WIDE_SWEEP {tag}{wc.case_id(c)} p {c.p} e_gpu {e_gpu:.3e} e_oracle {r.e_oracle:.3e} "
          f"kappa_s {r.kappa_s:.3e} elem_gpu {el_gpu:.3e} elem_oracle {el_or:.3e} bar {bar:.3e}")
    assert np.all(np.isfinite(beta))
    assert bar <= 3 * c.p * wc.U * r.kappa_s, (bar, r.kappa_s)
    assert e_gpu <= bar, (e_gpu, r.e_oracle, bar)
    assert el_gpu <= bar, (el_gpu, el_or, bar)


# ---- 1. teacher-forced single sweeps ----
@pytest.mark.parametrize("c", wc.CHOL_CASES, ids=wc.case_id)
def test_forced_sweep_matches_extended_reference(gpu_lib, c):
    r = wc.reference(c)
    s, flags = forced_sweep(gpu_lib, c, r)
    assert flags == 0
    check_scalars_and_lambda(c, r, s)
    check_beta_chol(c, r, s["beta"])


@pytest.mark.parametrize("c", wc.ORTHO_CASES, ids=wc.case_id)
def test_forced_sweep_orthogonal(gpu_lib, c):
    r = wc.reference(c)
    s, flags = forced_sweep(gpu_lib, c, r, ortho=True)
    assert flags == 0
    check_scalars_and_lambda(c, r, s)
    e_gpu = wc.rel_err(s["beta"], r.beta_oracle)
    el_gpu = wc.elementwise_err(s["beta"], r.beta_oracle, r.tau, r.lam)
    print(f"WIDE_SWEEP {wc.case_id(c)} p {c.p} e_gpu {e_gpu:.3e} elem_gpu {el_gpu:.3e}")
    assert e_gpu <= 1e-13, e_gpu
    assert el_gpu <= 1e-13, el_gpu


# ---- 2. the batch kernel, one forced chain among three ----
@pytest.mark.parametrize("c", wc.BATCH_CASES, ids=wc.case_id)
def test_batch_forced_chain(gpu_lib, c):
    """Chain 1 of three from the shrunk state against the oracle sweep on stream + 1 under the
    single sweep's bars; it is bit for bit the single engine's sweep, and chains 0 and 2 are bit
    for bit what the unforced batch draws."""
    bb = gpu_lib
    K = 3
    r = wc.reference(c, stream=wc.BATCH_STREAM + 1)
    base = forced = eng = None
    with wide_chains(bb):
        try:
            cfg = engine_config(bb, c, wc.BATCH_STREAM)
            base = bb.ChainBatch(cfg, K, r.X, r.y)
            forced = bb.ChainBatch(cfg, K, r.X, r.y)
            assert forced.threads() == (256 if c.p <= 64 else 512)
            eng = bb.Engine(engine_config(bb, c, wc.BATCH_STREAM + 1), r.X, r.y)
            for h in (base, forced, eng):
                h.init_state()
            forced.set_state(1, r.beta0, r.tau0, r.sig20, c.alpha)
            eng.set_state(r.beta0, r.tau0, r.sig20, c.alpha)
            for h in (base, forced, eng):
                h.run(c.t, 1, first_slot=-1)
                h.sync()
            st_b = [base.state(k) for k in range(K)]
            st_f = [forced.state(k) for k in range(K)]
            st_e = eng.state()
            assert all(b.error_flags(k) == 0 for b in (base, forced) for k in range(K))
            assert eng.error_flags() == 0
        finally:
            for h in (base, forced, eng):
                if h is not None:
                    h.close()
    s = st_f[1]
    check_scalars_and_lambda(c, r, s)
    check_beta_chol(c, r, s["beta"], tag="batch-")
    for key in ("beta", "lambda", "tau", "sig2", "alpha"):
        assert np.array_equal(s[key], st_e[key]), key
        for k in (0, 2):
            assert np.array_equal(st_f[k][key], st_b[k][key]), (k, key)
    assert not np.array_equal(st_f[1]["beta"], st_b[1]["beta"])


# ---- 3. free-running chains at the partial shapes ----
@pytest.mark.parametrize("n,p,kw", [
    (150, 33, {}),
    (200, 49, dict(sig2_true=1.5)),
    (130, 65, dict(tau_true=0.8)),
    (300, 103, dict(alpha=0.3, nu_shape=0.5, nu_rate=0.5)),
    (260, 127, {}),
    (200, 70, dict(ortho=True)),
    (300, 113, dict(ortho=True)),
], ids=["150x33", "200x49-sig2known", "130x65-tauknown", "300x103-a0.3", "260x127",
        "ortho200x70", "ortho300x113"])
def test_free_running_chain_matches_oracle(gpu_lib, n, p, kw):
    """nsamp = 37 and burn = 21: 58 sweeps, so the last pre-draw block is partial."""
    bb = gpu_lib
    X, y = (wc.ortho_problem(n, p) if kw.get("ortho") else synthetic_problem(n, p))[:2]
    seed = wc.SEED + 50 + p
    with wide_chains(bb):
        bb.set_seed(seed)
        g = bb.bridge_reg_stb(y, X, nsamp=37, burn=21, **kw)
    o = gibbs.bridge_regression_stable(
        y, X, 37, burn=21, alpha=kw.get("alpha", 0.5), nu_shape=kw.get("nu_shape", 2.0),
        nu_rate=kw.get("nu_rate", 2.0), true_sig2=kw.get("sig2_true", 0.0),
        true_tau=kw.get("tau_true", 0.0), ortho=kw.get("ortho", False), seed=seed, stream=0,
        method="chol")
    compare_chain({key: g[key] for key in KEYS}, o)


# ---- 4. launch-split invariance ----
def test_launch_split_invariance(gpu_lib):
    """37 sweeps in one launch against the same sweeps as 16 + 5 + 16: the second and third
    launches start at counters 17 and 22, off the first launch's pre-draw blocks (1, 17, 33)."""
    bb = gpu_lib
    n, p, M = 200, 97, 37
    X, y, _ = synthetic_problem(n, p)
    cfg = bb.EngineConfig(n=n, p=p, seed=wc.SEED + 60, stream=3, trace_capacity=M)
    one = split = None
    with wide_chains(bb):
        try:
            one = bb.Engine(cfg, X, y)
            split = bb.Engine(cfg, X, y)
            for e in (one, split):
                e.init_state()
            s0 = one.state()
            assert np.array_equal(s0["beta"], split.state()["beta"])
            one.run(1, M, first_slot=0)
            for t0, count in ((1, 16), (17, 5), (22, 16)):
                split.run(t0, count, first_slot=t0 - 1)
            tr_one, tr_split = one.trace(0, M), split.trace(0, M)
            st_one, st_split = one.state(), split.state()
            assert one.error_flags() == 0 and split.error_flags() == 0
        finally:
            for e in (one, split):
                if e is not None:
                    e.close()
    for key in KEYS:
        assert np.all(np.isfinite(tr_one[key])), key
        assert np.array_equal(tr_one[key], tr_split[key]), key
        assert np.array_equal(st_one[key], st_split[key]), key
    assert not np.array_equal(tr_one["beta"][:, 0], tr_one["beta"][:, M - 1])
