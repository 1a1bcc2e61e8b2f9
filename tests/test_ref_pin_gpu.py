"""Every device path that draws lambda, against what the REFERENCE's compiled retstable_LD
returned on the same variates (tests/golden/ref_retstable.npz).

These tests read the fixture only: no oracle call, no reference tree.  The bars are the
device-vs-oracle bars of tests/test_gpu_parity.py (the oracle is bit-equal to the fixture,
tests/test_ref_pin_cpu.py): no accept/reject decision flip (relative 1e-6), every value
within relative 1e-11 (libm against ocml in pow / exp / log / sin), no device error flag
(engines and chain batches report theirs; bb_retstable_batch fails on a raised flag;
bb_sample_lambda does not read its error word back, so there the values carry the bar:
finite, positive, no flip).

Draw j depends on (beta_j, alpha, tau, key, t, j0 + j) alone, so a launch of p > 1100
coefficients whose first 1100 are a pool's must return the pool's lambda there: that is how
the launches that only exist above 40 000 or 50 000 coefficients are held to the fixture.
bb.kernel_instance("lambda") names the kernel a launch took, and the tests require the one
they are about.

Sweeps are teacher-forced so that lambda depends on the fixture alone: tau is known
(true_tau = the pool's), alpha known, the state is set to the pool's beta, and lambda is
drawn from that state before beta moves (oracle/gibbs.py bridge_regression_stable: tau,
sig2, lambda, beta).  The design does not enter lambda.
"""
import contextlib

import numpy as np
import pytest

from tests.golden import make_ref_golden as mk
from tests.tuning import tuning

pytestmark = pytest.mark.gpu

SEED = mk.SEED
WIDE_KEY = 25
SIG2 = 1.3


@pytest.fixture(scope="module")
def fx():
    return mk.load()


def flips(a, b, tol=1e-6):
    a, b = np.asarray(a), np.asarray(b)
    return int(np.sum(np.abs(a - b) > tol * np.maximum(np.abs(b), 1e-300)))


def check(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.all(np.isfinite(got)) and np.all(got > 0), what
    nf = flips(got, want)
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f"{what}: {len(want)} draws, {nf} flips, max rel err {err:.3e}")
    assert nf == 0, f"{what}: {nf} decision flips out of {len(want)} at " \
                    f"{np.flatnonzero(np.abs(got - want) > 1e-6 * np.abs(want))[:8]}"
    assert err < 1e-11, (what, err)


def design(n, p, seed=3):
    rng = np.random.default_rng(seed + n + p)
    X = rng.standard_normal((n, p))
    return np.asfortranarray(X), rng.standard_normal(n)


# ---------------------------------------------------------------------------
# the kernel-level entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2, 8, 64])
def test_retstable_batch_block_a(gpu_lib, fx, group):
    bb = gpu_lib
    x = bb.retstable_batch(fx["A_alpha"], fx["A_V0"], fx["A_h"], seed=SEED, stream=0, t=0,
                           group=group)
    check(x, fx["A_x"], f"retstable_batch group {group}")
    one = fx["A_alpha"] == 1.0
    assert np.array_equal(x[one], fx["A_V0"][one])


def test_retstable_ld_block_a(gpu_lib, fx):
    """The .C("retstable_LD") entry draws call k of a seed on (stream k, t = 0, j = index):
    after set_seed(SEED) its first call is on block A's counters."""
    bb = gpu_lib
    state = bb.get_rng_state()
    try:
        bb.set_seed(SEED)
        x = bb.retstable_ld(len(fx["A_h"]), alpha=fx["A_alpha"], V0=fx["A_V0"], h=fx["A_h"])
        assert bb.get_rng_state() == (SEED, 1)
    finally:
        bb.set_rng_state(*state)
    check(x, fx["A_x"], "retstable_ld")


POOL_CASES = [("p0", None), ("p0", 20), ("p0", 32), ("p0", 33), ("p0", 128), ("p1", None),
              ("p1", 20), ("p1", 33), ("p2", None), ("p2", 32), ("p2", 128), ("p0j", None),
              ("p0j", 33)]


@pytest.mark.parametrize("group", [0, 8])
@pytest.mark.parametrize("name,p", POOL_CASES)
def test_sample_lambda_pools(gpu_lib, fx, name, p, group):
    """(Up to 50 000 coefficients the speculative launch draws whatever `group` says; the
    explicit groups that select a kernel are in test_sample_lambda_large.)"""
    bb = gpu_lib
    q = fx["pools"][name]
    p = len(q["beta"]) if p is None else p
    lam = bb.sample_lambda(q["beta"][:p], q["alpha"], q["tau"], SEED, q["stream"], q["t"],
                           j0=q["j0"], group=group)
    check(lam, q["lam"][:p], f"sample_lambda {name}[:{p}] group {group}")
    zero = q["beta"][:p] == 0.0
    assert zero.sum() >= 1  # the h = 0 draws (the `m != 0` guard) are in every prefix


# the lambda launch modes bb_set_tuning offers that a launch of at most 1100 coefficients can
# take: key 5, the lanes per coefficient of the speculative launch (64 by default up to
# p = 1024, 16 above); key 4 bit 0, its 4-waves-per-SIMD instance
@pytest.mark.parametrize("key,value", [(5, 4), (5, 8), (5, 16), (5, 32), (5, 64), (4, 0), (4, 1)])
@pytest.mark.parametrize("name,p", [("p0", None), ("p1", 33), ("p2", None)])
def test_sample_lambda_launch_modes(gpu_lib, fx, name, p, key, value):
    bb = gpu_lib
    q = fx["pools"][name]
    p = len(q["beta"]) if p is None else p
    with tuning(bb, key, value):
        lam = bb.sample_lambda(q["beta"][:p], q["alpha"], q["tau"], SEED, q["stream"], q["t"],
                               j0=q["j0"])
    check(lam, q["lam"][:p], f"sample_lambda {name}[:{p}] key {key} = {value}")


@contextlib.contextmanager
def tunings(bb, pairs):
    with contextlib.ExitStack() as st:
        for key, value in pairs:
            st.enter_context(tuning(bb, key, value))
        yield


def padded(q, p):
    """The pool's beta with filler behind (the pool repeated): beta of a launch of p draws."""
    return np.resize(q["beta"], p)


# The launches above 40 000 coefficients (bb_kernels.hip launch_lambda): the continuous-
# batching kernel with its sampler inlined and the tail's lanes lent (k_lambda_cl, the default),
# without lending (key 15 = 0: k_lambda_cb_in), out of line at 3 and 4 waves per SIMD (key 4
# bit 2 off: k_lambda_cb, bit 1: k_lambda_cb_o4), the 8-lane speculative launch (key 4 bit 3
# off, up to 50 000).  Above 50 000, with bit 3 of key 4 off, an explicit group other than 8
# takes k_lambda<G> (inner-attempt speculation).  That launch records no kernel name, so its
# cases (kernel None) require that the name recorded by a 64-lane speculative launch made just
# before is still the recorded one: none of the noted kernels drew.
LARGE = [
    (40001, 0, (), "k_lambda_cl<"),
    (40001, 0, ((15, 0),), "k_lambda_cb_in<"),
    (40001, 0, ((4, 8),), "k_lambda_cb<"),
    (40001, 0, ((4, 10),), "k_lambda_cb_o4<"),
    (40001, 0, ((4, 4),), "k_lambda_spec<8"),
    (40001, 0, ((4, 5),), "k_lambda_spec_o4<8"),
    (50001, 0, (), "k_lambda_cl<"),
    (50001, 8, (), "k_lambda_cl<"),
    (50001, 8, ((15, 0),), "k_lambda_cb_in<"),
    (50001, 8, ((4, 0),), "k_lambda_cb<"),
    (50001, 8, ((4, 2),), "k_lambda_cb_o4<"),
    (50001, 8, ((4, 4),), "k_lambda_cl<"),
    (50001, 1, ((4, 4),), None),
    (50001, 4, ((4, 4),), None),
    (50001, 16, ((4, 4),), None),
    (50001, 64, ((4, 4),), None),
    (50001, 2, ((4, 0),), None),
    (50001, 32, ((4, 0),), None),
]


@pytest.mark.parametrize("p,group,keys,kernel", LARGE)
@pytest.mark.parametrize("name", ["p0", "p2", "p0j"])
def test_sample_lambda_large(gpu_lib, fx, name, p, group, keys, kernel):
    bb = gpu_lib
    q = fx["pools"][name]
    with tunings(bb, keys):
        if kernel is None:
            bb.sample_lambda(q["beta"][:33], q["alpha"], q["tau"], SEED, q["stream"], q["t"])
            before = bb.kernel_instance("lambda")
            assert "k_lambda_spec<64" in before, before
        lam = bb.sample_lambda(padded(q, p), q["alpha"], q["tau"], SEED, q["stream"], q["t"],
                               j0=q["j0"], group=group)
        got = bb.kernel_instance("lambda")
    assert np.all(np.isfinite(lam)) and np.all(lam > 0)
    if kernel is not None:
        assert kernel in got, (got, kernel)
    else:  # k_lambda<G>: the launch that notes nothing
        assert got == before, (got, before)
    check(lam[:len(q["lam"])], q["lam"], f"sample_lambda {name} in p {p} group {group} {keys}")


# ---------------------------------------------------------------------------
# one teacher-forced sweep per lambda kernel
# ---------------------------------------------------------------------------
def forced_lambda(bb, q, n, p, X=None, y=None, **cfg_kw):
    """lambda of one sweep of an engine on the pool's key and t, from the pool's state."""
    if X is None:
        X, y = design(n, p)
    cfg = bb.EngineConfig(n=n, p=p, seed=SEED, stream=q["stream"], true_tau=q["tau"],
                          true_alpha=q["alpha"], trace_capacity=1, **cfg_kw)
    e = bb.Engine(cfg, X, y)
    try:
        e.init_state()
        e.set_state(padded(q, p), q["tau"], SIG2, q["alpha"])
        e.run(q["t"], 1, first_slot=-1)
        e.sync()
        s = e.state()
        assert e.error_flags() == 0
        assert s["tau"] == q["tau"] and s["alpha"] == q["alpha"]
        return s["lambda"], e.method(), dict(e.launch_counts(), kernel=bb.kernel_instance("lambda"))
    finally:
        e.close()


@pytest.mark.parametrize("name", ["p0", "p1", "p2"])
@pytest.mark.parametrize("p", [20, 32])
def test_sweep_small_fused(gpu_lib, fx, name, p):
    """p <= 32, p <= n, alpha known: the whole sweep in one workgroup (bb_small.hip)."""
    q = fx["pools"][name]
    lam, method, _ = forced_lambda(gpu_lib, q, 40, p)
    assert method == 1
    check(lam, q["lam"][:p], f"small fused {name} p {p}")


@pytest.mark.parametrize("name", ["p0", "p1", "p2"])
def test_sweep_dense_chol(gpu_lib, fx, name):
    """32 < p <= n: the general dense path, lambda by the speculative launch (64 lanes)."""
    q = fx["pools"][name]
    lam, method, _ = forced_lambda(gpu_lib, q, 80, 64)
    assert method == 1
    check(lam, q["lam"][:64], f"dense chol {name}")


@pytest.mark.parametrize("name", ["p0", "p1", "p2"])
def test_sweep_dense_woodbury(gpu_lib, fx, name):
    """p = 1100 > n: the Woodbury path, the lambda launch past 1024 columns (16 lanes)."""
    q = fx["pools"][name]
    lam, method, _ = forced_lambda(gpu_lib, q, 48, 1100)
    assert method == 2
    check(lam, q["lam"], f"dense woodbury {name}")


@pytest.mark.parametrize("key,value", [(7, 0), (7, 1), (7, 2), (6, 0), (17, 0), (17, 2),
                                       (8, 0), (4, 1), (5, 8), (5, 64)])
def test_sweep_dense_woodbury_launch_modes(gpu_lib, fx, key, value):
    """The Woodbury sweep's lambda launch modes at 16 lanes: fused with the X u stream (key
    7 = 1, 2; the default 3 is mode 2 here: the first sweep after init_state fuses), on its own
    (key 7 = 0, key 6 = 0), with the bound sums folded in or not (key 17), under the gated
    protocol (key 8 = 0), and the speculative launch's instances (keys 4, 5)."""
    q = fx["pools"]["p0"]
    with tuning(gpu_lib, key, value):
        lam, method, counts = forced_lambda(gpu_lib, q, 48, 1100)
    print(f"key {key} = {value}: launches {counts}")
    assert method == 2 and counts["lambda_xu"] + counts["lambda_alone"] == 1
    assert ("k_lambda_xu" if counts["lambda_xu"] else "k_lambda_spec") in counts["kernel"]
    if key == 7 or key == 6:  # the launch the mode names is the one that drew
        assert counts["lambda_xu"] == (1 if (key, value) in ((7, 1), (7, 2)) else 0)
    check(lam, q["lam"], f"dense woodbury key {key} = {value}")


# The Woodbury sweep at 8 lanes per coefficient (40 000 < p <= 50 000, bb_kernels.hip
# launch_lambda_xu): the split launch with the wave-adaptive sampler (k_lambda_xs, the
# default, key 7 = 3), one launch drawing then streaming with that sampler (key 7 = 1, 2:
# k_lambda_xw) or with fixed 8-lane groups (key 13 = 0: k_lambda_xu<8, .>; the 4-wave
# instance under key 4 bit 0), and the launch of its own (key 7 = 0 or key 6 = 0: the
# continuous-batching kernels of test_sample_lambda_large, in LAMBDA_WOODBURY mode).
WIDE_WOODBURY = [
    ((), "k_lambda_xs<"),
    (((7, 2),), "k_lambda_xw<"),
    (((7, 1),), "k_lambda_xw<"),
    (((13, 0),), "k_lambda_xu<8"),
    (((7, 1), (13, 0)), "k_lambda_xu<8"),
    (((4, 13),), "k_lambda_xu_o4<8"),
    (((7, 0),), "k_lambda_cl<"),
    (((6, 0),), "k_lambda_cl<"),
    (((7, 0), (15, 0)), "k_lambda_cb_in<"),
    (((7, 0), (4, 8)), "k_lambda_cb<"),
    (((7, 0), (4, 10)), "k_lambda_cb_o4<"),
    (((7, 0), (4, 4)), "k_lambda_spec<8"),
]


@pytest.fixture(scope="module")
def wide_design():
    return design(48, 40001)


@pytest.mark.parametrize("keys,kernel", WIDE_WOODBURY)
@pytest.mark.parametrize("name", ["p0", "p2"])
def test_sweep_dense_woodbury_8_lanes(gpu_lib, fx, wide_design, name, keys, kernel):
    q = fx["pools"][name]
    X, y = wide_design
    with tunings(gpu_lib, keys):
        lam, method, counts = forced_lambda(gpu_lib, q, 48, 40001, X=X, y=y)
    print(f"{keys}: {counts}")
    assert method == 2 and counts["lambda_xu"] + counts["lambda_alone"] == 1
    assert kernel in counts["kernel"], (counts, kernel)
    assert np.all(np.isfinite(lam)) and np.all(lam > 0)
    check(lam[:1100], q["lam"], f"dense woodbury p 40001 {name} {keys}")


@pytest.mark.parametrize("name", ["p0", "p1", "p2"])
@pytest.mark.parametrize("p", [33, 128])
def test_sweep_wide_fused(gpu_lib, fx, name, p):
    """32 < p <= 128 under set_wide_chains(True): the sweep in one workgroup (bb_wide.hip)."""
    bb = gpu_lib
    q = fx["pools"][name]
    old = bb.set_wide_chains(True)
    try:
        lam, method, _ = forced_lambda(bb, q, p + 1, p)
    finally:
        bb.set_wide_chains(old)
    assert bb.set_tuning(WIDE_KEY, -1) == int(old)
    assert method == 1
    check(lam, q["lam"][:p], f"wide fused {name} p {p}")


@pytest.mark.parametrize("name", ["p0", "p1"])
def test_sweep_sparse(gpu_lib, fx, name):
    """A CSC design, p = 1100 > n: the sparse Woodbury engine."""
    sps = pytest.importorskip("scipy.sparse")
    q = fx["pools"][name]
    n, p = 48, 1100
    rng = np.random.default_rng(8)
    X = sps.random(n, p, density=0.15, random_state=rng, format="csc",
                   data_rvs=rng.standard_normal)
    lam, method, _ = forced_lambda(gpu_lib, q, n, p, X=X, y=rng.standard_normal(n))
    assert method == 5
    check(lam, q["lam"], f"sparse {name}")


@pytest.mark.parametrize("name", ["p0", "p2"])
def test_sweep_logit(gpu_lib, fx, name):
    """The logistic engine (method 6): lambda with the Polya-Gamma draws as trailing
    workgroups of the same launch."""
    q = fx["pools"][name]
    n, p = 120, 64
    X = design(n, p)[0] * 1e-3  # x_i' beta of the Polya-Gamma draws stays moderate
    y = (np.random.default_rng(4).uniform(size=n) < 0.5).astype(np.float64)
    lam, method, _ = forced_lambda(gpu_lib, q, n, p, X=X, y=y, method=6)
    assert method == 6
    check(lam, q["lam"][:p], f"logit {name}")


@pytest.mark.parametrize("name", ["p0", "p1"])
def test_sweep_shard_group(gpu_lib, fx, name):
    """Two column shards on one device: the second member draws on counters j0 + j, j0 = 550."""
    bb = gpu_lib
    q = fx["pools"][name]
    n, p, world = 48, 1100, 2
    X, y = design(n, p)
    per = p // world
    shards = []
    for r in range(world):
        cfg = bb.EngineConfig(n=n, p=p, p_local=per, j0=r * per, rank=r, world=world, seed=SEED,
                              stream=q["stream"], true_tau=q["tau"], true_alpha=q["alpha"])
        shards.append(bb.Engine(cfg, np.asfortranarray(X[:, r * per:(r + 1) * per]), y))
    grp = bb.ShardGroup(shards)
    try:
        grp.init_state()
        for r, e in enumerate(shards):
            e.set_state(q["beta"][r * per:(r + 1) * per], q["tau"], SIG2, q["alpha"])
        grp.run(q["t"], 1)
        grp.sync()
        lam = np.concatenate([e.state()["lambda"] for e in shards])
        assert all(e.error_flags() == 0 for e in shards)
    finally:
        grp.close()
        for e in shards:
            e.close()
    check(lam[:per], q["lam"][:per], f"shard 0 {name}")
    check(lam[per:], q["lam"][per:], f"shard 1 {name}")


@pytest.mark.parametrize("p,wide", [(20, False), (32, False), (33, True), (103, True)])
def test_sweep_chain_batch(gpu_lib, fx, p, wide):
    """Three chains in one launch, chain c under stream 5 + c, each forced to its own pool:
    the small batch kernel, and the wide one under set_wide_chains(True)."""
    bb = gpu_lib
    pools = [fx["pools"][f"c{c}"] for c in range(3)]
    q0 = pools[0]
    assert [q["stream"] for q in pools] == [q0["stream"] + c for c in range(3)]
    n = p + 8
    X, y = design(n, p)
    old = bb.set_wide_chains(wide)
    b = None
    try:
        cfg = bb.EngineConfig(n=n, p=p, seed=SEED, stream=q0["stream"], true_tau=q0["tau"],
                              true_alpha=q0["alpha"], trace_capacity=2)
        b = bb.ChainBatch(cfg, 3, X, y)
        b.init_state()
        for c, q in enumerate(pools):
            b.set_state(c, q["beta"][:p], q["tau"], SIG2, q["alpha"])
        b.run(q0["t"], 1, 0, 1, 1)
        b.sync()
        got = [(b.state(c)["lambda"], b.trace(c, 0, 1)["lambda"][:, 0]) for c in range(3)]
        assert all(b.error_flags(c) == 0 for c in range(3))
    finally:
        if b is not None:
            b.close()
        bb.set_wide_chains(old)
    for c, q in enumerate(pools):
        check(got[c][0], q["lam"][:p], f"chain batch p {p} chain {c}")
        assert np.array_equal(got[c][0], got[c][1])
