"""The residual-certified mixed plan on the GPU (bb_nid.hip nid_plan_resid,
k_nid_k2; bb_set_tuning key 29): the mixed plan's first solve on a guessed interval, the
correction's iterates chosen from the fp64 residual, the redo on the a-priori plan when the
residual certifies nothing.  A sweep with the key on and one with it off from the same state draw
the same lambda, tau and sig2 bits and the same beta to the solves' common tolerance.

Shapes: C3's rows with an eighth of its columns (n = 2000, p = 6250, the existing mixed-plan
test's) and a small one (n = 200, p = 2400), both below the default's cost gate, so they run
with the key's test value 2 (the plan wherever a first solve qualifies); the default itself
(key 29 = 1) is checked at C3's own shape, where it engages, and at 2000 x 6250, where it must
not."""
import numpy as np
import pytest

from tests.test_gpu_parity import flips, rel_err
from tests.test_nid_gpu import SEED, _engine

pytestmark = pytest.mark.gpu

KEY = 29
SCALES = (1e-5, 1e-4, 3e-4, 1e-3, 1e-2)   # test_mixed_plan_sweep_equals_fp64_plan's ladder
SHAPES = [(2000, 6250), (200, 2400)]

_problems = {}


def _problem(n, p):
    if (n, p) not in _problems:
        import bench
        X = bench.make_columns(n, 0, p)
        y, btrue = bench.make_problem_y(n, p)
        for a in (X, y, btrue):
            a.setflags(write=False)
        _problems[(n, p)] = (X, y, btrue)
    return _problems[(n, p)]


def _sweep(bb, e, key, t, state=None):
    """One sweep under key 29 = key -> (state, nid_stats, nid_mixed, E-apply passes it ran)."""
    old = bb.set_tuning(KEY, key)
    try:
        s0, m0 = e.nid_stats(), e.nid_mixed()
        if state is not None:
            e.set_state(*state)
        e.run(t, 1)
        e.sync()
        st, mx = e.nid_stats(), e.nid_mixed()
        passes = st["products"] - s0["products"] + mx["products32"] - m0["products32"]
        return e.state(), st, mx, passes
    finally:
        bb.set_tuning(KEY, old)


def _ladder(bb, n, p, key, capsys, scales=SCALES):
    """The state ladder, each state swept with the key on and off (two engines, the same
    states): asserts the parity and returns the per-sweep log and the `on` engine's counters."""
    X, y, btrue = _problem(n, p)
    rng = np.random.default_rng(11)
    on, off = _engine(bb, X, y, n, p), _engine(bb, X, y, n, p)
    log = []
    try:
        on.init_state()
        off.init_state()
        assert on.nid_mixed()["holds_x32"] and off.nid_mixed()["holds_x32"]
        for scale in scales:
            beta, tau = btrue * scale + scale * rng.standard_normal(p), scale
            for t in (3, 4):
                r0 = on.nid_mixed()
                a, sa, ma, pa = _sweep(bb, on, key, t, (beta, tau, 1.0, 0.5))
                o, so, mo, po = _sweep(bb, off, 0, t, (beta, tau, 1.0, 0.5))
                took = ma["resid_sweeps"] - r0["resid_sweeps"]
                redo = ma["redo_sweeps"] - r0["redo_sweeps"]
                err = rel_err(a["beta"], o["beta"])
                log.append(dict(scale=scale, eps=sa["eps"], on=(sa["mode"], ma["k2"]),
                                off=(so["mode"], mo["k2"]), passes=(pa, po), resid=took,
                                redo=redo, ratio=ma["resid_ratio"], err=err))
                with capsys.disabled():
                    print(f"\n[resid {n}x{p} key {key}] {log[-1]}")
                assert sa["eps"] == so["eps"]
                assert a["tau"] == o["tau"] and a["sig2"] == o["sig2"]
                assert np.array_equal(a["lambda"], o["lambda"])
                assert err < 1e-12, log[-1]
                assert took + redo <= 1 and mo["resid_sweeps"] == 0 and mo["redo_sweeps"] == 0
                if redo:   # the a-priori plan, from x = 0: the key-off sweep's plan and passes
                    assert (sa["mode"], ma["k2"]) == (so["mode"], mo["k2"]), log[-1]
                    assert ma["beta32"] == mo["beta32"]
                beta, tau = o["beta"], o["tau"]
        assert on.error_flags() == 0 and off.error_flags() == 0
        return log, on.nid_mixed()
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("n,p", SHAPES)
def test_resid_sweep_equals_a_priori_plan(gpu_lib, capsys, n, p):
    """Key 29 = 2 against 0 over the state ladder: the same lambda, tau, sig2 bits, beta to
    1e-12; resid_sweeps counts the sweeps the residual certified, and at least one state runs
    fewer E-apply passes than the a-priori plan."""
    log, m = _ladder(gpu_lib, n, p, 2, capsys)
    assert m["resid_sweeps"] == sum(r["resid"] for r in log) >= 2, (log, m)
    assert any(r["resid"] and r["passes"][0] < r["passes"][1] for r in log), log


@pytest.mark.parametrize("n,p", SHAPES)
def test_wrong_guess_is_redone(gpu_lib, capsys, n, p):
    """Key 29 = 8 divides the guess factor by 16^6 (phi = 4.8e-7), so the first solve's interval
    is far too small: sweeps whose residual certifies no K2 are redone on the a-priori plan
    (redo_sweeps > 0) with the same bars, and no error flag."""
    log, m = _ladder(gpu_lib, n, p, 8, capsys)
    assert m["redo_sweeps"] == sum(r["redo"] for r in log) > 0, (log, m)


def test_default_engages_at_c3_shape_only(gpu_lib, capsys):
    """The default (key 29 = 1) takes the plan at C3's shape, n = 2000, p = 50000 -- same bars --
    and leaves the 2000 x 6250 engines, whose existing tests pin the a-priori plan, alone."""
    bb = gpu_lib
    assert bb.set_tuning(KEY, -1) == 1
    log, m = _ladder(bb, 2000, 50000, 1, capsys, scales=(3e-4, 1e-3))
    assert m["resid_sweeps"] >= 1, (log, m)
    log, m = _ladder(bb, 2000, 6250, 1, capsys, scales=(3e-4,))
    assert m["resid_sweeps"] == 0 and m["redo_sweeps"] == 0, (log, m)
    assert all(r["on"] == r["off"] for r in log), log


def test_resid_teacher_forced_against_oracle(gpu_lib, capsys):
    """Sweeps on the residual-certified plan teacher-forced against the oracle's Cholesky-based
    Woodbury draw, with test_mixed_plan_teacher_forced_against_oracle's bars (beta 1e-10 relative
    L2, lambda / tau / sig2 1e-11, no flips)."""
    from tests.test_steady_state_gpu import oracle_sweep
    bb = gpu_lib
    n, p = SHAPES[1]
    X, y, btrue = _problem(n, p)
    rng = np.random.default_rng(3)
    e = _engine(bb, X, y, n, p)
    try:
        e.init_state()
        beta, tau, sig2 = btrue * 1e-3 + 1e-3 * rng.standard_normal(p), 1e-3, 1.0
        took = 0
        for t in (1001, 1002, 1003):
            r0 = e.nid_mixed()["resid_sweeps"]
            g, st, mx, _ = _sweep(bb, e, 2, t, (beta, tau, sig2, 0.5))
            b, lam, tau, sig2 = oracle_sweep(X, y, beta, tau, sig2, 0.5, t, SEED, 0)
            took += mx["resid_sweeps"] - r0
            with capsys.disabled():
                print(f"\n[resid oracle t={t}] eps={st['eps']:.3g} K1={st['mode']} K2={mx['k2']} "
                      f"ratio={mx['resid_ratio']:.2e} beta rel {rel_err(g['beta'], b):.2e}")
            assert abs(g["tau"] - tau) / tau < 1e-11 and abs(g["sig2"] - sig2) / sig2 < 1e-11
            assert flips(g["lambda"], lam) == 0
            assert np.max(np.abs(g["lambda"] - lam) / lam) < 1e-11
            assert rel_err(g["beta"], b) < 1e-10
            beta = b
        assert took >= 1, took
        assert e.error_flags() == 0
    finally:
        e.close()


def test_resid_chain_is_reproducible(gpu_lib):
    """Two engines, 30 free sweeps each from the same mid-regime state under key 29 = 2: the same
    bits and the same counters (every choice is a device function of the chain's state)."""
    bb = gpu_lib
    n, p = SHAPES[0]
    X, y, btrue = _problem(n, p)
    rng = np.random.default_rng(9)
    state = (btrue * 3e-4 + 3e-4 * rng.standard_normal(p), 3e-4, 1.0, 0.5)
    out = []
    old = bb.set_tuning(KEY, 2)
    try:
        for _ in range(2):
            e = _engine(bb, X, y, n, p)
            e.init_state()
            e.set_state(*state)
            e.run(1, 30, first_slot=-1)
            e.sync()
            out.append((e.state(), e.nid_stats(), e.nid_mixed()))
            assert e.error_flags() == 0
            e.close()
    finally:
        bb.set_tuning(KEY, old)
    (a, sa, ma), (b, sb, mb) = out
    assert sa == sb and ma == mb, (sa, sb, ma, mb)
    assert ma["resid_sweeps"] >= 10, ma
    for k in ("beta", "lambda"):
        assert np.array_equal(a[k], b[k]), k
    assert a["tau"] == b["tau"] and a["sig2"] == b["sig2"]


def _run_group(bb, X, y, n, p, world, state_scale):
    per = p // world
    shards = []
    for r in range(world):
        cfg = bb.EngineConfig(n=n, p=p, p_local=per, j0=r * per, rank=r, world=world, seed=SEED,
                              stream=0, true_alpha=0.5, trace_capacity=1)
        shards.append(bb.Engine(cfg, np.asfortranarray(X[:, r * per:(r + 1) * per]), y))
    grp = bb.ShardGroup(shards)
    try:
        grp.init_state()
        grp.run(1, 6)
        grp.sync()
        assert all(e.error_flags() == 0 for e in shards)
        return [e.state() for e in shards], [e.nid_stats() for e in shards]
    finally:
        grp.close()
        for e in shards:
            e.close()


def test_shards_and_group_members_keep_their_plans(gpu_lib):
    """A 2-member shard group, and an engine running the shard protocol (bb_set_tuning key 9 with
    a one-rank communicator), draw the same bits with key 29 = 2 as with 0: they decide the fp64
    plan only."""
    bb = gpu_lib
    n, p = 200, 2400
    X, y, btrue = _problem(n, p)
    outs = []
    for key in (2, 0):
        old = bb.set_tuning(KEY, key)
        try:
            outs.append(_run_group(bb, X, y, n, p, 2, 3e-4))
        finally:
            bb.set_tuning(KEY, old)
    (pa, sa), (pb, sb) = outs
    assert sa == sb and sa[0]["cheb_sweeps"] >= 4, (sa, sb)
    for qa, qb in zip(pa, pb):
        for k in ("beta", "lambda"):
            assert np.array_equal(qa[k], qb[k]), k
        assert qa["tau"] == qb["tau"] and qa["sig2"] == qb["sig2"]
    rng = np.random.default_rng(4)
    state = (btrue * 1e-3 + 1e-3 * rng.standard_normal(p), 1e-3, 1.0, 0.5)
    outs = []
    old9 = bb.set_tuning(9, 1)
    try:
        for key in (2, 0):
            old = bb.set_tuning(KEY, key)
            try:
                e = _engine(bb, X, y, n, p)
                e.comm_init(bb.Engine.comm_unique_id())
                e.init_state()
                e.set_state(*state)
                e.run(1, 4, first_slot=-1)
                e.sync()
                outs.append((e.state(), e.nid_stats(), e.nid_mixed()))
                assert e.error_flags() == 0
                e.close()
            finally:
                bb.set_tuning(KEY, old)
    finally:
        bb.set_tuning(9, old9)
    (a, sa, ma), (b, sb, mb) = outs
    assert sa == sb and ma == mb and ma["resid_sweeps"] == 0 and ma["mixed_sweeps"] == 0
    assert sa["cheb_sweeps"] >= 1, sa
    for k in ("beta", "lambda"):
        assert np.array_equal(a[k], b[k]), k
    assert a["tau"] == b["tau"] and a["sig2"] == b["sig2"]
