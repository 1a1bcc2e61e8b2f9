"""The tilted-stable sampler and lambda | beta, tau pinned to the reference's own compiled
``retstable_LD``.

tests/golden/ref_retstable.npz holds what the reference's unmodified Code/C/retstable.cpp
returned when it drew from the oracle's variates (oracle/ref.py).  The fixture tests run
everywhere and require the oracle to reproduce it BIT FOR BIT, attempt counts included (the
measured state: same compiler flags, same libm).  The live tests run where the reference
tree is present: they replay fresh draws through the compiled reference and regenerate the
fixture.
"""
import numpy as np
import pytest

import oracle
from oracle import ref
from tests.golden import make_ref_golden as mk

SEED = mk.SEED


@pytest.fixture(scope="module")
def fx():
    return mk.load()


@pytest.fixture(scope="module")
def live():
    """The compiled reference sampler, built on first use; skips where it cannot be."""
    if not ref.available():
        pytest.skip("reference sampler not available: " + ref.why_unavailable())
    return ref


# ---------------------------------------------------------------------------
# the fixture against the oracle (everywhere)
# ---------------------------------------------------------------------------
def test_fixture_shape(fx):
    """The fixture is what the generator describes (its edges are asserted when it is made)."""
    a, v, h = mk.block_a_inputs()
    assert int(fx["seed"][0]) == SEED
    assert np.array_equal(fx["A_alpha"], a) and np.array_equal(fx["A_V0"], v)
    assert np.array_equal(fx["A_h"], h)
    assert len(h) >= 2300 and set(fx["pools"]) == set(mk.POOLS)
    assert fx["A_n_outer"].max() >= 5 and fx["A_n_outer"].max() <= mk.MAX_OUTER
    for k, b in enumerate(mk.beta_pools()):
        assert np.array_equal(fx[f"B_beta{k}"], b)
        assert np.sum(b[:32] == 0.0) == 2 and np.sum(b[:20] == 0.0) == 1
    one = fx["A_alpha"] == 1.0
    assert one.sum() == 9 and np.array_equal(fx["A_x"][one], fx["A_V0"][one])
    assert not np.any(fx["A_n_outer"][one])


def test_oracle_reproduces_reference_draws(fx):
    """Block A: oracle.retstable_batch is bit-equal to the reference's retstable_LD, and
    every draw takes the same outer and inner attempts."""
    x = oracle.retstable_batch(fx["A_alpha"], fx["A_V0"], fx["A_h"], seed=SEED, stream=0, t=0)
    bad = np.flatnonzero(x != fx["A_x"])
    assert bad.size == 0, [(i, fx["A_alpha"][i], fx["A_V0"][i], fx["A_h"][i]) for i in bad[:8]]
    assert np.array_equal(x, fx["A_x"])
    x2, no, ni = oracle.retstable_counts(fx["A_alpha"], fx["A_V0"], fx["A_h"], SEED, 0, 0)
    assert np.array_equal(x2, fx["A_x"])
    assert np.array_equal(no, fx["A_n_outer"]) and np.array_equal(ni, fx["A_n_inner"])


@pytest.mark.parametrize("name", list(mk.POOLS))
def test_oracle_reproduces_reference_lambda(fx, name):
    """Block B: oracle.sample_lambda is bit-equal to 2 retstable_LD(beta^2/tau^2, alpha/2) of
    the reference on every pool, on every prefix, with the same attempts."""
    q = fx["pools"][name]
    lam = oracle.sample_lambda(q["beta"], q["alpha"], q["tau"], SEED, q["stream"], q["t"],
                               j0=q["j0"])
    bad = np.flatnonzero(lam != q["lam"])
    assert bad.size == 0, [(int(j), q["beta"][j]) for j in bad[:8]]
    for p in (20, 32, 33, 128):
        assert np.array_equal(oracle.sample_lambda(q["beta"][:p], q["alpha"], q["tau"], SEED,
                                                   q["stream"], q["t"], j0=q["j0"]), q["lam"][:p])
    no, ni = oracle.lambda_counts(q["beta"], q["alpha"], q["tau"], SEED, q["stream"], q["t"],
                                  j0=q["j0"])
    assert np.array_equal(no, q["n_outer"]) and np.array_equal(ni, q["n_inner"])


def test_tape_lists_the_draw(fx):
    """bbo_retstable_tape: the value and counts of bbo_retstable, three items per inner and
    two per outer attempt, uniform first in each."""
    for i in (0, 5, 700, 1500, 2100, len(fx["A_h"]) - 1):
        a, v, h = fx["A_alpha"][i], fx["A_V0"][i], fx["A_h"][i]
        tp = oracle.retstable_tape(h, a, v, SEED, 0, 0, i, cap=4)  # grows past a short cap
        assert tp["x"] == fx["A_x"][i]
        assert tp["n_outer"] == fx["A_n_outer"][i] and tp["n_inner"] == fx["A_n_inner"][i]
        assert tp["inner"].sum() == tp["n_inner"] and len(tp["inner"]) == tp["n_outer"]
        assert len(tp["kind"]) == 3 * tp["n_inner"] + 2 * tp["n_outer"]
        assert np.all((tp["value"][tp["kind"] == oracle.TAPE_UNIF] > 0)
                      & (tp["value"][tp["kind"] == oracle.TAPE_UNIF] < 1))


# ---------------------------------------------------------------------------
# live replay through the compiled reference (where its tree is present)
# ---------------------------------------------------------------------------
def _replay_all(h, a, v, stream, t):
    r = ref.retstable_ref(h, a, v, seed=SEED, stream=stream, t=t, j=np.arange(len(h)))
    assert not np.any(r["flags"]), np.unique(r["flags"])
    assert np.array_equal(r["consumed"], r["n_items"])
    bad = np.flatnonzero(r["x"] != r["x_oracle"])
    assert bad.size == 0, [(a[i], v[i], h[i]) for i in bad[:8]]
    assert np.array_equal(r["x"], oracle.retstable_batch(a, v, h, seed=SEED, stream=stream, t=t))
    return r


def test_recipe_builds_where_the_reference_is():
    """A broken recipe must not hide as a skip of the live tests: with the reference's source
    present, the build has to succeed."""
    if not ref.source_present():
        pytest.skip("no reference tree: " + ref.why_unavailable())
    assert ref.available(), ref.why_unavailable()


def test_live_replay_grid(live):
    """57 600 grid draws: every draw consumes its tape exactly, kinds matching, bit-equal."""
    A = [0.05, 0.15, 0.25, 0.35, 0.45, 0.5, 0.75, 0.95]
    H = [0, 1e-8, 1e-4, 1e-2, 0.3, 1, 3, 10, 1e2, 1e4, 1e6, 1e9]
    V = [1, 0.37, 5]
    a, h, v = [np.repeat(np.asarray(g, dtype=np.float64).ravel(), 200)
               for g in np.meshgrid(A, H, V, indexing="ij")]
    assert len(h) == 57600
    r = _replay_all(h, a, v, stream=11, t=2)
    assert r["n_outer"].max() <= mk.MAX_OUTER


def test_live_replay_random(live):
    """20 000 draws, h log-uniform over 1e-12 .. 1e12, alpha uniform in (0.02, 0.98)."""
    rng = np.random.default_rng(77)
    n = 20000
    h = 10.0 ** rng.uniform(-12, 12, n)
    a = rng.uniform(0.02, 0.98, n)
    v = rng.choice([1.0, 0.37, 5.0], n)
    _replay_all(h, a, v, stream=12, t=1)


def test_fixture_regenerates(live, fx):
    cur = mk.arrays()
    assert set(cur) == set(fx) - {"pools"}
    for k, val in cur.items():
        assert np.array_equal(val, fx[k]) and val.dtype == fx[k].dtype, k


def test_shim_reports_a_wrong_tape(live, fx):
    """The tape player: a short tape ends the reference's loops (flag, no hang), an item
    served to another kind of call is flagged, a spare item is flagged, ANY serves both."""
    i = int(np.argmax(fx["A_n_outer"]))
    a, v, h = fx["A_alpha"][i], fx["A_V0"][i], fx["A_h"][i]
    tp = oracle.retstable_tape(h, a, v, SEED, 0, 0, i)
    kind, value = tp["kind"], tp["value"]
    x, used, f = ref.replay(h, a, v, kind, value)
    assert (x, used, f) == (fx["A_x"][i], len(kind), 0)
    _, used, f = ref.replay(h, a, v, kind[:-1], value[:-1])
    assert f & ref.EXHAUSTED and used == len(kind) - 1
    _, _, f = ref.replay(h, a, v, kind[:0], value[:0])
    assert f & ref.EXHAUSTED
    wrong = kind.copy()
    wrong[-1] = oracle.TAPE_NORM if kind[-1] != oracle.TAPE_NORM else oracle.TAPE_EXPON
    _, _, f = ref.replay(h, a, v, wrong, value)
    assert f & ref.KIND_MISMATCH
    _, used, f = ref.replay(h, a, v, np.append(kind, 0), np.append(value, 0.5))
    assert f == ref.LEFTOVER and used == len(kind)
    x, used, f = ref.replay(h, a, v, np.full(len(kind), oracle.TAPE_ANY), value)
    assert (x, used, f) == (fx["A_x"][i], len(kind), 0)
