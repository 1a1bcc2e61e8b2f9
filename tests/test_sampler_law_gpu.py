"""The device's scalar samplers against their exact laws at the branch edges
(tests/sampler_law.py), N = 2^20 draws a case through the batch entry points, and draw by draw
against the oracle on the same counters.  The batch calls raise when a kernel sets an error flag
(rejection cap, empty interval), so a returned batch is a batch without one.  Keys are fixed:
every result is deterministic."""
import numpy as np
import pytest

import oracle
from oracle import gibbs
from tests import sampler_law as sl

pytestmark = pytest.mark.gpu

N = 2 ** 20
CASES = sl.all_cases()
IDS = [f"{fam}-{c.id}" for fam, _, c in CASES]


def same_draws(g, o):
    """The bars of test_truncated_gpu.py: equal NaN / inf patterns, 1e-12 relative elsewhere."""
    assert np.array_equal(np.isnan(g), np.isnan(o))
    assert np.array_equal(np.isinf(g), np.isinf(o)) and np.array_equal(g[np.isinf(o)],
                                                                        o[np.isinf(o)])
    ok = np.isfinite(o)
    assert np.allclose(g[ok], o[ok], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("fam,k,case", CASES, ids=IDS)
def test_device_draws_follow_the_law(gpu_lib, fam, k, case):
    g = sl.draw(gpu_lib, case, N, sl.stream(fam, k))
    assert case.law.inside(g)
    sl.judge(f"device {fam} {case.id}", case.law, g)
    same_draws(g, sl.draw(oracle, case, N, sl.stream(fam, k)))


@pytest.mark.parametrize("k,psi", list(enumerate(sl.PG_PSI)), ids=[repr(p) for p in sl.PG_PSI])
def test_device_pg_draws_follow_the_law(gpu_lib, k, psi):
    """pg_rtigauss switches at |psi| = 3.125 (z = 1 / 0.64): the double below it takes the
    truncated chi-square proposal, 3.125 itself the inverse-Gaussian one."""
    g = gpu_lib.pg_batch(np.full(N, psi), sl.SEED, sl.stream("pg", k), 0)
    assert np.all(np.isfinite(g)) and np.all(g > 0)
    sl.pg_judge(f"device PG(1, {psi!r})", g, psi)
    o = oracle.pg_batch(np.full(N, psi), sl.SEED, sl.stream("pg", k), 0)
    flips = int(np.sum(np.abs(g - o) > 1e-9 * np.maximum(np.abs(o), 1e-300)))
    assert flips == 0
    assert np.max(np.abs(g - o) / o) < 1e-12


S2PI = sl.SQRT_2PI_LITERAL
DOTC = {  # one case per mode of the reference's .C utilities, each through its R-level wrapper
    "rtnorm_left": (lambda bb: bb.rtnorm_left(N, left=3.0), sl.TruncNormal(3.0, sl.INF)),
    "rtnorm_right": (lambda bb: bb.rtnorm_right(N, right=-8.0), sl.TruncNormal(-sl.INF, -8.0)),
    "rtnorm_both": (lambda bb: bb.rtnorm_both(N, left=2.5, right=2.5 + S2PI, mu=2.5, sig=1.0),
                    sl.TruncNormal(2.5, 2.5 + S2PI, 2.5, 1.0)),
    "rtnorm": (lambda bb: bb.rtnorm(N, mu=3.0, sig=0.1, right=2.7),
               sl.TruncNormal(-sl.INF, 2.7, 3.0, 0.1)),
    "rtexp_left": (lambda bb: bb.rtexp_left(N, left=0.5, rate=2.0), sl.TruncExpon(0.5, sl.INF, 2.0)),
    "rtexp_both": (lambda bb: bb.rtexp_both(N, left=0.0, right=800.0, rate=1.0),
                   sl.TruncExpon(0.0, 800.0, 1.0)),
    "rtexp": (lambda bb: bb.rtexp(N, left=0.0, right=1e-12, rate=1.0),
              sl.TruncExpon(0.0, 1e-12, 1.0)),
    "rrtgamma": (lambda bb: bb.rrtgamma(N, shape=3.0, rate=4.0, rtrunc=0.5),
                 sl.Gamma(3.0, 0.5, 4.0)),
}


@pytest.mark.parametrize("name", sorted(DOTC))
def test_dotC_wrappers_follow_the_law(gpu_lib, name):
    """The wrappers draw under the library's call key (set_seed), so the law alone judges
    them; rrtgamma (3, rate 4, 0.5) is regime 3 at its boundary T = a - 1."""
    call, law = DOTC[name]
    gpu_lib.set_seed(20240917 + sorted(DOTC).index(name))
    x = call(gpu_lib)
    assert x is not None and law.resolved() and law.inside(x)
    sl.judge(f".C {name}", law, x)


def test_triangle_chain_draws_what_the_sequential_sampler_draws(gpu_lib):
    """tnorm_par (16 attempts of a truncated-normal draw tested at once) is only reachable inside
    the fused triangle chain, k_tri_chain.  The chain tests already compare it bit for bit with
    the sequential rejection loop (test_tri_chains_gpu.py: test_batch_equals_sequential_calls,
    test_instances_agree_bitwise, test_fallback_equals_sequential_calls), and the loop is tnorm,
    whose law the cases above hold; that comparison is not repeated here.  This test ties the
    two ends together once: the first sweeps of a fused chain against the oracle's sequential
    tnorm on the engine's basis."""
    bb = gpu_lib
    rng = np.random.default_rng(20240917)
    n, p = 60, 10
    X = rng.standard_normal((n, p))
    y = X[:, :3] @ np.array([2.0, -1.5, 1.0]) + rng.standard_normal(n)
    basis = bb.Engine(bb.EngineConfig(n=n, p=p, method=4), X, y).tri_basis()
    bb.set_seed(11)
    g = bb.bridge_reg_tri(y, X, nsamp=4, burn=0, extras=True)
    o = gibbs.bridge_regression_tri(y, X, 4, basis, burn=0, seed=11, stream=0)
    assert np.linalg.norm(g["beta"] - o["beta"]) <= 1e-9 * np.linalg.norm(o["beta"])
