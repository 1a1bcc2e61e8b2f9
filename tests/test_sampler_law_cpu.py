"""The scalar samplers' exact laws at their branch edges, on the CPU (tests/sampler_law.py):
(a) the PIT formulas against 50-digit arithmetic, (b) every verdict and power condition on the
oracle's draws, (c) the verdict against itself on exact-law draws.  tests/test_sampler_law_gpu.py
runs the same cases through the device.  Keys are fixed: every result is deterministic."""
import math

import numpy as np
import pytest

import oracle
from tests import sampler_law as sl

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp

N = 2 ** 18
# PG: the draws times 1.01 move the mean by 0.01 sqrt(N) / cv s.e., cv = sd / mean about 0.82 at
# psi <= 3.125.  At N = 2^18 that is 6.3: a sample whose own z is below -1.3 passes the mean
# check as drawn AND stretched, one stream in ten.  At N = 2^20 it is 12.5 > 5 + 5, so every
# sample that passes as drawn fails stretched.
N_PG = 2 ** 20
CASES = sl.all_cases()
IDS = [f"{fam}-{c.id}" for fam, _, c in CASES]
PIT_TOL = 1e-9


def _mp_cdf(law, x):
    """F(x) of a law in 50-digit arithmetic, from the same doubles."""
    mp.dps = 50
    x = mp.mpf(float(x))
    if isinstance(law, sl.TruncNormal):
        mu, sig = mp.mpf(law.mu), mp.mpf(law.sig)
        r2 = mp.sqrt(2)

        def surv(v):  # of the standard normal at (v - mu) / sig; mpmath keeps the exponent
            return mp.erfc((mp.mpf(v) - mu) / sig / r2) / 2 if math.isfinite(v) else \
                mp.mpf(0 if v > 0 else 1)

        if law.b < 0:  # mirrored: work with the lower tail, which is the small one
            def surv(v):  # noqa: F811
                return mp.erfc(-(mp.mpf(v) - mu) / sig / r2) / 2 if math.isfinite(v) else \
                    mp.mpf(1 if v > 0 else 0)
            return (surv(x) - surv(law.lo)) / (surv(law.hi) - surv(law.lo))
        return (surv(law.lo) - surv(x)) / (surv(law.lo) - surv(law.hi))
    if isinstance(law, sl.TruncExpon):
        r, lo = mp.mpf(law.rate), mp.mpf(law.lo)
        den = mp.expm1(-r * (mp.mpf(law.hi) - lo)) if math.isfinite(law.hi) else mp.mpf(-1)
        return mp.expm1(-r * (x - lo)) / den
    a, r = mp.mpf(law.shape), mp.mpf(law.rate)
    den = mp.gammainc(a, 0, r * mp.mpf(law.hi)) if math.isfinite(law.hi) else mp.gamma(a)
    return mp.gammainc(a, 0, r * x) / den


def _pit_points(law, count=256):
    """Points spread over the support and into both 2^-20 tails."""
    tail = 2.0 ** -np.linspace(30.0, 10.0, count // 8)
    u = np.concatenate([tail, np.linspace(2.0 ** -10, 1.0 - 2.0 ** -10, count - 2 * len(tail)),
                        1.0 - tail])
    return law.ppf(u)


def _mp_density(law):
    """The law's density up to a constant, in multiprecision (exp, log and powers only)."""
    if isinstance(law, sl.TruncNormal):
        mu, sig = mp.mpf(law.mu), mp.mpf(law.sig)
        z0 = (mp.mpf(law.mean) - mu) / sig
        return lambda v: mp.exp(-(((v - mu) / sig) ** 2 - z0 ** 2) / 2)
    if isinstance(law, sl.TruncExpon):
        r, lo = mp.mpf(law.rate), mp.mpf(law.lo)
        return lambda v: mp.exp(-r * (v - lo))
    a, r, m = mp.mpf(law.shape), mp.mpf(law.rate), mp.mpf(law.mean)
    return lambda v: mp.exp((a - 1) * mp.log(v / m) - r * (v - m)) if v > 0 else mp.mpf(0)


def _mp_cdf_by_quadrature(law, xs):
    """F at the ascending points xs as cumulative integrals of the density (Ga(4e6, 1), where
    mpmath's incomplete gamma series does not converge); the support is cut 60 sd from the mean,
    beyond which the mass is below exp(-1000)."""
    f = _mp_density(law)
    edges = [mp.mpf(max(law.lo, law.mean - 60 * law.sd))] + [mp.mpf(float(v)) for v in xs] + \
        [mp.mpf(min(law.hi, law.mean + 60 * law.sd))]
    parts = [mp.quad(f, [edges[i], edges[i + 1]]) for i in range(len(edges) - 1)]
    total = mp.fsum(parts)
    return [mp.fsum(parts[:i + 1]) / total for i in range(len(xs))]


@pytest.mark.parametrize("fam,k,case", CASES, ids=IDS)
def test_pit_matches_50_digit_arithmetic(fam, k, case):
    mp.dps = 50
    x = np.sort(_pit_points(case.law))
    u = case.law.pit(x)
    if isinstance(case.law, sl.Gamma) and case.law.shape > 1e5:
        ref = np.array([float(v) for v in _mp_cdf_by_quadrature(case.law, x)])
    else:
        ref = np.array([float(_mp_cdf(case.law, v)) for v in x])
    err = float(np.max(np.abs(u - ref)))
    print(f"{fam} {case.id}: max |du| = {err:.2e} over u in [{ref.min():.2e}, 1 - "
          f"{1 - ref.max():.2e}]")
    assert ref.min() < 2.0 ** -19 and ref.max() > 1.0 - 2.0 ** -19  # the tails were reached
    assert err <= PIT_TOL


@pytest.mark.parametrize("fam,k,case", CASES, ids=IDS)
def test_mean_matches_quadrature(fam, k, case):
    """The exact mean (the centre of the power condition's stretch) against the ratio of the
    integrals of x f and f, f the density in 30-digit arithmetic: within 1e-6 of the law's sd
    (the mean is a double: half a spacing is up to 2^-21 = 4.8e-7 sd at a case the lattice
    condition keeps).  Infinite supports are cut where the tail mass is below 1e-17."""
    mp.dps = 30
    law = case.law
    f = _mp_density(law)
    lo, hi = law.bracket()
    pts = sorted(set([lo, hi] + [float(v) for v in law.ppf(np.array([0.01, 0.5, 0.99]))]))
    m = mp.mpf(law.mean)  # integrate x - mean: the error is then relative to the sd
    if isinstance(law, sl.Gamma) and law.shape < 1.0:
        # x = t^(1 / shape) takes the singularity of x^(shape - 1) at 0 out of the integrand
        inv, r = 1 / mp.mpf(law.shape), mp.mpf(law.rate)
        pts = [mp.mpf(v) ** mp.mpf(law.shape) for v in pts]
        off = mp.quad(lambda t: (t ** inv - m) * mp.exp(-r * t ** inv), pts) / \
            mp.quad(lambda t: mp.exp(-r * t ** inv), pts)
    else:
        off = mp.quad(lambda v: (v - m) * f(v), pts) / mp.quad(f, pts)
    print(f"{fam} {case.id}: mean {law.mean!r}, error = {float(off) / law.sd:+.2e} sd")
    assert abs(float(off)) <= 1e-6 * law.sd


@pytest.mark.parametrize("fam,k,case", CASES, ids=IDS)
def test_oracle_draws_follow_the_law(fam, k, case):
    x = sl.draw(oracle, case, N, sl.stream(fam, k))
    assert case.law.inside(x)
    sl.judge(f"oracle {fam} {case.id}", case.law, x)


@pytest.mark.parametrize("k,psi", list(enumerate(sl.PG_PSI)), ids=[repr(p) for p in sl.PG_PSI])
def test_oracle_pg_draws_follow_the_law(k, psi):
    x = oracle.pg_batch(np.full(N_PG, psi), sl.SEED, sl.stream("pg", k), 0)
    assert np.all(np.isfinite(x)) and np.all(x > 0)
    sl.pg_judge(f"oracle PG(1, {psi!r})", x, psi)


SELF = {"tnorm": "3_3.6-std", "texpon": "c30", "rtgamma": "a50.0_T10.0_rate1", "gamma": "shape2.5"}


@pytest.mark.parametrize("fam", sorted(SELF))
def test_verdict_passes_exact_law_draws(fam):
    """Draws made by inverting the PIT from numpy uniforms pass the verdict, and fail it
    stretched: the statistics judge the law, not the sampler's algorithm."""
    (case,) = [c for f, _, c in CASES if f == fam and c.id == SELF[fam]]
    u = np.random.default_rng(2024).random(N)
    x = case.law.ppf(u)
    assert float(np.max(np.abs(case.law.pit(x) - u))) <= PIT_TOL
    sl.judge(f"inverse PIT {fam} {case.id}", case.law, x)


def test_pg_verdict_passes_exact_law_draws():
    """PG(1, c) from its definition, sum_k g_k / (2 pi^2 ((k - 1/2)^2 + c^2 / (4 pi^2))) with g_k ~
    Exp(1): 64 terms drawn, the rest (1e-3 of the mean, 2e-7 of the variance) at its
    expectation."""
    c, n, terms = 2.0, N_PG, 64
    rng = np.random.default_rng(7)
    w = 1.0 / (2.0 * math.pi ** 2 * ((np.arange(1, terms + 1) - 0.5) ** 2
                                      + c * c / (4.0 * math.pi ** 2)))
    x = np.zeros(n)
    for lo in range(0, n, 65536):
        x[lo:lo + 65536] = rng.standard_exponential((min(65536, n - lo), terms)) @ w
    x += sl.pg_mean(c) - w.sum()
    sl.pg_judge(f"series PG(1, {c})", x, c)
