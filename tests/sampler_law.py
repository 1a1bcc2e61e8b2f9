"""Exact laws of the scalar samplers, and the statistics that hold a batch of draws to them.

A helper module (like tests/posterior_law.py, not collected).  Nothing here imports ``oracle`` or
``bayesbridge_amd``: the laws are plain numpy / scipy in fp64 and share no code with what they
judge.  The parity tests say "the device draws what the oracle draws", and both sides restate the
same published algorithms; a test built on this module says "what is drawn follows the law", at
the parameters where the algorithms switch branches.

The samplers and their laws:
    tnorm (bb_tri_body.h)        N(mu, sd^2) on [lo, hi]            TruncNormal
    texpon (bb_tri.hip)          Exp(rate) shifted to [left, right]  TruncExpon
    rtgamma_std (bb_tri.hip)     Ga(shape, rate) on (0, T]           Gamma
    gamma1 (bb_sampler.h)        Ga(shape, 1)                        Gamma
    pg1 (bb_pg.h)                PG(1, psi)                          no closed CDF: pg_checks

Probability integral transform u = F(x), written so that nothing cancels against the
denominator it is divided by:
    truncated normal, a = (lo - mu) / sd > 0, dz = (x - lo) / sd (an exact difference):
        S(a + dz) / S(a) = q(dz) = erfcx((a + dz) / sqrt 2) / erfcx(a / sqrt 2) exp(-dz (2 a + dz) / 2)
        u = expm1(log q(dz)) / expm1(log q(b - a))        (S the normal survival function)
    b < 0: the same through the mirror image, u = 1 - F_mirror(-x);
    a <= 0 <= b: u = (erf(z / sqrt 2) - erf(a / sqrt 2)) / (erf(b / sqrt 2) - erf(a / sqrt 2)), the
        difference of ndtr values with the 1/2 they share removed (ndtr(1e-8) - ndtr(0) itself
        keeps 8 digits); erf(a) <= 0 <= erf(b), so the denominator is a sum of magnitudes and
        the numerator's rounding error is at most 2^-53 of it;
    truncated exponential: u = expm1(-rate (x - left)) / expm1(-rate (right - left));
    gamma laws: u = gammainc(shape, rate x) / gammainc(shape, rate T) (shape >= 1e5:
        gammainc_large).
tests/test_sampler_law_cpu.py holds every case's formula to 1e-9 of 50-digit arithmetic.  Each
law also gives its exact mean, again in a form without cancellation, and ``ppf`` (the PIT
inverted: bisection, or scipy's gammaincinv for the gamma laws).

Verdict on N draws of one case (``judge``), u = F(x):
    K = sqrt N D_N <= 2.5, D_N the two-sided Kolmogorov distance of u from the uniform law.  The
        asymptotic tail 2 exp(-2 2.5^2) is 7.5e-6 per case; the keys are fixed, so a pass is
        deterministic and nothing is retried;
    chi^2 over 64 equiprobable bins of u below the 1 - 1e-6 quantile of chi^2_63 (131.4);
    the counts of u < 2^-10 and of u > 1 - 2^-10 within 6 binomial sd of N 2^-10 each (KS is
        weak in the tails);
    power: the same draws stretched by 1.02 about the law's exact mean (what leaves the support
        takes u = 0 or 1) must FAIL the KS bound.  A case that cannot fail this way is not a case.
PG(1, c) (``pg_judge``): the exact mean tanh(c / 2) / (2 c), the exact variance and the Laplace
transform cosh(c / 2) / cosh(sqrt((c^2 / 2 + s) / 2)) at s = 0.5, 2, 10, 50, each |z| <= 5 with
the s.e. taken from the sample; power: the draws times 1.01 fail the mean check.

Two conditions keep the tests honest.  Doubles are a lattice: a case is kept only if the spacing
of doubles at the law's mean is at most 2^-20 of the law's sd (``resolved``; beyond a of about
1e5, or at mu = 1e6 with a narrow interval, D_N would measure the lattice, which is no sampler
error).  And draws on the same counters share their uniforms, so every case has its own stream
(``stream``).
"""
import math
from collections import namedtuple

import numpy as np
from scipy import special, stats

K_MAX = 2.5
CHI2_BINS = 64
CHI2_MAX = float(stats.chi2.isf(1e-6, CHI2_BINS - 1))
TAIL_P = 2.0 ** -10
TAIL_SD = 6.0
STRETCH = 1.02
LATTICE = 2.0 ** -20
PG_Z = 5.0
PG_STRETCH = 1.01
PG_S = (0.5, 2.0, 10.0, 50.0)
SEED = 0x5A3B1E
SQRT2 = math.sqrt(2.0)
SQRT_2PI_LITERAL = 2.5066282746310002  # the switch of tnorm as bb_tri_body.h writes it


# ---------------------------------------------------------------------------------------
# the laws
# ---------------------------------------------------------------------------------------
class Law:
    """lo <= x <= hi the support; pit(x) = F(x) (0 below, 1 above the support); mean exact."""

    def ppf(self, u):
        """F^-1 by bisection on pit between the ends of ``bracket()``."""
        u = np.asarray(u, dtype=np.float64)
        lo, hi = self.bracket()
        lo, hi = np.full(u.shape, lo), np.full(u.shape, hi)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if np.all((mid <= lo) | (mid >= hi)):
                break
            below = self.pit(mid) < u
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        return 0.5 * (lo + hi)

    @property
    def sd(self):
        """The law's sd to a few per cent (the midpoint rule over 4096 quantiles): what the
        lattice condition compares the spacing of doubles with."""
        if getattr(self, "_sd", None) is None:
            q = self.ppf((np.arange(4096) + 0.5) / 4096.0)
            self._sd = float(np.sqrt(np.mean((q - self.mean) ** 2)))
        return self._sd

    def resolved(self):
        return float(np.spacing(abs(self.mean))) <= LATTICE * self.sd

    def inside(self, x):
        return bool(np.all((x >= self.lo) & (x <= self.hi)))


def _log_q(dz, a):
    """log of S(a + dz) / S(a), a > 0, dz >= 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lq = np.log(special.erfcx((a + dz) / SQRT2)) - math.log(special.erfcx(a / SQRT2)) \
            - 0.5 * dz * (2.0 * a + dz)
    return np.where(np.isinf(dz), -np.inf, lq)


def _pit_pos(dz, a, w):
    """F of the standard normal on [a, a + w], a > 0, at a + dz."""
    den = -np.expm1(_log_q(np.float64(w), a))
    return -np.expm1(_log_q(np.clip(dz, 0.0, w), a)) / den


def _mean_pos(a, w):
    """E z - a of the standard normal on [a, a + w], a > 0:
    sqrt(2 / pi) (1 - e) / (erfcx(a') - erfcx(b') e) - a, e = exp(-w (2 a + w) / 2)."""
    e = 0.0 if math.isinf(w) else math.exp(-0.5 * w * (2.0 * a + w))
    eb = 0.0 if math.isinf(w) else special.erfcx((a + w) / SQRT2) * e
    return math.sqrt(2.0 / math.pi) * (1.0 - e) / (special.erfcx(a / SQRT2) - eb) - a


class TruncNormal(Law):
    """N(mu, sd^2) on [lo, hi], from the doubles the sampler is given."""

    def __init__(self, lo, hi, mu=0.0, sig=1.0):
        self.lo, self.hi, self.mu, self.sig = float(lo), float(hi), float(mu), float(sig)
        self.a, self.b = (self.lo - mu) / sig, (self.hi - mu) / sig
        self.w = (self.hi - self.lo) / sig  # b - a from the exact difference of the bounds
        a, b = self.a, self.b
        assert a < b
        if a > 0.0:
            self.mean = self.lo + sig * _mean_pos(a, self.w)
        elif b < 0.0:
            self.mean = self.hi - sig * _mean_pos(-b, self.w)
        else:
            # phi(a) - phi(b) without cancellation, over Phi(b) - Phi(a)
            s, t = (a, b) if abs(a) <= abs(b) else (b, a)
            d = math.exp(-0.5 * s * s) * -math.expm1(-0.5 * (abs(t) - abs(s)) * (abs(t) + abs(s)))
            d = d if s == a else -d
            den = 0.5 * (special.erf(b / SQRT2) - special.erf(a / SQRT2))
            self.mean = mu + sig * d / math.sqrt(2.0 * math.pi) / den

    def pit(self, x):
        x = np.asarray(x, dtype=np.float64)
        a, b = self.a, self.b
        with np.errstate(invalid="ignore"):
            if a > 0.0:
                u = _pit_pos((x - self.lo) / self.sig, a, self.w)
            elif b < 0.0:
                u = 1.0 - _pit_pos((self.hi - x) / self.sig, -b, self.w)
            else:
                ea, eb = special.erf(a / SQRT2), special.erf(b / SQRT2)
                u = (special.erf((x - self.mu) / self.sig / SQRT2) - ea) / (eb - ea)
        return np.clip(np.where(x < self.lo, 0.0, np.where(x > self.hi, 1.0, u)), 0.0, 1.0)

    def bracket(self):
        a, b, mu, sig = self.a, self.b, self.mu, self.sig
        lo = self.lo if math.isfinite(a) else mu + sig * (min(b, 0.0) - 40.0 / max(-b, 1.0))
        hi = self.hi if math.isfinite(b) else mu + sig * (max(a, 0.0) + 40.0 / max(a, 1.0))
        return lo, hi


class TruncExpon(Law):
    """left + Exp(rate) restricted to [left, right]; c = rate (right - left)."""

    def __init__(self, left, right, rate):
        self.lo, self.hi, self.rate = float(left), float(right), float(rate)
        c = self.c = rate * (self.hi - self.lo)
        if c < 1e-3:  # 1 - c / expm1(c) = c / 2 - c^2 / 12 + c^4 / 720 - ...
            g = c / 2.0 - c * c / 12.0 + c ** 4 / 720.0
        elif c > 700.0:
            g = 1.0 - c * math.exp(-c) if math.isfinite(c) else 1.0
        else:
            g = 1.0 - c / math.expm1(c)
        self.mean = self.lo + g / rate

    def pit(self, x):
        x = np.asarray(x, dtype=np.float64)
        d = np.clip(x - self.lo, 0.0, self.hi - self.lo)
        u = np.expm1(-self.rate * d) / math.expm1(-self.c)
        return np.clip(np.where(x < self.lo, 0.0, np.where(x > self.hi, 1.0, u)), 0.0, 1.0)

    def bracket(self):
        return self.lo, min(self.hi, self.lo + 750.0 / self.rate)


_TEMME_C0 = (-1.0 / 3.0, 1.0 / 12.0, -2.0 / 135.0, 1.0 / 864.0, 1.0 / 2835.0, -139.0 / 777600.0)
_TEMME_C1 = (-1.0 / 540.0, -1.0 / 288.0, 1.0 / 378.0)
LARGE_SHAPE = 1e5


def gammainc_large(a, x):
    """P(a, x) for a >= 1e5 by Temme's uniform expansion (SIAM J. Math. Anal. 10 (1979) 757),
        P = erfc(-eta sqrt(a / 2)) / 2 - exp(-a eta^2 / 2) / sqrt(2 pi a) (c0(eta) + c1(eta) / a),
        eta^2 / 2 = mu - log1p(mu),  mu = (x - a) / a,
    c0 and c1 by their Taylor series at eta = 0 and eta^2 / 2 by the series of mu - log1p(mu)
    (|mu| <= 0.02; scipy's value beyond, where P or 1 - P is below 1e-9).  scipy's gammainc is
    0.5 % low RELATIVELY 4.5 sd below the mean at a = 4e6 (1.6e-8 in u, measured against the
    50-digit series), which the 2^-10 tail count of 2^20 draws would see."""
    x = np.asarray(x, dtype=np.float64)
    mu = (x - a) / a
    near = np.abs(mu) <= 0.02
    m = np.where(near, mu, 0.0)
    h = np.zeros_like(m)  # eta^2 / 2 = m^2 / 2 - m^3 / 3 + m^4 / 4 - ...
    for k in range(12, 1, -1):
        h = (h + (1.0 if k % 2 == 0 else -1.0) / k) * m
    h = h * m
    eta = np.sign(m) * np.sqrt(2.0 * h)
    c0 = np.polyval(_TEMME_C0[::-1], eta)
    c1 = np.polyval(_TEMME_C1[::-1], eta)
    p = 0.5 * special.erfc(-eta * math.sqrt(0.5 * a)) \
        - np.exp(-a * h) / math.sqrt(2.0 * math.pi * a) * (c0 + c1 / a)
    return np.where(near, p, special.gammainc(a, x))


class Gamma(Law):
    """Ga(shape, rate) on (0, T] (T = inf: the whole law)."""

    def __init__(self, shape, T=math.inf, rate=1.0):
        self.shape, self.rate = float(shape), float(rate)
        self.lo, self.hi = 0.0, float(T)
        self.P = (lambda v: gammainc_large(self.shape, v)) if shape >= LARGE_SHAPE else \
            (lambda v: special.gammainc(self.shape, v))
        self.den = 1.0 if math.isinf(T) else float(self.P(rate * T))
        num = 1.0 if math.isinf(T) else float(special.gammainc(shape + 1.0, rate * T))
        self.mean = shape / rate * num / self.den

    def pit(self, x):
        x = np.asarray(x, dtype=np.float64)
        u = self.P(self.rate * np.clip(x, 0.0, self.hi)) / self.den
        return np.clip(np.where(x > self.hi, 1.0, u), 0.0, 1.0)

    def ppf(self, u):
        x = special.gammaincinv(self.shape, np.asarray(u, dtype=np.float64) * self.den)
        return np.minimum(x / self.rate, self.hi)

    def bracket(self):
        if math.isfinite(self.hi):
            return 0.0, self.hi
        return 0.0, float(special.gammainccinv(self.shape, 1e-18)) / self.rate

    def inside(self, x):
        return bool(np.all((x > 0.0) & (x <= self.hi)))


# ---------------------------------------------------------------------------------------
# verdicts
# ---------------------------------------------------------------------------------------
def ks_k(u):
    """sqrt N D_N of u against the uniform law on [0, 1]."""
    u = np.sort(np.asarray(u, dtype=np.float64))
    n = u.shape[0]
    i = np.arange(1, n + 1)
    return math.sqrt(n) * float(max(np.max(i / n - u), np.max(u - (i - 1) / n)))


def verdict(u):
    """The four statistics of section "Verdict": dict(K, chi2, lo, hi), lo / hi the tail counts
    in binomial sd from their expectation."""
    u = np.asarray(u, dtype=np.float64)
    n = u.shape[0]
    counts = np.bincount(np.minimum((u * CHI2_BINS).astype(np.int64), CHI2_BINS - 1),
                         minlength=CHI2_BINS)
    e = n / CHI2_BINS
    sd = math.sqrt(n * TAIL_P * (1.0 - TAIL_P))
    return dict(K=ks_k(u), chi2=float(np.sum((counts - e) ** 2) / e),
                lo=(np.count_nonzero(u < TAIL_P) - n * TAIL_P) / sd,
                hi=(np.count_nonzero(u > 1.0 - TAIL_P) - n * TAIL_P) / sd)


def passes(v):
    return (v["K"] <= K_MAX and v["chi2"] < CHI2_MAX and abs(v["lo"]) <= TAIL_SD
            and abs(v["hi"]) <= TAIL_SD)


def stretched(law, x):
    return law.mean + STRETCH * (np.asarray(x, dtype=np.float64) - law.mean)


def judge(what, law, x):
    """The figures printed, then the verdict on x and the power condition asserted.  Returns
    dict(K, chi2, lo, hi, power)."""
    v = verdict(law.pit(x))
    v["power"] = ks_k(law.pit(stretched(law, x)))
    print(f"{what}: N = {len(x)}, K = {v['K']:.3f}, chi2 = {v['chi2']:.1f}, tails "
          f"{v['lo']:+.2f} / {v['hi']:+.2f} sd, K of the 1.02 stretch = {v['power']:.2f}")
    assert v["K"] <= K_MAX, (what, v)
    assert v["chi2"] < CHI2_MAX, (what, v)
    assert abs(v["lo"]) <= TAIL_SD and abs(v["hi"]) <= TAIL_SD, (what, v)
    assert v["power"] > K_MAX, (what, v)
    return v


def pg_mean(c):
    c = abs(c)
    return 0.25 if c == 0.0 else math.tanh(0.5 * c) / (2.0 * c)


def pg_var(c):
    """(sinh c - c) / (4 c^3 cosh^2(c / 2)) = ((1 - e^2) / 2 - c e) / (c^3 (1 + e)^2), e = exp(-c),
    which does not overflow; 1 / 24 at c = 0."""
    c = abs(c)
    if c < 1e-2:
        return 1.0 / 24.0 - c * c / 60.0
    e = math.exp(-c)
    return (0.5 * (1.0 - e * e) - c * e) / (c ** 3 * (1.0 + e) ** 2)


def _log_cosh(x):
    x = abs(x)
    return x + math.log1p(math.exp(-2.0 * x)) - math.log(2.0)


def pg_laplace(c, s):
    """E exp(-s x), x ~ PG(1, c)."""
    return math.exp(_log_cosh(0.5 * c) - _log_cosh(math.sqrt(0.5 * (0.5 * c * c + s))))


def pg_checks(x, c):
    """{name: z} of the sample mean of x, of (x - E x)^2 and of exp(-s x) against their exact
    values, each s.e. from the sample."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    m = pg_mean(c)
    stats_ = {"mean": (x, m), "var": ((x - m) ** 2, pg_var(c))}
    for s in PG_S:
        stats_[f"laplace_{s:g}"] = (np.exp(-s * x), pg_laplace(c, s))
    return {k: float((y.mean() - t) / (y.std(ddof=1) / math.sqrt(n)))
            for k, (y, t) in stats_.items()}


def pg_judge(what, x, c):
    z = pg_checks(x, c)
    zp = pg_checks(PG_STRETCH * np.asarray(x), c)["mean"]
    print(f"{what}: N = {len(x)}, z " + ", ".join(f"{k} {v:+.2f}" for k, v in z.items())
          + f"; z of the mean of the draws times 1.01 = {zp:+.2f}")
    for k, v in z.items():
        assert abs(v) <= PG_Z, (what, k, v)
    assert abs(zp) > PG_Z, (what, zp)
    z["power"] = abs(zp)
    return z


# ---------------------------------------------------------------------------------------
# the cases (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------
# entry: the batch call ("rtnorm_left", ... of trunc_batch; "rrtgamma"; "gamma"); params: its
# scalar arguments in the call's order, recycled over the N draws; law: what the draws follow.
Case = namedtuple("Case", "id entry params law")


def tn_thr(a):
    """tn_pos's switch between the uniform and the exponential proposal, the header's expression."""
    sq = math.sqrt(a * a + 4.0)
    return a + 2.0 / (a + sq) * math.exp(0.5 + 0.25 * (a * a - a * sq))


INF = math.inf
_THR2 = tn_thr(2.0)
TNORM_STD = [
    (-1.0, 3.0), (0.0, SQRT_2PI_LITERAL), (0.0, float(np.nextafter(SQRT_2PI_LITERAL, 0.0))),
    (-0.3, 0.2), (-1e-3, 1e-3), (0.0, 1e-8), (0.5, 0.9), (3.0, 3.1), (30.0, 30.01),
    (1e4, 1e4 + 5e-5), (0.5, INF), (3.0, INF), (8.0, INF), (37.5, INF), (1e4, INF), (3.0, 3.6),
    (2.0, _THR2 * (1.0 - 2.0 ** -40)), (2.0, _THR2 * (1.0 + 2.0 ** -40)),
]
TNORM_IDS = ["m1_3", "0_sqrt2pi", "0_below_sqrt2pi", "m0.3_0.2", "pm1e-3", "0_1e-8", "0.5_0.9",
             "3_3.1", "30_30.01", "1e4_narrow", "0.5_inf", "3_inf", "8_inf", "37.5_inf",
             "1e4_inf", "3_3.6", "2_thr_below", "2_thr_above"]
TNORM_SCALES = [(0.0, 1.0, "std"), (3.0, 0.1, "mu3_sig0.1"), (1e6, 1.0, "mu1e6")]


def tnorm_cases():
    """Every (a, b) of TNORM_STD, every one-sided or positive one mirrored (one-sided through
    rtnorm with left = -inf, two-sided through rtnorm_both with a < b <= 0), each at every
    (mu, sig) of TNORM_SCALES; the cases the lattice condition refuses are left out."""
    out = []
    for mu, sig, tag in TNORM_SCALES:
        for (a, b), name in zip(TNORM_STD, TNORM_IDS):
            lo, hi = mu + sig * a, mu + sig * b
            if math.isinf(b):
                out.append(Case(f"{name}-{tag}", "rtnorm_left", (lo, mu, sig),
                                TruncNormal(lo, INF, mu, sig)))
            else:
                out.append(Case(f"{name}-{tag}", "rtnorm_both", (lo, hi, mu, sig),
                                TruncNormal(lo, hi, mu, sig)))
            if a < 0.0:
                continue
            lo, hi = mu - sig * b, mu - sig * a
            if math.isinf(b):
                out.append(Case(f"{name}-mirror-{tag}", "rtnorm", (-INF, hi, mu, sig),
                                TruncNormal(-INF, hi, mu, sig)))
            else:
                out.append(Case(f"{name}-mirror-{tag}", "rtnorm_both", (lo, hi, mu, sig),
                                TruncNormal(lo, hi, mu, sig)))
    return [c for c in out if c.law.resolved()]


TEXPON_C = [1e-12, 1e-6, 1e-2, 1.0, 30.0, 700.0, 800.0]


def texpon_cases():
    out = [Case(f"c{c:g}", "rtexpon_rate_both", (0.0, c, 1.0), TruncExpon(0.0, c, 1.0))
           for c in TEXPON_C]
    out.append(Case("left_only", "rtexpon_rate_left", (0.5, 2.0), TruncExpon(0.5, INF, 2.0)))
    out.append(Case("left_only_dotC_rule", "rtexpon_rate", (0.5, INF, 2.0),
                    TruncExpon(0.5, INF, 2.0)))
    for rate in (1e-8, 1.0, 1e8):
        out.append(Case(f"rate{rate:g}_c1", "rtexpon_rate", (0.0, 1.0 / rate, rate),
                        TruncExpon(0.0, 1.0 / rate, rate)))
        out.append(Case(f"rate{rate:g}_left_only", "rtexpon_rate_left", (0.0, rate),
                        TruncExpon(0.0, INF, rate)))
    out.append(Case("left1e6", "rtexpon_rate_left", (1e6, 1.0), TruncExpon(1e6, INF, 1.0)))
    out.append(Case("left1e6_c1", "rtexpon_rate_both", (1e6, 1e6 + 1.0, 1.0),
                    TruncExpon(1e6, 1e6 + 1.0, 1.0)))
    return [c for c in out if c.law.resolved()]


RTGAMMA_AT = [
    (0.5, 0.5), (0.5, 5.0), (1.0, 1.0), (3.0, 3.0), (50.0, 50.0), (2.0, 100.0),  # T >= a
    (0.5, 0.3), (0.2, 1e-3), (1.0, 0.999), (1.0, 1e-6), (0.05, 0.04),            # a <= 1
    (3.0, 0.2), (3.0, 2.0), (50.0, 10.0), (1000.0, 500.0), (1.0 + 1e-7, 1e-8),   # T <= a - 1
    (3.0, 2.5), (50.0, 49.5), (1.5, 0.6), (2000.0, 1999.5),                      # a - 1 < T < a
    (3.0, float(np.nextafter(3.0, 0.0))), (float(np.nextafter(1.0, 2.0)), 0.5),
]


def rtgamma_cases():
    """(shape, T) in standardised units at rate 1, and at rate 4 with right_t = T / 4 (an exact
    quotient, so the regime boundaries T = a, T = a - 1 stay where they are)."""
    out = []
    for rate in (1.0, 4.0):
        for a, T in RTGAMMA_AT:
            out.append(Case(f"a{a!r}_T{T!r}_rate{rate:g}", "rrtgamma", (a, rate, T / rate),
                            Gamma(a, T / rate, rate)))
    return [c for c in out if c.law.resolved()]


GAMMA_SHAPES = [0.05, 0.3, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 2.5, 1e3, 4e6]


def gamma_cases():
    return [Case(f"shape{a!r}", "gamma", (a,), Gamma(a)) for a in GAMMA_SHAPES]


PG_PSI = [0.0, float(np.nextafter(3.125, 0.0)), 3.125, -5.0, 40.0, 700.0]

FAMILIES = {"tnorm": tnorm_cases, "texpon": texpon_cases, "rtgamma": rtgamma_cases,
            "gamma": gamma_cases}


def all_cases():
    """[(family, index in the family, Case)] of the four families with a closed CDF."""
    return [(fam, k, c) for fam, fn in FAMILIES.items() for k, c in enumerate(fn())]


_STREAM0 = {"tnorm": 1000, "texpon": 2000, "rtgamma": 3000, "gamma": 4000, "pg": 9000}


def stream(family, k):
    """The Philox stream of case k of a family: its own, so no two cases share uniforms."""
    return _STREAM0[family] + k


def draw(mod, case, n, stream_):
    """n draws of a case from ``mod`` (``oracle`` or ``bayesbridge_amd``: the same batch calls)."""
    ps = [np.full(n, v) for v in case.params]
    if case.entry == "rrtgamma":
        return mod.rrtgamma_batch(*ps, seed=SEED, stream=stream_)
    if case.entry == "gamma":
        return mod.gamma_batch(ps[0], SEED, stream_, 0)
    return mod.trunc_batch(case.entry, ps, seed=SEED, stream=stream_)
