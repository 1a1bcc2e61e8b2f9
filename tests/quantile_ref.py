"""A numpy restatement of the quantile sketch's bin scheme (include/bayesbridge.h) and of the
pooled selection, for the tests: the key of a value, the edges of a bin, and what
bb_trace_quantiles / the `_q` summary entries must return for draws the device did not bin."""
import numpy as np

SIGN_BINS = 128 * 256
ZERO_BIN = SIGN_BINS + 1
BINS = 2 * SIGN_BINS + 3
PROBS = [0.0, 0.025, 0.5, 0.975, 1.0]


def from_bits(u):
    return np.atleast_1d(np.asarray(u, dtype=np.uint64)).view(np.float64)


def key(z):
    """The bin index of every z (-1 for NaN)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    b = z.view(np.uint64)
    a = b & np.uint64(0x7FFFFFFFFFFFFFFF)
    neg = (b >> np.uint64(63)).astype(bool)
    e = (a >> np.uint64(52)).astype(np.int64)
    m = ((a >> np.uint64(44)) & np.uint64(0xFF)).astype(np.int64)
    r = (e - 959) * 256 + m
    out = np.where(neg, SIGN_BINS - r, ZERO_BIN + 1 + r)
    out = np.where(e < 959, ZERO_BIN, out)
    out = np.where(e >= 1087, np.where(neg, 0, BINS - 1), out)
    return np.where(a > np.uint64(0x7FF0000000000000), -1, out)


def edges(bins):
    """(lo, hi) of every bin index (NaN for -1)."""
    bins = np.atleast_1d(np.asarray(bins, dtype=np.int64))
    neg = bins < ZERO_BIN
    r = np.clip(np.where(neg, SIGN_BINS - bins, bins - ZERO_BIN - 1), 0, SIGN_BINS - 1)
    u = ((r >> 8) + 959).astype(np.uint64) << np.uint64(52) | (r & 255).astype(np.uint64) << np.uint64(44)
    a, b = from_bits(u), from_bits(u + (np.uint64(1) << np.uint64(44)))
    lo, hi = np.where(neg, -b, a), np.where(neg, -a, b)
    two64, tiny = 2.0 ** 64, 2.0 ** -64
    lo = np.where(bins == ZERO_BIN, -tiny, lo)
    hi = np.where(bins == ZERO_BIN, tiny, hi)
    lo = np.where(bins == 0, -np.inf, np.where(bins == BINS - 1, two64, lo))
    hi = np.where(bins == 0, -two64, np.where(bins == BINS - 1, np.inf, hi))
    bad = bins < 0
    return np.where(bad, np.nan, lo), np.where(bad, np.nan, hi)


def selection(x, probs=PROBS):
    """centre, zlo, zhi, below, inbin, counts of draws x (K, M, Q) pooled over the chains: the
    edges of the bin of the k-th smallest x - c, numpy's counts of the draws in lower bins and in
    that bin, and N, NaN, negative, positive, zero-bin, overflow."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    Q = x.shape[2]
    probs = np.asarray(probs, dtype=np.float64)
    out = {"centre": x[0, 0].copy(), "counts": np.zeros((Q, 6))}
    for name in ("zlo", "zhi", "below", "inbin"):
        out[name] = np.full((Q, probs.size), np.nan)
    for q in range(Q):
        col = x[:, :, q].ravel()
        z = col - out["centre"][q]
        nan = np.isnan(z)
        zs = np.sort(z[~nan])
        b = key(z)
        N = zs.size
        out["counts"][q] = [N, nan.sum(), (col < 0).sum(), (col > 0).sum(),
                            (b == ZERO_BIN).sum(), ((b == 0) | (b == BINS - 1)).sum()]
        for j, pr in enumerate(probs):
            if N == 0:
                continue
            k = int(min(N, max(1, np.ceil(pr * float(N)))))
            bk = int(key(zs[k - 1])[0])
            lo, hi = edges(bk)
            out["zlo"][q, j], out["zhi"][q, j] = lo[0], hi[0]
            out["below"][q, j] = ((b >= 0) & (b < bk)).sum()
            out["inbin"][q, j] = (b == bk).sum()
    return out


def assert_selection_equal(got, want, what=""):
    """Bit for bit: the brackets, the counts and the centre."""
    for name in ("centre", "zlo", "zhi", "below", "inbin", "counts"):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert np.all(same), (what, name, a[~same], b[~same])
