"""CPU tests of the pooled quantile sketch (bb_quantile.hip): the drop-in boundary declares and
exports the new entries, the library's host copy of the bin key and edges (bb_quantile_bin)
agrees bit for bit with the numpy restatement of tests/quantile_ref.py, the key is monotone, and
the point estimates and the probs validation are pure Python."""
import ctypes

import numpy as np
import pytest

import bayesbridge_amd as bb
from bayesbridge_amd import diagnostics as dg
from tests import quantile_ref as qr
from tests.test_abi import declared_functions

NEW_SYMBOLS = ["bridge_reg_stable_chains_summary_q", "bridge_regression_chains_summary_q",
               "bridge_reg_logit_chains_summary_q", "bb_chains_quantiles_reset",
               "bb_chains_quantiles_get", "bb_trace_quantiles", "bb_quantile_bin"]


def lib_bin(z):
    """bb_quantile_bin of every z: bins, lo, hi."""
    L = bb.library()
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    bins, lo, hi = np.zeros(z.size, dtype=np.int64), np.zeros(z.size), np.zeros(z.size)
    b, e0, e1 = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    for i, v in enumerate(z):
        rc = L.bb_quantile_bin(float(v), ctypes.byref(b), ctypes.byref(e0), ctypes.byref(e1))
        assert rc == (-1 if np.isnan(v) else 0)
        bins[i], lo[i], hi[i] = b.value, e0.value, e1.value
    return bins, lo, hi


def edge_values():
    up, dn = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, -np.inf)  # noqa: E731
    t, w = 2.0 ** -64, 2.0 ** 64
    allm = qr.from_bits(np.uint64((1000 << 52) | (0xFF << 44) | 12345))  # hi carries into e
    top = qr.from_bits(np.uint64((1086 << 52) | (0xFF << 44)))           # hi is 2^64
    pos = np.array([0.0, 5e-324, dn(t), t, up(t), dn(w), w, up(w), np.inf, float(allm[0]),
                    float(top[0]), 1.0, dn(1.0), up(1.0), 2.2250738585072014e-308])
    return np.concatenate([pos, -pos, [np.nan]])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))


def test_new_symbols_are_declared_and_exported():
    names = declared_functions()
    L = bb.library()
    for n in NEW_SYMBOLS:
        assert n in names, n
        assert n in bb.EXPORTED_SYMBOLS, n
        assert hasattr(L, n), n
    assert "bb_quantile.hip" in bb._build.SOURCES and "bb_quantile.h" in bb._build.HEADERS
    assert "trace_quantiles" in bb.__all__ and "quantiles_from_bins" in dg.__all__


def test_library_key_equals_restatement():
    rng = np.random.default_rng(5)
    z = np.concatenate([rng.integers(0, 2 ** 64, 40000, dtype=np.uint64).view(np.float64),
                        edge_values()])
    bins, lo, hi = lib_bin(z)
    assert np.array_equal(bins, qr.key(z))
    rlo, rhi = qr.edges(qr.key(z))
    assert same_bits(lo, rlo) and same_bits(hi, rhi)
    ok = ~np.isnan(z)
    assert np.all(bins[ok] >= 0) and np.all(bins[ok] < qr.BINS) and np.all(bins[~ok] == -1)
    assert np.all((lo[ok] <= z[ok]) & (z[ok] <= hi[ok]))  # every bin contains its values


def test_edge_bins():
    t, w = 2.0 ** -64, 2.0 ** 64
    up, dn = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, -np.inf)  # noqa: E731
    want = {0.0: qr.ZERO_BIN, -0.0: qr.ZERO_BIN, 5e-324: qr.ZERO_BIN, dn(t): qr.ZERO_BIN,
            -dn(t): qr.ZERO_BIN, t: qr.ZERO_BIN + 1, -t: qr.SIGN_BINS, up(t): qr.ZERO_BIN + 1,
            dn(w): qr.BINS - 2, -dn(w): 1, w: qr.BINS - 1, -w: 0, np.inf: qr.BINS - 1,
            -np.inf: 0}
    for z, b in want.items():
        got, lo, hi = lib_bin(z)
        assert got[0] == b == qr.key(z)[0], (z, got, b)
    # a key with all eight mantissa bits set: hi carries into the exponent
    z = float(qr.from_bits(np.uint64((1000 << 52) | (0xFF << 44) | 12345))[0])
    _, lo, hi = lib_bin(z)
    assert hi[0] == 2.0 ** (1001 - 1023) and lo[0] == hi[0] * (511.0 / 512.0)
    _, lo, hi = lib_bin(-z)
    assert lo[0] == -(2.0 ** (1001 - 1023)) and hi[0] == lo[0] * (511.0 / 512.0)
    _, lo, hi = lib_bin(dn(w))
    assert hi[0] == w and lo[0] == w * (511.0 / 512.0)
    _, lo, hi = lib_bin([0.0, w, -w])
    assert (lo[0], hi[0]) == (-t, t) and (lo[1], hi[1]) == (w, np.inf)
    assert (lo[2], hi[2]) == (-np.inf, -w)
    # a bracket is at most 2^-8 |z| wide
    z = np.random.default_rng(6).standard_normal(2000) * 10.0 ** np.arange(-10, 10).repeat(100)
    _, lo, hi = lib_bin(z)
    assert np.all(hi - lo <= np.abs(z) * 2.0 ** -8)


def test_key_is_monotone():
    rng = np.random.default_rng(7)
    z = rng.integers(0, 2 ** 64, 200000, dtype=np.uint64).view(np.float64)
    z = np.sort(np.concatenate([z[~np.isnan(z)], edge_values()[:-1]]))
    k = qr.key(z)
    assert np.all(np.diff(k) >= 0) and k[0] == 0 and k[-1] == qr.BINS - 1
    lo, hi = qr.edges(np.arange(qr.BINS))
    assert np.all(lo[1:] == hi[:-1])  # the bins tile the line in index order
    assert np.all(lo < hi)


def test_quantiles_from_bins():
    probs = [0.0, 0.5, 1.0]
    centre = np.array([10.0, -1.0, 3.0])
    counts = np.array([[8, 0, 0, 8, 0, 0], [4, 1, 3, 1, 0, 2], [0, 5, 0, 0, 0, 0]], dtype=float)
    inf, nan = np.inf, np.nan
    zlo = np.array([[-2.0, 1.0, 4.0], [-inf, -0.5, 2.0 ** 64], [nan] * 3])
    zhi = np.array([[-1.0, 2.0, 5.0], [-2.0 ** 64, 0.5, inf], [nan] * 3])
    below = np.array([[0.0, 2.0, 7.0], [0.0, 1.0, 3.0], [nan] * 3])
    inbin = np.array([[2.0, 4.0, 1.0], [1.0, 2.0, 1.0], [nan] * 3])
    out = dg.quantiles_from_bins(probs, centre, zlo, zhi, below, inbin, counts)
    # N = 8: ranks 1, 4, 8; rank 4 is the second of the four draws above two lower ones
    assert np.array_equal(out["quantile"][0], [10 - 2 + 0.25, 10 + 1 + 1.5 / 4, 10 + 4 + 0.5])
    assert np.array_equal(out["quantile_lo"][0], [8.0, 11.0, 14.0])
    assert np.array_equal(out["quantile_hi"][0], [9.0, 12.0, 15.0])
    # overflow bins give their finite edge; rank 2 of N = 4 is the first of two in its bin
    assert np.array_equal(out["quantile"][1], [-1 - 2.0 ** 64, -1 - 0.5 + 0.25, -1 + 2.0 ** 64])
    assert out["quantile_lo"][1, 0] == -inf and out["quantile_hi"][1, 2] == inf
    assert np.all(np.isnan(out["quantile"][2])) and np.all(np.isnan(out["quantile_lo"][2]))
    assert np.array_equal(out["prob_pos"][:2], [1.0, 0.25])
    assert np.array_equal(out["prob_neg"][:2], [0.0, 0.75])
    assert np.isnan(out["prob_pos"][2]) and np.isnan(out["prob_neg"][2])
    lo, hi, est = out["quantile_lo"][:2], out["quantile_hi"][:2], out["quantile"][:2]
    assert np.all((lo <= est) & (est <= hi))


@pytest.mark.parametrize("probs", [[], np.linspace(0, 1, 65), [0.5, 1.5], [-0.1], [np.nan],
                                   [0.2, np.inf]],
                         ids=["empty", "65", "above1", "negative", "nan", "inf"])
def test_probs_are_validated_before_the_gpu(probs):
    X = np.random.default_rng(0).standard_normal((20, 3))
    y = X[:, 0]
    with pytest.raises(ValueError, match="prob"):
        bb.bridge_reg_stb_chains_summary(y, X, nsamp=10, nchains=2, probs=probs)
    with pytest.raises(ValueError, match="prob"):
        bb.bridge_reg_tri_chains_summary(y, X, nsamp=10, nchains=2, probs=probs)
    with pytest.raises(ValueError, match="prob"):
        bb.bridge_reg_logit_chains_summary((y > 0) * 1.0, X, nsamp=10, nchains=2, probs=probs)
    with pytest.raises(ValueError, match="prob"):
        bb.trace_quantiles(np.zeros((1, 8, 2)), probs)


def test_good_probs_pass_validation():
    assert np.array_equal(bb._check_probs([0, 0.5, 1], "t"), [0.0, 0.5, 1.0])
    assert bb._check_probs(0.25, "t").shape == (1,)
    assert bb._check_probs(np.linspace(0, 1, 64), "t").size == 64


def test_quantile_entries_fail_loudly_without_gpu():
    if bb.device_count() > 0:
        pytest.skip("a GPU is visible")
    X = np.random.default_rng(0).standard_normal((20, 3))
    y = X[:, 0]
    with pytest.raises(RuntimeError):
        bb.bridge_reg_stb_chains_summary(y, X, nsamp=10, nchains=2, probs=[0.5])
    with pytest.raises(RuntimeError):
        bb.trace_quantiles(np.zeros((1, 8, 2)), [0.5])
