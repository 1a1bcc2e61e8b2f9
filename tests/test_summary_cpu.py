"""CPU tests of the summary mode (posterior summaries of chain batches without traces): the
drop-in boundary declares and exports the new entries, and the diagnostics computed from
moments and autocovariances are the ones computed from the traces (shared arithmetic)."""
import numpy as np
import pytest

import bayesbridge_amd as bb
from bayesbridge_amd import diagnostics as dg
from tests.test_abi import declared_functions

NEW_SYMBOLS = ["bridge_reg_stable_chains_summary", "bridge_regression_chains_summary",
               "bb_chains_summary_reset", "bb_chains_summary_add", "bb_chains_summary_get",
               "bb_trace_summary"]


def ar1(phi, n, seed, mean=0.0):
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    x[0] = rng.standard_normal() / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + rng.standard_normal()
    return x + mean


def numpy_summary(x, L):
    """The summary of x (K, M, Q) by direct sums: what the device accumulators return."""
    x = np.asarray(x, dtype=np.float64)
    K, M, Q = x.shape
    xc = x - x.mean(axis=1, keepdims=True)
    acov = np.zeros((K, Q, L + 1))
    for k in range(min(L, M - 1) + 1):
        acov[:, :, k] = (xc[:, k:] * xc[:, :M - k]).sum(axis=1) / M
    n = M // 2
    halves = np.stack([x[:, :n], x[:, M - n:]], axis=-1)  # (K, n, Q, 2)
    return {"nsamp": M, "mean": x.mean(axis=1), "var": x.var(axis=1, ddof=1), "acov": acov,
            "hmean": halves.mean(axis=1), "hvar": halves.var(axis=1, ddof=1)}


def test_new_symbols_are_declared_and_exported():
    names = declared_functions()
    L = bb.library()
    for n in NEW_SYMBOLS:
        assert n in names, n
        assert n in bb.EXPORTED_SYMBOLS, n
        assert hasattr(L, n), n
    assert "bb_summary.hip" in bb._build.SOURCES


def test_effective_size_from_acov_equals_effective_size():
    n = 2000
    cols = [ar1(phi, n, 40 + i) for i, phi in enumerate((0.0, 0.6, 0.95))] + [np.full(n, 3.25)]
    x = np.stack(cols, axis=1)
    L = dg.default_maxlag(n)
    assert L == 33
    want = dg.effective_size(x)
    got = dg.effective_size_from_acov(n, np.stack([dg._acov(x[:, j], L) for j in range(4)]))
    assert got.shape == (4,)
    assert got[3] == 0.0 and want[3] == 0.0  # the constant column
    assert np.all(np.abs(got[:3] - want[:3]) <= 1e-12 * want[:3]), (got, want)
    # batched: leading dimensions are kept
    both = dg.effective_size_from_acov(n, np.stack([dg._acov(x[:, j], L) for j in (1, 2)])[None])
    assert both.shape == (1, 2) and np.array_equal(both[0], got[1:3])


def test_rhat_from_moments_equals_rhat():
    K, M, P = 4, 101, 3  # odd M: the middle draw is dropped
    rng = np.random.default_rng(7)
    x = rng.standard_normal((K, M, P)) + np.arange(K)[:, None, None] * 0.3
    s = numpy_summary(x, 0)
    got = dg.rhat_from_moments(M, s["hmean"], s["hvar"])
    want = dg.rhat(x)
    assert got.shape == (P,)
    assert np.all(np.abs(got - want) <= 1e-12), (got, want)
    one = dg.rhat_from_moments(M, s["hmean"][:, 0], s["hvar"][:, 0])
    assert abs(one - dg.rhat(x[:, :, 0])) <= 1e-12
    with pytest.raises(ValueError):
        dg.rhat_from_moments(3, s["hmean"], s["hvar"])
    with pytest.raises(ValueError):
        dg.rhat_from_moments(M, s["hmean"], s["hvar"][:, :2])


def test_sum_stat_from_summary_equals_sum_stat_chains():
    K, M = 3, 500
    x = np.stack([np.stack([ar1(phi, M, 100 * c + i, mean=mu) for i, (phi, mu) in
                            enumerate(((0.5, 2.0), (0.9, -1.0), (0.0, 50.0)))], axis=1)
                  for c in range(K)])
    x = np.concatenate([x, np.full((K, M, 1), 0.5)], axis=2)  # a known parameter: constant
    want = dg.sum_stat_chains(x[:, :, :3], 2.5)
    s = numpy_summary(x, dg.default_maxlag(M))
    got = dg.sum_stat_from_summary(dict(s, p=3), 2.5)
    assert set(got) == set(want)
    sd = want["sd"]
    assert np.all(np.abs(got["mean"] - want["mean"]) <= 1e-12 * sd)
    assert np.all(np.abs(got["sd"] - sd) <= 1e-12 * sd)
    assert np.all(np.abs(got["ess"] - want["ess"]) <= 1e-9 * want["ess"])
    assert np.all(np.abs(got["rhat"] - want["rhat"]) <= 1e-12)
    assert np.allclose(got["esr"], got["ess"] / 2.5, rtol=1e-15)
    assert got["chains"] == K and got["runtime"] == 2.5
    assert got["ess_summary"] == (got["ess"].min(), np.median(got["ess"]), got["ess"].max())
    # every parameter, the constant one included: zero variance, ESS 0
    full = dg.sum_stat_from_summary(s, 2.5)
    assert full["ess"].shape == (4,) and full["ess"][3] == 0.0 and full["sd"][3] == 0.0


def test_default_maxlag_is_codas_order():
    assert [dg.default_maxlag(n) for n in (1, 2, 5, 120, 100000)] == [0, 1, 4, 20, 50]
    assert bb._summary_maxlag(120, None) == 20 and bb._summary_maxlag(120, 7) == 7
    assert bb._summary_maxlag(10 ** 7, None) == 63


def test_summary_entries_fail_loudly_without_gpu():
    if bb.device_count() > 0:
        pytest.skip("a GPU is visible")
    X = np.random.default_rng(0).standard_normal((20, 3))
    y = X[:, 0]
    with pytest.raises(RuntimeError):
        bb.bridge_reg_stb_chains_summary(y, X, nsamp=10, nchains=2)
    with pytest.raises(RuntimeError):
        bb.bridge_reg_tri_chains_summary(y, X, nsamp=10, nchains=2)
    with pytest.raises(RuntimeError):
        bb.trace_summary(np.zeros((1, 8, 2)), 3)
    with pytest.raises(RuntimeError):
        bb.ChainBatch(bb.EngineConfig(n=20, p=3), 2, X, y)
