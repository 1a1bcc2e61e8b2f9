"""CPU tests of the multi-chain interface: the exported symbols, the chain diagnostics
(split R-hat, pooled summaries) and the no-GPU behaviour of the new entry point."""
import numpy as np
import pytest

import bayesbridge_amd as bb
from bayesbridge_amd import diagnostics as dg
from tests.test_abi import declared_functions

CHAIN_SYMBOLS = ["bridge_reg_stable_chains", "bb_chains_create", "bb_chains_destroy",
                 "bb_chains_count", "bb_chains_resident_per_cu", "bb_chains_init_state",
                 "bb_chains_run", "bb_chains_sync", "bb_chains_get_trace",
                 "bb_chains_get_state", "bb_chains_set_state", "bb_chains_error_flags"]


def test_chain_symbols_declared_and_exported():
    L = bb.library()
    declared = declared_functions()
    for name in CHAIN_SYMBOLS:
        assert name in declared, name
        assert name in bb.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name


def closed_form(x):
    """Split R-hat from its definition, sequence by sequence."""
    K, M = x.shape
    n = M // 2
    seqs = [x[c, :n] for c in range(K)] + [x[c, M - n:] for c in range(K)]
    W = np.mean([s.var(ddof=1) for s in seqs])
    B = n * np.var([s.mean() for s in seqs], ddof=1)
    return np.sqrt(((n - 1) / n * W + B / n) / W)


def test_rhat_identical_chains_with_equal_halves():
    half = np.array([0.3, -1.2, 2.5, 0.7, -0.4, 1.1])
    x = np.tile(np.r_[half, half], (4, 1))
    n = half.size
    assert dg.rhat(x) == np.sqrt((n - 1) / n)


def test_rhat_shifted_chains_match_closed_form():
    rng = np.random.default_rng(5)
    base = rng.standard_normal(40)
    x = np.stack([base + c * 0.75 for c in range(3)])
    got = dg.rhat(x)
    assert got > 1.0
    assert abs(got - closed_form(x)) <= 4 * np.finfo(float).eps * got
    # W is the variance of the halves of `base`, B that of the shifted half means
    n = 20
    halves = [base[:n], base[n:]]
    W = np.mean([h.var(ddof=1) for h in halves])
    means = [h.mean() + c * 0.75 for c in range(3) for h in halves]
    B = n * np.var(means, ddof=1)
    assert abs(got - np.sqrt(((n - 1) / n * W + B / n) / W)) < 1e-12


def test_rhat_odd_length_drops_the_middle_draw():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 21))
    y = x.copy()
    y[:, 10] = 1e6  # the middle draw of an odd-length chain is not used
    assert dg.rhat(x) == dg.rhat(y)
    assert dg.rhat(x) == dg.rhat(np.delete(x, 10, axis=1))


def test_rhat_reduces_per_coefficient():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((4, 50, 3))
    x[:, :, 1] += np.arange(4)[:, None]
    r = dg.rhat(x)
    assert r.shape == (3,)
    for j in range(3):
        # a strided and a contiguous trace are summed in different orders: a few ulps
        assert abs(r[j] - dg.rhat(np.ascontiguousarray(x[:, :, j]))) <= 1e-14 * r[j]
    assert r[1] > 1.5 > r[0]
    with pytest.raises(ValueError):
        dg.rhat(np.zeros(10))


def test_rhat_of_iid_normals_is_one():
    x = np.random.default_rng(20240501).standard_normal((8, 2000))
    assert 0.99 <= dg.rhat(x) <= 1.02


def test_sum_stat_chains_single_chain_matches_sum_stat():
    rng = np.random.default_rng(8)
    e = rng.standard_normal((600, 4))
    beta = np.zeros_like(e)
    for t in range(1, 600):  # AR(1) traces
        beta[t] = 0.6 * beta[t - 1] + e[t]
    one = dg.sum_stat(beta, 2.0)
    many = dg.sum_stat_chains(beta[None], 2.0)
    assert np.array_equal(many["ess"], one["ess"]) and np.array_equal(many["esr"], one["esr"])
    assert many["ess_summary"] == one["ess_summary"] and many["chains"] == 1
    assert np.allclose(many["mean"], beta.mean(axis=0), rtol=0, atol=1e-15)
    assert np.allclose(many["sd"], beta.std(axis=0, ddof=1), rtol=1e-15)
    assert many["rhat"].shape == (4,)
    two = dg.sum_stat_chains(np.stack([beta, beta[::-1]]), 2.0)
    assert np.allclose(two["ess"], one["ess"] + dg.effective_size(beta[::-1]), rtol=1e-15)


def test_no_gpu_fails_loudly():
    if bb.device_count() > 0:
        return  # with a device the calls run: tests/test_chains_gpu.py
    X = np.random.default_rng(1).standard_normal((20, 3))
    with pytest.raises(RuntimeError):
        bb.bridge_reg_stb_chains(X @ np.ones(3), X, nsamp=5, nchains=2)
    with pytest.raises(RuntimeError):
        bb.ChainBatch(bb.EngineConfig(n=20, p=3), 2, X, X @ np.ones(3))
