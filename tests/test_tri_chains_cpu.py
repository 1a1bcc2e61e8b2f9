"""CPU tests of the triangle-mixture chain batch's interface: the new entry points are
exported unmangled and declared in include/bayesbridge.h, and fail loudly without a GPU."""
import numpy as np
import pytest

import bayesbridge_amd as bb
from tests.test_abi import declared_functions

TRI_CHAIN_SYMBOLS = ["bridge_regression_chains", "bb_chains_get_tri_trace",
                     "bb_chains_set_tri_state", "bb_chains_get_tri_basis", "bb_chains_threads",
                     "bb_chains_set_threads", "bb_compute_units"]


def test_tri_chain_symbols_declared_and_exported():
    L = bb.library()
    declared = declared_functions()
    for name in TRI_CHAIN_SYMBOLS:
        assert name in declared, name
        assert name in bb.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name


def test_bridge_regression_chains_appends_nchains():
    """The 26 arguments of bridge_regression with `const int *nchains` appended."""
    L = bb.library()
    single, chains = L.bridge_regression.argtypes, L.bridge_regression_chains.argtypes
    assert len(single) == 26 and len(chains) == 27
    assert list(chains[:26]) == list(single) and chains[26] is bb._ip


def test_no_gpu_fails_loudly():
    if bb.device_count() > 0:
        return  # with a device the calls run: tests/test_tri_chains_gpu.py
    X = np.random.default_rng(1).standard_normal((20, 3))
    with pytest.raises(RuntimeError):
        bb.bridge_reg_tri_chains(X @ np.ones(3), X, nsamp=5, nchains=2)
    with pytest.raises(RuntimeError):
        bb.ChainBatch(bb.EngineConfig(n=20, p=3, method=4), 2, X, X @ np.ones(3))
