"""CPU tests of the logistic chain batch's boundary: the two .C entries are exported and
declared, bb_chains_create's shape rules for method 6 each refuse with their own message, and
the entries' argument checks return before a key is taken or an output is written.  No compute
call: there is no GPU here (the accepted shape fails later, for want of a device)."""
import ctypes

import numpy as np

import bayesbridge_amd as bb
from tests.test_abi import declared_functions

ENTRIES = ("bridge_reg_logit_chains", "bridge_reg_logit_chains_summary")
SHAPE_REFUSALS = ("a logistic chain batch needs p <= 32", "a logistic chain batch needs p <= n",
                  "a logistic chain batch needs n <= 4096")
MAX_N = 4096  # kLogitChainMaxN (bb_kernels.h)


def create_error(n, p, **kw):
    """bb_last_error after bb_chains_create of an n x p logistic design (None: created)."""
    L = bb.library()
    rng = np.random.default_rng(1)
    X = np.asfortranarray(rng.standard_normal((n, p)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    c = bb.EngineConfig(n=n, p=p, method=6, **kw).to_c()
    h = ctypes.c_void_p()
    rc = L.bb_chains_create(ctypes.byref(c), 2, bb._p(X), bb._p(y), ctypes.byref(h))
    if rc == 0:
        L.bb_chains_destroy(h)
        return None
    assert not h.value
    return L.bb_last_error().decode()


def test_entries_are_exported_and_declared():
    L = bb.library()
    names = declared_functions()
    for n in ENTRIES + ("bb_chains_get_omega",):
        assert hasattr(L, n), n
        assert n in names, n
        assert n in bb.EXPORTED_SYMBOLS, n


def test_shape_refusals_have_their_own_messages():
    msgs = [create_error(40, 33), create_error(8, 9), create_error(MAX_N + 1, 4)]
    for got, want in zip(msgs, SHAPE_REFUSALS):
        assert got is not None and want in got, (got, want)
    assert len(set(msgs)) == 3


def test_accepted_shape_is_not_refused_for_its_shape():
    """p = 32, n = 40 passes the batch rules of chain_plan (alpha known or unknown); without a device the
    creation fails later, with another message."""
    for kw in ({}, dict(true_alpha=0.0)):
        msg = create_error(40, 32, **kw)
        if bb.device_count() >= 1:
            assert msg is None, msg
        else:
            assert msg is not None
            assert not any(r in msg for r in SHAPE_REFUSALS), msg
            assert "chain batch needs" not in msg and "chain batch runs" not in msg, msg


def call_entry(name, y, X, M, K):
    """The .C entry on sentinel-filled outputs; returns the outputs."""
    L = bb.library()
    n, p = X.shape
    d = lambda v: ctypes.byref(ctypes.c_double(float(v)))  # noqa: E731
    i = lambda v: ctypes.byref(ctypes.c_int(int(v)))  # noqa: E731
    rt = ctypes.c_double(-7.0)
    k = max(K, 1)
    tail = [bb._p(y), bb._p(X), d(2.0), d(2.0), d(1.0), d(1.0), d(0.0), d(0.5), i(p), i(n), i(M),
            i(3), ctypes.byref(rt), i(K)]
    if name.endswith("_summary"):
        outs = [np.full(k * (p + 3) * s, -7.0) for s in (1, 1, 4, 2, 2)]
        flags = np.full(k, -7, dtype=np.int32)
        getattr(L, name)(*[bb._p(o) for o in outs], flags.ctypes.data_as(bb._ip), i(3), *tail)
        outs.append(flags.astype(np.float64))
    else:
        outs = [np.full(k * M * p, -7.0), np.full(k * M * p, -7.0), np.full(k * M, -7.0),
                np.full(k * M, -7.0)]
        getattr(L, name)(*[bb._p(o) for o in outs], *tail)
    return outs + [np.array([rt.value])]


def test_argument_checks_leave_outputs_and_stream_untouched():
    rng = np.random.default_rng(2)
    X = np.asfortranarray(rng.standard_normal((12, 3)))
    y = (rng.random(12) < 0.5).astype(np.float64)
    ybad = y.copy()
    ybad[5] = 0.5
    for name in ENTRIES:
        for yy, K, word in ((y, 0, "nchains"), (ybad, 2, "{0, 1}")):
            bb.set_rng_state(77, 5)
            outs = call_entry(name, yy, X, 6, K)
            assert bb.get_rng_state() == (77, 5), (name, word)
            for o in outs:
                assert np.all(o == -7.0), (name, word)
            msg = bb.library().bb_last_error().decode()
            assert name in msg and word in msg, msg
