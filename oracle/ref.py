"""TEST INFRASTRUCTURE ONLY -- the reference's own compiled tilted-stable sampler.

``make ref`` (oracle/Makefile) compiles the reference's ``Code/C/retstable.cpp`` untouched,
with ``ref_shim/RNG.hpp`` standing in for the ``RNG.hpp`` it includes and does not ship, and
``ref_driver.cpp`` around it.  The driver feeds ``retstable_LD`` the oracle's own variates
(``bbo_retstable_tape``: the Philox blocks of the draw's counters in the order the sampler
asks for them) and reports what it returned and whether it consumed exactly that tape.

Only the fixture generator (tests/golden/make_ref_golden.py) and tests/test_ref_pin_cpu.py
import this module; nothing of the product does.  The reference tree is looked for at
``$BB_REFERENCE`` (default ``/root/reference``); where it is absent ``available()`` is
false and the committed fixture tests/golden/ref_retstable.npz carries the pin.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from . import TAPE_ANY, TAPE_EXPON, TAPE_NORM, TAPE_UNIF  # noqa: F401  (tape item kinds)
from . import _key

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_ref", "libbbref.so")
_SOURCE = os.path.join("Code", "C", "retstable.cpp")
_lib = None
_why = None

# flag word of a replayed draw (ref_driver.cpp); 0 = kinds matched, tape consumed exactly
KIND_MISMATCH, EXHAUSTED, LEFTOVER, TAPE_CUT = 1, 2, 4, 8

_dp = ctypes.POINTER(ctypes.c_double)
_lp = ctypes.POINTER(ctypes.c_long)
_ip = ctypes.POINTER(ctypes.c_int)
_u64p = ctypes.POINTER(ctypes.c_uint64)


def reference_dir() -> str:
    return os.environ.get("BB_REFERENCE", "/root/reference")


def _load():
    global _lib, _why
    if _lib is not None or _why is not None:
        return _lib
    ref = reference_dir()
    if not os.path.exists(os.path.join(ref, _SOURCE)):
        _why = f"no reference tree ({os.path.join(ref, _SOURCE)} not found)"
        return None
    r = subprocess.run(["make", "-s", "-C", _HERE, "ref", f"REFERENCE={ref}"],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(_LIB_PATH):
        _why = "building the reference sampler failed: " + (r.stderr.strip()[-400:] or "no output")
        return None
    L = ctypes.CDLL(_LIB_PATH)
    d, lg, u64 = ctypes.c_double, ctypes.c_long, ctypes.c_uint64
    L.bbr_replay.argtypes = [d, d, d, _ip, _dp, lg, _dp, _lp]
    L.bbr_replay.restype = ctypes.c_int
    L.bbr_retstable_batch.argtypes = [lg, _dp, _dp, _dp, _u64p, _u64p, _u64p, _dp, _dp, _lp, _lp,
                                      _lp, _lp, _ip]
    L.bbr_retstable_batch.restype = None
    L.bbr_lambda_batch.argtypes = [lg, _dp, d, d, _u64p, u64, u64, _dp, _dp, _lp, _lp, _ip]
    L.bbr_lambda_batch.restype = None
    _lib = L
    return _lib


def source_present() -> bool:
    """The reference's sampler source is there to be built."""
    return os.path.exists(os.path.join(reference_dir(), _SOURCE))


def available() -> bool:
    """True when the reference tree exists and its sampler builds (built lazily, once)."""
    return _load() is not None


def why_unavailable() -> str:
    _load()
    return _why or ""


def _need():
    L = _load()
    if L is None:
        raise RuntimeError(why_unavailable())
    return L


def _f64(a, num=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if num is None else np.ascontiguousarray(np.broadcast_to(a, (num,)))


def replay(h, alpha, V0, kind, value):
    """``retstable_LD(h, alpha, r, V0)`` on a tape given as (kind, value) arrays.
    Returns (x, items consumed, flag word)."""
    L = _need()
    kind = np.ascontiguousarray(kind, dtype=np.intc)
    value = _f64(value)
    x, used = ctypes.c_double(0.0), ctypes.c_long(0)
    f = L.bbr_replay(float(h), float(alpha), float(V0), kind.ctypes.data_as(_ip),
                     value.ctypes.data_as(_dp), kind.shape[0], ctypes.byref(x), ctypes.byref(used))
    return x.value, used.value, f


def retstable_ref(h, alpha, V0=1.0, seed=0, stream=0, t=0, j=0):
    """The reference's ``retstable_LD`` for draws (h[i], alpha[i], V0[i]) on the oracle's
    variates of counters (t[i], j[i]) under key (seed, stream).  Scalars broadcast.
    Returns dict(x (reference), x_oracle, n_items, consumed, n_outer, n_inner, flags)."""
    L = _need()
    h = _f64(h).reshape(-1)
    num = h.shape[0]
    alpha, V0 = _f64(alpha, num), _f64(V0, num)
    tt = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.uint64), (num,)))
    jj = np.ascontiguousarray(np.broadcast_to(np.asarray(j, dtype=np.uint64), (num,)))
    out = dict(x=np.zeros(num), x_oracle=np.zeros(num), n_items=np.zeros(num, dtype=np.int_),
               consumed=np.zeros(num, dtype=np.int_), n_outer=np.zeros(num, dtype=np.int_),
               n_inner=np.zeros(num, dtype=np.int_), flags=np.zeros(num, dtype=np.intc))
    L.bbr_retstable_batch(num, h.ctypes.data_as(_dp), alpha.ctypes.data_as(_dp),
                          V0.ctypes.data_as(_dp), _key(seed, stream), tt.ctypes.data_as(_u64p),
                          jj.ctypes.data_as(_u64p), out["x"].ctypes.data_as(_dp),
                          out["x_oracle"].ctypes.data_as(_dp), out["n_items"].ctypes.data_as(_lp),
                          out["consumed"].ctypes.data_as(_lp), out["n_outer"].ctypes.data_as(_lp),
                          out["n_inner"].ctypes.data_as(_lp), out["flags"].ctypes.data_as(_ip))
    return out


def lambda_ref(beta, alpha, tau, seed, stream, t, j0=0):
    """lambda | beta, tau as the reference forms it (BridgeRegression.cpp:509) around its
    ``retstable_LD``, coefficient j on counters (t, j0 + j).
    Returns dict(lam (reference), lam_oracle, n_outer, n_inner, flags)."""
    L = _need()
    beta = _f64(beta)
    p = beta.shape[0]
    out = dict(lam=np.zeros(p), lam_oracle=np.zeros(p), n_outer=np.zeros(p, dtype=np.int_),
               n_inner=np.zeros(p, dtype=np.int_), flags=np.zeros(p, dtype=np.intc))
    L.bbr_lambda_batch(p, beta.ctypes.data_as(_dp), float(alpha), float(tau), _key(seed, stream),
                       int(t), int(j0), out["lam"].ctypes.data_as(_dp),
                       out["lam_oracle"].ctypes.data_as(_dp), out["n_outer"].ctypes.data_as(_lp),
                       out["n_inner"].ctypes.data_as(_lp), out["flags"].ctypes.data_as(_ip))
    return out
