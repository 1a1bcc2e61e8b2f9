"""Generate tests/golden/ref_retstable.npz from the REFERENCE's own compiled tilted-stable
sampler (oracle/ref.py: its retstable_LD replayed on the oracle's variates).

The file holds data only: the inputs and counters of each draw, the value the reference
returned and the attempts it took.  tests/test_ref_pin_cpu.py requires the oracle to
reproduce it bit for bit, tests/test_ref_pin_gpu.py holds every device path that draws
lambda to it, and where the reference tree is present the CPU test regenerates it.

No draw is dropped: the generator fails if a draw's tape is not consumed exactly with
matching kinds, or takes more than 64 outer attempts, or if an edge the fixture exists for
(listed in ``arrays``) does not occur in it.
Run:  python tests/golden/make_ref_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle  # noqa: E402

SEED = 0xB4E5B41D6E
PATH = os.path.join(HERE, "ref_retstable.npz")
MAX_OUTER = 64

# --- block A: direct draws on key (SEED, stream 0), t = 0, j = index ------------------------
A_ALPHA = [0.05, 0.15, 0.25, 0.45, 0.5, 0.75, 0.95]
A_H = [0.0, 1e-300] + [10.0 ** k for k in range(-8, 13)]
A_V0 = [1.0, 0.37, 5.0]
A_REPS = 4
GAMMA1 = [(0.25, 1.0), (0.5, 0.37), (0.75, 5.0)]  # (alpha, V0) of the cells around gamma = 1
GAMMA1_REPS = 16
# gamma = h^alpha V0 alpha (1 - alpha) = 1 exactly (sqrt(16) V0 / 4 and 4 / 4): the cells
# where `gamma >= 1` and `gamma > 1` part
GAMMA1_EXACT = [(0.5, 1.0, 16.0), (0.5, 4.0, 1.0)]
GAMMA1_EXACT_REPS = 32
# large gamma: U = |N| / sqrt(gamma) is small, the series branches of sinc_MM
SINC = [(0.05, 1.0, 1e130), (0.05, 5.0, 1e140), (0.5, 1.0, 1e8), (0.5, 0.37, 1e10),
        (0.95, 1.0, 1e4), (0.95, 5.0, 1e6)]
SINC_REPS = 32

# --- block B: lambda pools --------------------------------------------------------------------
POOL_LEN = 1100
MAGNITUDES = [0.0, 1e-8, 1e-4, 0.1, 1.0, 10.0, 1e3]
ZEROS = (7, 25)  # exact zeros inside the first 32 (one inside the first 20)
# name: (alpha, tau, beta pool, stream, t, j0, length)
POOLS = {
    "p0": (0.5, 0.7, 0, 0, 3, 0, POOL_LEN),
    "p1": (0.3, 2.0, 1, 1, 4, 0, POOL_LEN),
    "p2": (0.9, 1e-2, 2, 2, 5, 0, POOL_LEN),
    "p0j": (0.5, 0.7, 0, 0, 3, 12345, POOL_LEN),
    # the chains of a batch draw under streams stream0 + c: one short pool per chain
    "c0": (0.5, 0.7, 0, 5, 6, 0, 128),
    "c1": (0.5, 0.7, 1, 6, 6, 0, 128),
    "c2": (0.5, 0.7, 2, 7, 6, 0, 128),
}


def block_a_inputs():
    a, v, h = [], [], []

    def cell(aa, vv, hh, reps):
        a.extend([aa] * reps)
        v.extend([vv] * reps)
        h.extend([hh] * reps)

    for aa in A_ALPHA:
        for hh in A_H:
            for vv in A_V0:
                cell(aa, vv, hh, A_REPS)
    for vv in A_V0:  # alpha = 1 returns V0 and consumes nothing
        for hh in (0.0, 1.0, 1e6):
            cell(1.0, vv, hh, 1)
    for aa, vv in GAMMA1:
        hs = (1.0 / (aa * (1.0 - aa) * vv)) ** (1.0 / aa)
        for f in (1 - 1e-3, 1 - 2.0 ** -40, 1 + 2.0 ** -40, 1 + 1e-3):
            cell(aa, vv, hs * f, GAMMA1_REPS)
    for aa, vv, hh in GAMMA1_EXACT:
        cell(aa, vv, hh, GAMMA1_EXACT_REPS)
    for aa, vv, hh in SINC:
        cell(aa, vv, hh, SINC_REPS)
    return np.array(a), np.array(v), np.array(h)


def beta_pools():
    """Three beta vectors: few-bit mantissas (the file stays small) times mixed magnitudes."""
    rng = np.random.default_rng(20240917)
    out = []
    for _ in range(3):
        mant = rng.integers(32, 64, size=POOL_LEN) / 32.0
        sign = rng.choice([-1.0, 1.0], size=POOL_LEN)
        mag = np.array(MAGNITUDES)[rng.integers(1, len(MAGNITUDES), size=POOL_LEN)]
        mag[:len(MAGNITUDES) - 1] = MAGNITUDES[1:]  # every magnitude inside a prefix of 20
        b = sign * mant * mag
        b[list(ZEROS)] = 0.0
        out.append(b)
    return out


def _check_edges(a, v, h, res):
    """Every edge block A exists for occurs in it (assertions of the generator)."""
    gam = h ** a * v * a * (1 - a)
    n_small = n_mid = n_big = 0
    outer_kinds = set()
    norm_side = {}
    for i in range(len(h)):
        if a[i] == 1.0:
            assert res["n_items"][i] == 0 and res["x"][i] == v[i], i
            continue
        tp = oracle.retstable_tape(h[i], a[i], v[i], SEED, 0, 0, i)
        assert tp["n_outer"] == res["n_outer"][i] and len(tp["kind"]) == res["n_items"][i], i
        outer_kinds.add(int(tp["kind"][-1]))
        # the accepted inner attempt (V, W_, W): the three items before the last outer
        # block's two
        k_w = len(tp["kind"]) - 4
        pos, saw_norm = 0, False
        for o, ni in enumerate(tp["inner"]):
            for _ in range(ni):
                saw_norm |= tp["kind"][pos + 1] == oracle.TAPE_NORM
                pos += 3
            pos += 2
        assert pos == len(tp["kind"]), i
        norm_side[(a[i], v[i], h[i])] = norm_side.get((a[i], v[i], h[i]), False) or saw_norm
        if tp["kind"][k_w] == oracle.TAPE_NORM:
            ax = a[i] * abs(tp["value"][k_w]) / np.sqrt(gam[i])  # alpha U of the accepted U
            n_small += ax < 2e-4
            n_mid += 2e-4 <= ax < 0.006
            n_big += ax >= 0.006
    assert n_small > 0 and n_mid > 0 and n_big > 0, (n_small, n_mid, n_big)
    assert outer_kinds == {oracle.TAPE_UNIF, oracle.TAPE_NORM, oracle.TAPE_EXPON}, outer_kinds
    assert res["n_outer"].max() >= 5, res["n_outer"].max()
    # both sides of `gamma >= 1`: a normal W_ is asked for on the >= side only
    for aa, vv in GAMMA1:
        hs = (1.0 / (aa * (1.0 - aa) * vv)) ** (1.0 / aa)
        for f in (1 - 1e-3, 1 - 2.0 ** -40):
            assert (hs * f) ** aa * vv * aa * (1 - aa) < 1 and not norm_side[(aa, vv, hs * f)]
        for f in (1 + 2.0 ** -40, 1 + 1e-3):
            assert (hs * f) ** aa * vv * aa * (1 - aa) > 1 and norm_side[(aa, vv, hs * f)]
    for aa, vv, hh in GAMMA1_EXACT:
        assert hh ** aa * vv * aa * (1 - aa) == 1.0 and norm_side[(aa, vv, hh)]
    return dict(n_small=int(n_small), n_mid=int(n_mid), n_big=int(n_big))


def _clean(flags, n_outer, what):
    assert not np.any(flags), f"{what}: tape flags {np.unique(flags)} (0 = consumed exactly)"
    assert n_outer.max() <= MAX_OUTER, f"{what}: {n_outer.max()} outer attempts"


def arrays(report=None):
    from oracle import ref

    out = {}
    a, v, h = block_a_inputs()
    res = ref.retstable_ref(h, a, v, seed=SEED, stream=0, t=0, j=np.arange(len(h)))
    _clean(res["flags"], res["n_outer"], "block A")
    assert np.array_equal(res["consumed"], res["n_items"])
    edges = _check_edges(a, v, h, res)
    out["A_alpha"], out["A_V0"], out["A_h"] = a, v, h
    out["A_x"] = res["x"]
    out["A_n_outer"] = res["n_outer"].astype(np.int16)
    out["A_n_inner"] = res["n_inner"].astype(np.int32)
    betas = beta_pools()
    for k, b in enumerate(betas):
        out[f"B_beta{k}"] = b
    names, meta = [], []
    for name, (alpha, tau, bk, stream, t, j0, length) in POOLS.items():
        r = ref.lambda_ref(betas[bk][:length], alpha, tau, SEED, stream, t, j0=j0)
        _clean(r["flags"], r["n_outer"], "pool " + name)
        out[f"B_{name}_lambda"] = r["lam"]
        out[f"B_{name}_n_outer"] = r["n_outer"].astype(np.int16)
        out[f"B_{name}_n_inner"] = r["n_inner"].astype(np.int32)
        names.append(name)
        meta.append([alpha, tau, bk, stream, t, j0, length])
    out["B_names"] = np.array(names)
    out["B_meta"] = np.array(meta, dtype=np.float64)  # alpha, tau, beta pool, stream, t, j0, len
    out["seed"] = np.array([SEED], dtype=np.uint64)
    if report is not None:
        report.update(edges, draws_a=len(h), max_outer_a=int(res["n_outer"].max()),
                      draws_b=int(sum(m[-1] for m in meta)),
                      max_outer_b=int(max(out[f"B_{n}_n_outer"].max() for n in names)))
    return out


def load(path=PATH):
    """The committed fixture as a dict, with ``pools``: name -> dict(alpha, tau, beta, stream,
    t, j0, lam, n_outer, n_inner)."""
    z = np.load(path)
    d = {k: z[k] for k in z.files}
    pools = {}
    for name, m in zip(d["B_names"], d["B_meta"]):
        name = str(name)
        length = int(m[6])
        pools[name] = dict(alpha=float(m[0]), tau=float(m[1]),
                           beta=d[f"B_beta{int(m[2])}"][:length], stream=int(m[3]), t=int(m[4]),
                           j0=int(m[5]), lam=d[f"B_{name}_lambda"],
                           n_outer=d[f"B_{name}_n_outer"], n_inner=d[f"B_{name}_n_inner"])
    d["pools"] = pools
    return d


if __name__ == "__main__":
    rep = {}
    np.savez_compressed(PATH, **arrays(rep))
    print("wrote", PATH, os.path.getsize(PATH), "bytes", rep)
