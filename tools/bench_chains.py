"""Aggregate rate of K independent small-design chains in one launch (bridge_reg_stb_chains,
bb_small.hip k_small_chains) against one chain at a time.

Designs: C1 (bench.py's n=100, p=20 synthetic design) and a diabetes-shaped 442 x 10 synthetic
design.  For K in {1, 8, 64, CUs, 2 CUs, 4 CUs}: burn-in 500, 5000 samples, the post-burn
runtime the call reports (it includes copying the traces out), aggregate sweeps/s = K nsamp /
runtime, per-chain sweeps/s, and the resident workgroups per CU the runtime reports.  The
kernel-only rate (ChainBatch.run without traces) separates the sweeps from the copy-out.
K = 2 CUs and 4 CUs are measured a second time with bb_set_tuning key 21 (the 256-thread
instance, two chains per CU) into the record's "chains_two_per_cu".

--method tri measures the triangle mixture instead (bridge_reg_tri_chains, bb_tri.hip
k_tri_chains) into profiles/chains_tri_{c1,db}.json.  Its instances all give the same bits, so
there is no tuning key: the record's "instances" holds the kernel-only rate of every instance
(ChainBatch.set_threads) at K = CUs, 2 CUs and 4 CUs, alternated within each round.

--summary measures the summary mode (bridge_reg_*_chains_summary: each ring fill reduced on the
device by bb_summary.hip k_trace_summary, nothing but the summaries copied) against the trace
call of the same build at K = CUs and 4 CUs into profiles/chains_summary_{c1,db}.json
(chains_summary_tri_* with --method tri): per K, alternated within each round, the summary
call, the trace call, the kernel-only rate, and the share of the summary call's runtime that
k_trace_summary takes (timed alone on a full ring of a ChainBatch, scaled to the call).

--summary --quantiles measures the summary call with pooled quantiles (probs = 0.025, 0.5,
0.975: the sketch of bb_quantile.hip built behind the sweeps) against the summary call without
them and the trace call of the same build, alternated within each round at K = CUs and 4 CUs,
into profiles/chains_summary_quantiles_{c1,db}.json, with the time k_trace_hist takes for the
call's samples (a full ring added with the sketch enabled less the same add without it) and
its share of the call.

--alpha measures alpha unknown (alpha = 0, sampled by MH) with the fused kernels sampling it
(bb_set_tuning key 26, bb_small_mh.hip) at K = 1, 256 and 1024 into
profiles/chains_alpha_{c1,db}.json: alternated within each round, the single call with the key
on (k_small_chain_mh) and off (the general path), and per K the key-on batch and this tree's
known-alpha batch, each as the call and kernel only.  The baseline a batch has to beat is
bridge_reg_stb_chains(alpha = 0) without the key, K sequential general-path chains:
--alpha --mode single [--tree DIR] measures it (on the parent checkout, say; fewer samples keep
K = 1024 sequential chains affordable) as one JSON line, which --baseline FILE merges.
--alpha --method tri is the same for the triangle mixture under key 27 (bb_tri_mh.hip:
k_tri_chain_mh, k_tri_chains_mh against k_tri_chains) into profiles/chains_tri_alpha_{c1,db}.json,
with the threads of the instance each K ran.

--wide measures the wide fused chains (bb_set_tuning key 25, bb_wide.hip) at the published
protocol's wider shapes, synthetic designs dbi (442 x 64) and bhi (506 x 103), into
profiles/chains_wide_{dbi,bhi}.json: alternated within each round, the single call with the key
off (the general path: K sequential such calls are the baseline a batch has to beat), the
single call with the key on (k_wide_chain), and batches at K = 8, CUs and 2 CUs with the
kernel-only rate and the resident workgroups per CU.  Default 1000 samples after a burn-in of
200 (the traces of 2 CUs chains of 5000 samples would be 4 GB).

--logit measures the logistic chain batch (bridge_reg_logit_chains, bb_logit_chain.hip
k_logit_chains) at lg5 (the 200 x 5 design of the logistic posterior-law tests) and lg32
(1000 x 32, the same generator) into profiles/chains_logit_{lg5,lg32}.json: alternated within
each round, the single bridge_reg_logit call (the general path) and batches at K = 1, CUs and
4 CUs, each as the call, kernel only and as the summary call, with the resident workgroups per
CU, and one CPU core running the compiled oracle chain (oracle.cpu_logit_chain).  The baseline a
batch has to beat is K sequential general-path chains: --logit --mode single [--tree DIR]
measures the single call (on the parent checkout, say) as one JSON line, which --baseline FILE
merges.  Default 1000 samples after a burn-in of 200.

Protocol: one warm-up call, then REPS rounds, each round visiting every K (and the
single-chain bridge_reg_stb call) once, so slow drifts of the device hit every K alike; the
median over rounds is reported with the min and max beside it.

  python tools/bench_chains.py                 # both designs -> profiles/chains_{c1,db}.json
  python tools/bench_chains.py --mode single --tree DIR   # bridge_reg_stb alone, from the
                                                          # checkout at DIR (A/B with a parent)
  python tools/bench_chains.py --method tri [--mode single --tree DIR]
  python tools/bench_chains.py --summary [--method tri] [--designs c1]
  python tools/bench_chains.py --summary --quantiles [--designs c1]
  python tools/bench_chains.py --wide [--designs dbi]
  python tools/bench_chains.py --alpha --mode single --tree DIR --nsamp 100 --burn 50 > FILE
  python tools/bench_chains.py --alpha --baseline FILE
  python tools/bench_chains.py --alpha --method tri [--mode single --tree DIR | --baseline FILE]
  python tools/bench_chains.py --logit --mode single --tree DIR > FILE
  python tools/bench_chains.py --logit --baseline FILE
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xB4E5B41D6E
CPU_CORE_C1 = 60323.0  # compiled reference-literal chain, one core (profiles/r06_bench_c1.json)


def designs():
    sys.path.insert(0, ROOT)
    import bench

    out = {"c1": (bench.make_columns(100, 0, 20), bench.make_problem_y(100, 20)[0])}
    rng = np.random.default_rng(20240501)
    X = rng.standard_normal((442, 10))
    X -= X.mean(axis=0)
    b = np.r_[3.0, -2.0, 1.5, -1.0, 2.5, np.zeros(5)]
    y = X @ b + 2.0 * rng.standard_normal(442)
    out["db"] = (np.asfortranarray(X), y - y.mean())
    # the shapes of the protocol's designs with interactions (diabetes 442 x 64, Boston 506 x
    # 103), synthetic like db: ten / thirteen main effects' worth of signal
    for name, n, p, seed in (("dbi", 442, 64, 20240502), ("bhi", 506, 103, 20240503)):
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, p))
        X -= X.mean(axis=0)
        b = np.r_[3.0, -2.0, 1.5, -1.0, 2.5, np.zeros(p - 5)]
        y = X @ b + 2.0 * rng.standard_normal(n)
        out[name] = (np.asfortranarray(X), y - y.mean())
    return out


def logit_problem(n, p, seed, scale=1.0):
    """The generator of the logistic tests (tests/test_logit_gpu.py), copied: tools do not
    import tests."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) * scale
    b = np.zeros(p)
    k = max(3, p // 20)
    b[:k] = rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ b))).astype(np.float64)
    return np.asfortranarray(X), y


def logit_designs():
    return {"lg5": logit_problem(200, 5, seed=3), "lg32": logit_problem(1000, 32, seed=3)}


class Method:
    """The entry points of one sampler: stable mixture or triangle mixture."""

    def __init__(self, bb, name):
        self.bb, self.tri = bb, name == "tri"

    def single(self, y, X, **kw):
        if self.tri:
            return self.bb.bridge_reg_tri(y, X, extras=True, **kw)
        return self.bb.bridge_reg_stb(y, X, **kw)

    def chains(self, y, X, **kw):
        return (self.bb.bridge_reg_tri_chains if self.tri
                else self.bb.bridge_reg_stb_chains)(y, X, **kw)

    def summary(self, y, X, **kw):
        return (self.bb.bridge_reg_tri_chains_summary if self.tri
                else self.bb.bridge_reg_stb_chains_summary)(y, X, **kw)

    def config(self, n, p, cap=1, true_alpha=0.5):
        return self.bb.EngineConfig(n=n, p=p, trace_capacity=cap, seed=SEED,
                                    method=4 if self.tri else 0, true_alpha=true_alpha)


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1])}


def kernel_rate(me, X, y, K, nsamp, threads=0, block=50, true_alpha=0.5, ran=None):
    """Sweeps/s of the batch kernel alone: blocks of `block` sweeps, no traces, one sync.
    threads: the triangle batch's instance (0: the one the batch selects); ran: a dict that
    receives the threads per workgroup of the instance that ran, under K."""
    n, p = X.shape
    b = me.bb.ChainBatch(me.config(n, p, true_alpha=true_alpha), K, X, y)
    try:
        if threads:
            b.set_threads(threads)
        if ran is not None:
            ran[K] = b.threads()
        b.init_state()
        b.run(1, 500, 0, 0, 0)
        b.sync()
        t0 = time.perf_counter()
        for s in range(0, nsamp, block):
            b.run(501 + s, min(block, nsamp - s), -1, 1, 1)
        b.sync()
        dt = time.perf_counter() - t0
        return K * nsamp / dt, b.resident_per_cu()
    finally:
        b.close()


def single_kernel_rate(me, X, y, nsamp):
    """kernel_rate for one bb.Engine (k_small_chain / k_tri_chain): the batch kernel's K = 1
    counterpart."""
    n, p = X.shape
    e = me.bb.Engine(me.config(n, p), X, y)
    try:
        e.init_state()
        e.run(1, 500, 0, 0, 0)
        e.sync()
        t0 = time.perf_counter()
        for s in range(0, nsamp, 50):
            e.run(501 + s, 50, -1, 1, 1)
        e.sync()
        return nsamp / (time.perf_counter() - t0)
    finally:
        e.close()


def bench_design(me, name, X, y, cus, args, Ks=None):
    bb = me.bb
    Ks = Ks or [k for k in dict.fromkeys([1, 8, 64, cus, 2 * cus, 4 * cus])
                if k <= args.max_chains]
    nsamp, burn = args.nsamp, args.burn
    bb.set_seed(SEED)
    me.chains(y, X, nsamp=200, nchains=2, burn=100)  # warm-up
    me.single(y, X, nsamp=200, burn=100)
    big = [k for k in (cus, 2 * cus, 4 * cus) if k <= args.max_chains] if me.tri else []
    inst = {(K, t): [] for K in big for t in args.instances}
    inst_res = {}
    rt = {K: [] for K in Ks}
    wall = {K: [] for K in Ks}
    kern = {K: [] for K in Ks}
    single, single_kern = [], []
    res = {}
    for _ in range(args.reps):
        bb.set_seed(SEED)
        single.append(nsamp / me.single(y, X, nsamp=nsamp, burn=burn)["runtime"])
        single_kern.append(single_kernel_rate(me, X, y, nsamp))
        for K in Ks:
            bb.set_seed(SEED)
            t0 = time.perf_counter()
            out = me.chains(y, X, nsamp=nsamp, nchains=K, burn=burn)
            wall[K].append(time.perf_counter() - t0)
            rt[K].append(out["runtime"])
            del out
            kr, res[K] = kernel_rate(me, X, y, K, nsamp)
            kern[K].append(kr)
        for K, t in inst:  # the instances side by side, every round
            kr, inst_res[K, t] = kernel_rate(me, X, y, K, nsamp, t)
            inst[K, t].append(kr)
    rows = []
    for K in Ks:
        agg = [K * nsamp / r for r in rt[K]]
        rows.append({"chains": K, "runtime_s": spread(rt[K]), "wall_s": spread(wall[K]),
                     "aggregate_sweeps_per_s": spread(agg),
                     "per_chain_sweeps_per_s": spread([a / K for a in agg]),
                     "kernel_aggregate_sweeps_per_s": spread(kern[K]),
                     "resident_per_cu": res[K]})
    one = rows[0]["aggregate_sweeps_per_s"]["median"]
    for r in rows:
        r["aggregate_vs_one_chain"] = r["aggregate_sweeps_per_s"]["median"] / one
        r["kernel_vs_one_chain"] = (r["kernel_aggregate_sweeps_per_s"]["median"] /
                                    rows[0]["kernel_aggregate_sweeps_per_s"]["median"])
    rec = {"design": name, "n": int(X.shape[0]), "p": int(X.shape[1]), "nsamp": nsamp,
           "burn": burn, "reps": args.reps, "compute_units": cus,
           "single_call_sweeps_per_s": spread(single),
           "single_kernel_sweeps_per_s": spread(single_kern), "chains": rows}
    if inst:
        rec["instances"] = [{"chains": K, "threads": t, "resident_per_cu": inst_res[K, t],
                             "kernel_aggregate_sweeps_per_s": spread(v)}
                            for (K, t), v in inst.items()]
    if name == "c1" and not me.tri:
        best = max(r["aggregate_sweeps_per_s"]["median"] for r in rows)
        rec["cpu_core_sweeps_per_s"] = CPU_CORE_C1
        rec["cpu_cores_worth"] = best / CPU_CORE_C1
    return rec


def summary_kernel_seconds(me, X, y, K, cap, nsamp, maxlag):
    """Seconds k_trace_summary takes for nsamp samples of K chains: one full ring of `cap`
    slots reduced alone (the sweeps that filled it already done), scaled to nsamp."""
    n, p = X.shape
    b = me.bb.ChainBatch(me.config(n, p, cap), K, X, y)
    try:
        b.init_state()
        b.run(1, cap - 1, 1, 1, 1)
        b.summary_reset(cap, maxlag)
        b.summary_add(0, 1, 0)  # the first launch of the kernel is not timed
        b.sync()
        t0 = time.perf_counter()
        b.summary_add(1, cap - 1, 1)
        b.sync()
        return (time.perf_counter() - t0) * nsamp / (cap - 1)
    finally:
        b.close()


def bench_summary(me, name, X, y, cus, args):
    """The summary call against the trace call, alternated within each round."""
    bb = me.bb
    Ks = [k for k in (args.chains or [cus, 4 * cus]) if k <= args.max_chains]
    nsamp, burn = args.nsamp, args.burn
    bb.set_seed(SEED)
    me.summary(y, X, nsamp=200, nchains=2, burn=100)  # warm-up
    me.chains(y, X, nsamp=200, nchains=2, burn=100)
    keys = ("summary", "trace", "kernel", "summary_kernel_s")
    v = {K: {k: [] for k in keys} for K in Ks}
    cap, lag = {}, 0
    for _ in range(args.reps):
        for K in Ks:
            bb.set_seed(SEED)
            out = me.summary(y, X, nsamp=nsamp, nchains=K, burn=burn)
            v[K]["summary"].append(K * nsamp / out["runtime"])
            cap[K], lag = bb.last_call_info()["trace_capacity"], out["maxlag"]
            bb.set_seed(SEED)
            out = me.chains(y, X, nsamp=nsamp, nchains=K, burn=burn)
            v[K]["trace"].append(K * nsamp / out["runtime"])
            del out
            v[K]["kernel"].append(kernel_rate(me, X, y, K, nsamp)[0])
            v[K]["summary_kernel_s"].append(
                summary_kernel_seconds(me, X, y, K, cap[K], nsamp, lag))
    rows = []
    for K in Ks:
        s, t = spread(v[K]["summary"]), spread(v[K]["trace"])
        ks = spread(v[K]["summary_kernel_s"])
        rows.append({"chains": K, "ring_capacity": cap[K],
                     "summary_call_sweeps_per_s": s, "trace_call_sweeps_per_s": t,
                     "kernel_aggregate_sweeps_per_s": spread(v[K]["kernel"]),
                     "summary_vs_trace": s["median"] / t["median"],
                     "k_trace_summary_s": ks,
                     "k_trace_summary_share": ks["median"] / (K * nsamp / s["median"])})
    from bayesbridge_amd import _kernel_code

    kname = "bb::k_trace_summary"
    return {"design": name, "n": int(X.shape[0]), "p": int(X.shape[1]), "nsamp": nsamp,
            "burn": burn, "reps": args.reps, "compute_units": cus, "maxlag": lag,
            "method": "tri" if me.tri else "stable", "chains": rows,
            "kernels": {kname: {"code_sha": _kernel_code.code_sha(kname)}}}


QUANTILE_PROBS = [0.025, 0.5, 0.975]


def hist_kernel_seconds(me, X, y, K, cap, nsamp, maxlag):
    """Seconds k_trace_hist takes for nsamp samples of K chains: a full ring of `cap` slots
    added with the quantile sketch enabled less the same add without it (both kernels run on
    the batch's stream, one behind the other), scaled to nsamp.  Returns (hist, both)."""
    n, p = X.shape
    b = me.bb.ChainBatch(me.config(n, p, cap), K, X, y)
    try:
        b.init_state()
        b.run(1, cap - 1, 1, 1, 1)
        took = []
        for sketch in (False, True):
            b.summary_reset(cap, maxlag)
            if sketch:
                b.quantiles_reset()
            b.summary_add(0, 1, 0)  # the first launches are not timed
            b.sync()
            t0 = time.perf_counter()
            b.summary_add(1, cap - 1, 1)
            b.sync()
            took.append((time.perf_counter() - t0) * nsamp / (cap - 1))
        return took[1] - took[0], took[1]
    finally:
        b.close()


def bench_summary_quantiles(me, name, X, y, cus, args):
    """The summary call with probs against the summary call without and the trace call,
    alternated within each round."""
    bb = me.bb
    Ks = [k for k in (args.chains or [cus, 4 * cus]) if k <= args.max_chains]
    nsamp, burn = args.nsamp, args.burn
    bb.set_seed(SEED)
    me.summary(y, X, nsamp=200, nchains=2, burn=100, probs=QUANTILE_PROBS)  # warm-up
    me.summary(y, X, nsamp=200, nchains=2, burn=100)
    me.chains(y, X, nsamp=200, nchains=2, burn=100)
    keys = ("quantiles", "summary", "trace", "hist_s", "both_s")
    v = {K: {k: [] for k in keys} for K in Ks}
    cap, lag = {}, 0
    for _ in range(args.reps):
        for K in Ks:
            bb.set_seed(SEED)
            out = me.summary(y, X, nsamp=nsamp, nchains=K, burn=burn, probs=QUANTILE_PROBS)
            v[K]["quantiles"].append(K * nsamp / out["runtime"])
            cap[K], lag = bb.last_call_info()["trace_capacity"], out["maxlag"]
            bb.set_seed(SEED)
            out = me.summary(y, X, nsamp=nsamp, nchains=K, burn=burn)
            v[K]["summary"].append(K * nsamp / out["runtime"])
            bb.set_seed(SEED)
            out = me.chains(y, X, nsamp=nsamp, nchains=K, burn=burn)
            v[K]["trace"].append(K * nsamp / out["runtime"])
            del out
            h, both = hist_kernel_seconds(me, X, y, K, cap[K], nsamp, lag)
            v[K]["hist_s"].append(h)
            v[K]["both_s"].append(both)
    rows = []
    for K in Ks:
        q, s, t = (spread(v[K][k]) for k in ("quantiles", "summary", "trace"))
        hs = spread(v[K]["hist_s"])
        rows.append({"chains": K, "ring_capacity": cap[K],
                     "quantiles_call_sweeps_per_s": q, "summary_call_sweeps_per_s": s,
                     "trace_call_sweeps_per_s": t,
                     "quantiles_vs_trace": q["median"] / t["median"],
                     "quantiles_vs_summary": q["median"] / s["median"],
                     "k_trace_hist_s": hs, "summary_and_hist_s": spread(v[K]["both_s"]),
                     "k_trace_hist_share": hs["median"] / (K * nsamp / q["median"])})
    from bayesbridge_amd import _kernel_code

    return {"design": name, "n": int(X.shape[0]), "p": int(X.shape[1]), "nsamp": nsamp,
            "burn": burn, "reps": args.reps, "compute_units": cus, "maxlag": lag,
            "probs": QUANTILE_PROBS, "method": "tri" if me.tri else "stable", "chains": rows,
            "kernels": {k: {"code_sha": _kernel_code.code_sha(k)}
                        for k in ("bb::k_trace_hist", "bb::k_quantile_select",
                                  "bb::k_trace_summary")}}


WIDE_BLOCK = 16  # sweeps per launch of the wide kernels' drivers (bb_kernels.h kWideBlock)


def bench_wide(me, name, X, y, cus, args):
    """The wide fused chains (key 25) against the general path, alternated within each round.
    The key is set only around the calls it is measured in and left off."""
    bb = me.bb
    Ks = [k for k in dict.fromkeys([8, cus, 2 * cus]) if k <= args.max_chains]
    nsamp, burn = args.nsamp, args.burn

    def call(on, fn):
        old = bb.set_tuning(25, 1 if on else 0)
        try:
            bb.set_seed(SEED)
            return fn()
        finally:
            bb.set_tuning(25, old)

    for on in (0, 1):  # warm-up
        call(on, lambda: me.single(y, X, nsamp=100, burn=50))
    call(1, lambda: me.chains(y, X, nsamp=100, nchains=2, burn=50))
    off, on_, res = [], [], {}
    agg = {K: [] for K in Ks}
    kern = {K: [] for K in Ks}
    for _ in range(args.reps):
        off.append(nsamp / call(0, lambda: me.single(y, X, nsamp=nsamp, burn=burn))["runtime"])
        on_.append(nsamp / call(1, lambda: me.single(y, X, nsamp=nsamp, burn=burn))["runtime"])
        for K in Ks:
            out = call(1, lambda: me.chains(y, X, nsamp=nsamp, nchains=K, burn=burn))
            agg[K].append(K * nsamp / out["runtime"])
            del out
            kr, res[K] = call(1, lambda: kernel_rate(me, X, y, K, nsamp, block=WIDE_BLOCK))
            kern[K].append(kr)
    s_off, s_on = spread(off), spread(on_)
    rows = []
    for K in Ks:
        a = spread(agg[K])
        rows.append({"chains": K, "aggregate_sweeps_per_s": a,
                     "kernel_aggregate_sweeps_per_s": spread(kern[K]),
                     "resident_per_cu": res[K],
                     # K sequential key-off calls run at the single call's rate in aggregate
                     "vs_sequential_general_path": a["median"] / s_off["median"],
                     "beats_sequential_beyond_spread": a["min"] > s_off["max"]})
    from bayesbridge_amd import _kernel_code

    inst = "64, 256" if X.shape[1] <= 64 else "128, 512"
    kernels = {k: {"code_sha": _kernel_code.code_sha(k)}
               for k in (f"bb::k_wide_chain<{inst}>", f"bb::k_wide_chains<{inst}>")}
    return {"design": name, "n": int(X.shape[0]), "p": int(X.shape[1]), "nsamp": nsamp,
            "burn": burn, "reps": args.reps, "compute_units": cus,
            "single_call_general_path_sweeps_per_s": s_off,
            "single_call_wide_sweeps_per_s": s_on,
            "single_wide_vs_general_path": s_on["median"] / s_off["median"],
            "single_wide_beats_general_path_beyond_spread": s_on["min"] > s_off["max"],
            "chains": rows, "kernels": kernels}


# bb_set_tuning: alpha sampled in the fused small chains (bb_small_mh.hip) and in the fused
# triangle chains (bb_tri_mh.hip)
ALPHA_KEY, TRI_ALPHA_KEY = 26, 27


def alpha_kernels(me, p, threads):
    """The kernels a --alpha run launches: the single chain's and the batch's alpha-sampling
    instances and the known-alpha batch's; threads: the triangle batch instances it ran."""
    if me.tri:
        inst = sorted({f"{t}, {'false' if t == 512 else 'true'}" for t in threads})
        anon = "bb::(anonymous namespace)::"
        return ([anon + "k_tri_chain_mh"] + [anon + f"k_tri_chains_mh<{i}>" for i in inst]
                + [anon + f"k_tri_chains<{i}>" for i in inst])
    lanes = "512, 64, 16" if p <= 8 else "512, 32, 8" if p <= 16 else "512, 16, 8"
    return [f"bb::k_small_chain_mh<{lanes}>", f"bb::k_small_chains_mh<{lanes}>",
            f"bb::k_small_chains<{lanes}>"]


def bench_alpha(me, name, X, y, cus, args):
    """Alpha unknown (alpha = 0: sampled by MH) under key 26 (--method tri: key 27) against this
    tree's known-alpha batch, alternated within each round; the key is set only around the calls
    it is measured in and left off.  The sequential general-path fallback at the same K comes
    from --baseline."""
    bb = me.bb
    key = TRI_ALPHA_KEY if me.tri else ALPHA_KEY
    Ks = [k for k in (args.chains or [1, 256, 1024]) if k <= args.max_chains]
    nsamp, burn = args.nsamp, args.burn

    def call(on, fn):
        old = bb.set_tuning(key, 1 if on else 0)
        try:
            bb.set_seed(SEED)
            return fn()
        finally:
            bb.set_tuning(key, old)

    call(1, lambda: me.chains(y, X, nsamp=200, nchains=2, burn=100, alpha=0.0))  # warm-up
    call(1, lambda: me.single(y, X, nsamp=200, burn=100, alpha=0.0))
    call(0, lambda: me.single(y, X, nsamp=200, burn=100, alpha=0.0))
    call(0, lambda: me.chains(y, X, nsamp=200, nchains=2, burn=100))
    keys = ("mh", "mh_kernel", "known", "known_kernel")
    v = {K: {k: [] for k in keys} for K in Ks}
    one_fused, one_general, res, ran = [], [], {}, {}
    for _ in range(args.reps):
        one_fused.append(nsamp / call(1, lambda: me.single(y, X, nsamp=nsamp, burn=burn,
                                                           alpha=0.0))["runtime"])
        one_general.append(nsamp / call(0, lambda: me.single(y, X, nsamp=nsamp, burn=burn,
                                                             alpha=0.0))["runtime"])
        for K in Ks:
            out = call(1, lambda: me.chains(y, X, nsamp=nsamp, nchains=K, burn=burn, alpha=0.0))
            v[K]["mh"].append(K * nsamp / out["runtime"])
            del out
            kr, res[K] = call(1, lambda: kernel_rate(me, X, y, K, nsamp, true_alpha=0.0,
                                                     ran=ran))
            v[K]["mh_kernel"].append(kr)
            out = call(0, lambda: me.chains(y, X, nsamp=nsamp, nchains=K, burn=burn))
            v[K]["known"].append(K * nsamp / out["runtime"])
            del out
            v[K]["known_kernel"].append(call(0, lambda: kernel_rate(me, X, y, K, nsamp))[0])
    base = {}
    if args.baseline:
        with open(args.baseline) as f:
            for line in f:
                if line.startswith("{"):
                    rec = json.loads(line)
                    base.update(rec.get("fallback_chains_sweeps_per_s", {}).get(name, {}))
                    base_meta = {k: rec.get(k) for k in ("source_sha", "nsamp", "burn", "reps")}
    rows = []
    for K in Ks:
        s = {k: spread(v[K][k]) for k in keys}
        row = {"chains": K, "resident_per_cu": res[K], "threads": ran[K],
               "alpha_sampled_call_sweeps_per_s": s["mh"],
               "alpha_sampled_kernel_sweeps_per_s": s["mh_kernel"],
               "alpha_known_call_sweeps_per_s": s["known"],
               "alpha_known_kernel_sweeps_per_s": s["known_kernel"],
               "sampled_vs_known_call": s["mh"]["median"] / s["known"]["median"],
               "sampled_vs_known_kernel": s["mh_kernel"]["median"] / s["known_kernel"]["median"]}
        fb = base.get(str(K))
        if fb:
            row["fallback_general_path_sweeps_per_s"] = fb
            row["vs_fallback"] = s["mh"]["median"] / fb["median"]
            row["beats_fallback_beyond_spread"] = s["mh"]["min"] > fb["max"]
        rows.append(row)
    from bayesbridge_amd import _kernel_code

    kernels = {k: {"code_sha": _kernel_code.code_sha(k)}
               for k in alpha_kernels(me, X.shape[1], ran.values())}
    f1, g1 = spread(one_fused), spread(one_general)
    rec = {"design": name, "n": int(X.shape[0]), "p": int(X.shape[1]), "nsamp": nsamp,
           "burn": burn, "reps": args.reps, "compute_units": cus,
           "method": "tri" if me.tri else "stable", "tuning_key": key,
           "single_call_fused_sweeps_per_s": f1, "single_call_general_path_sweeps_per_s": g1,
           "single_fused_vs_general_path": f1["median"] / g1["median"],
           "chains": rows, "kernels": kernels}
    if base:
        rec["fallback_measured_with"] = base_meta
    return rec


def bench_alpha_fallback(me, args):
    """bridge_reg_stb_chains(alpha = 0) (--method tri: bridge_reg_tri_chains) with every key as
    the checkout has it (one JSON line): on a checkout without key 26 (27), or with it off, K
    sequential general-path chains -- the baseline of --alpha, through --baseline."""
    out = {}
    for name, (X, y) in designs().items():
        if name not in args.designs.split(","):
            continue
        me.bb.set_seed(SEED)
        me.chains(y, X, nsamp=50, nchains=2, burn=20, alpha=0.0)
        out[name] = {}
        for K in args.chains or [1, 256, 1024]:
            v = []
            for _ in range(args.reps):
                me.bb.set_seed(SEED)
                r = me.chains(y, X, nsamp=args.nsamp, nchains=K, burn=args.burn, alpha=0.0)
                v.append(K * args.nsamp / r["runtime"])
                del r
            out[name][str(K)] = spread(v)
            print(f"{name} K={K:5d} fallback {out[name][str(K)]}", file=sys.stderr, flush=True)
    print(json.dumps({"source_sha": me.bb._build.source_sha(), "method": args.method,
                      "nsamp": args.nsamp, "burn": args.burn, "reps": args.reps,
                      "fallback_chains_sweeps_per_s": out}), flush=True)


def logit_kernel_rate(bb, X, y, K, nsamp):
    """kernel_rate for the logistic batch (method 6)."""
    n, p = X.shape
    b = bb.ChainBatch(bb.EngineConfig(n=n, p=p, seed=SEED, method=6), K, X, y)
    try:
        b.init_state()
        b.run(1, 200, 0, 0, 0)
        b.sync()
        t0 = time.perf_counter()
        for s in range(0, nsamp, 50):
            b.run(201 + s, min(50, nsamp - s), -1, 1, 1)
        b.sync()
        return K * nsamp / (time.perf_counter() - t0), b.resident_per_cu()
    finally:
        b.close()


def bench_logit(bb, name, X, y, cus, args):
    """The logistic batch against the single general-path call, alternated within each round."""
    sys.path.insert(0, ROOT)
    import oracle

    Ks = [k for k in (args.chains or dict.fromkeys([1, cus, 4 * cus])) if k <= args.max_chains]
    nsamp, burn = args.nsamp, args.burn
    bb.set_seed(SEED)
    bb.bridge_reg_logit(y, X, nsamp=100, burn=50)  # warm-up
    bb.bridge_reg_logit_chains(y, X, nsamp=100, nchains=2, burn=50)
    bb.bridge_reg_logit_chains_summary(y, X, nsamp=100, nchains=2, burn=50)
    keys = ("call", "kernel", "summary")
    v = {K: {k: [] for k in keys} for K in Ks}
    single, cpu, res = [], [], {}
    for _ in range(args.reps):
        bb.set_seed(SEED)
        single.append(nsamp / bb.bridge_reg_logit(y, X, nsamp=nsamp, burn=burn)["runtime"])
        t0 = time.perf_counter()
        oracle.cpu_logit_chain(y, X, nsamp, burn=burn, seed=SEED, stream=0)
        cpu.append((nsamp + burn) / (time.perf_counter() - t0))
        for K in Ks:
            bb.set_seed(SEED)
            out = bb.bridge_reg_logit_chains(y, X, nsamp=nsamp, nchains=K, burn=burn)
            v[K]["call"].append(K * nsamp / out["runtime"])
            del out
            kr, res[K] = logit_kernel_rate(bb, X, y, K, nsamp)
            v[K]["kernel"].append(kr)
            bb.set_seed(SEED)
            out = bb.bridge_reg_logit_chains_summary(y, X, nsamp=nsamp, nchains=K, burn=burn)
            v[K]["summary"].append(K * nsamp / out["runtime"])
    base, base_meta = None, None
    if args.baseline:
        with open(args.baseline) as f:
            for line in f:
                if line.startswith("{"):
                    r = json.loads(line)
                    base = r.get("single_call_sweeps_per_s", {}).get(name, base)
                    base_meta = {k: r.get(k) for k in ("source_sha", "nsamp", "burn", "reps")}
    s1, c1 = spread(single), spread(cpu)
    rows = []
    for K in Ks:
        s = {k: spread(v[K][k]) for k in keys}
        row = {"chains": K, "resident_per_cu": res[K], "call_sweeps_per_s": s["call"],
               "kernel_sweeps_per_s": s["kernel"], "summary_call_sweeps_per_s": s["summary"],
               # K sequential single calls run at the single call's rate in aggregate
               "vs_sequential_this_tree": s["call"]["median"] / s1["median"],
               "cpu_cores_worth": s["call"]["median"] / c1["median"]}
        if base:
            row["vs_sequential_parent"] = s["call"]["median"] / base["median"]
            row["beats_sequential_parent_beyond_spread"] = s["call"]["min"] > base["max"]
        rows.append(row)
    from bayesbridge_amd import _kernel_code

    p = X.shape[1]
    lanes = "512, 64, 16" if p <= 8 else "512, 32, 8" if p <= 16 else "512, 16, 8"
    kname = f"bb::k_logit_chains<{lanes}, false>"
    rec = {"design": name, "n": int(X.shape[0]), "p": int(p), "nsamp": nsamp, "burn": burn,
           "reps": args.reps, "compute_units": cus, "single_call_sweeps_per_s": s1,
           "cpu_core_oracle_sweeps_per_s": c1, "chains": rows,
           "kernels": {kname: {"code_sha": _kernel_code.code_sha(kname)}}}
    if base:
        rec["parent_single_call_sweeps_per_s"] = base
        rec["parent_measured_with"] = base_meta
    return rec


def bench_logit_single(bb, args):
    """bridge_reg_logit alone at the logistic designs (one JSON line): the baseline of --logit,
    through --baseline."""
    out = {}
    for name, (X, y) in logit_designs().items():
        if name not in args.designs.split(","):
            continue
        bb.set_seed(SEED)
        bb.bridge_reg_logit(y, X, nsamp=100, burn=50)
        v = []
        for _ in range(args.reps):
            bb.set_seed(SEED)
            v.append(args.nsamp / bb.bridge_reg_logit(y, X, nsamp=args.nsamp,
                                                      burn=args.burn)["runtime"])
        out[name] = spread(v)
        print(f"{name} single call {out[name]}", file=sys.stderr, flush=True)
    print(json.dumps({"tree": args.tree, "source_sha": bb._build.source_sha(),
                      "nsamp": args.nsamp, "burn": args.burn, "reps": args.reps,
                      "single_call_sweeps_per_s": out}), flush=True)


def bench_single(me, args):
    """The single-chain call alone at both designs (one JSON line): the A/B against another
    checkout."""
    if args.alpha:
        return bench_alpha_fallback(me, args)
    if args.logit:
        return bench_logit_single(me.bb, args)
    out = {}
    for name, (X, y) in designs().items():
        if name not in args.designs.split(","):
            continue
        me.bb.set_seed(SEED)
        me.single(y, X, nsamp=200, burn=100)
        v = []
        for _ in range(args.reps):
            me.bb.set_seed(SEED)
            v.append(args.nsamp / me.single(y, X, nsamp=args.nsamp, burn=args.burn)["runtime"])
        out[name] = spread(v)
    print(json.dumps({"tree": args.tree, "method": args.method,
                      "single_call_sweeps_per_s": out}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=["chains", "single"], default="chains")
    ap.add_argument("--method", choices=["stable", "tri"], default="stable")
    ap.add_argument("--tree", default=ROOT, help="checkout whose bayesbridge_amd is measured")
    ap.add_argument("--designs", default=None, help="default c1,db (--wide: dbi,bhi)")
    ap.add_argument("--nsamp", type=int, default=None, help="default 5000 (--wide: 1000)")
    ap.add_argument("--burn", type=int, default=None, help="default 500 (--wide: 200)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-chains", type=int, default=1 << 20)
    ap.add_argument("--tuning", default="",
                    help="KEY=VALUE,...: bb_set_tuning before measuring (A/B of a variant build)")
    ap.add_argument("--instances", type=lambda v: [int(t) for t in v.split(",")],
                    default=[512, 256, 128], help="triangle batch instances to compare (threads)")
    ap.add_argument("--summary", action="store_true",
                    help="the summary mode against the trace call (profiles/chains_summary_*)")
    ap.add_argument("--quantiles", action="store_true",
                    help="with --summary: the call with pooled quantiles against the call "
                         "without and the trace call (profiles/chains_summary_quantiles_*)")
    ap.add_argument("--wide", action="store_true",
                    help="the wide fused chains (key 25) at dbi / bhi (profiles/chains_wide_*)")
    ap.add_argument("--alpha", action="store_true",
                    help="alpha unknown under key 26 (profiles/chains_alpha_*); --method tri: "
                         "under key 27 (profiles/chains_tri_alpha_*)")
    ap.add_argument("--logit", action="store_true",
                    help="the logistic chain batch at lg5 / lg32 (profiles/chains_logit_*)")
    ap.add_argument("--baseline", default=None,
                    help="--alpha / --logit: the JSON line of a --mode single run to merge")
    ap.add_argument("--chains", type=lambda v: [int(t) for t in v.split(",")], default=None,
                    help="--summary: the batch sizes (default CUs,4 CUs); --alpha: 1,256,1024")
    ap.add_argument("--tag", default="", help="suffix of the output files' names")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    args.designs = args.designs or ("dbi,bhi" if args.wide else "lg5,lg32" if args.logit
                                    else "c1,db")
    args.nsamp = args.nsamp or (1000 if args.wide or args.logit else 5000)
    args.burn = args.burn if args.burn is not None else (200 if args.wide or args.logit else 500)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    import bayesbridge_amd as bb

    bb.set_verbose(0)
    for kv in filter(None, args.tuning.split(",")):
        k, v = kv.split("=")
        bb.set_tuning(int(k), int(v))
    me = Method(bb, args.method)
    if args.mode == "single":
        return bench_single(me, args)
    cus = (bb.compute_units() if hasattr(bb, "compute_units")
           else int(torch.cuda.get_device_properties(0).multi_processor_count))
    for name, (X, y) in (logit_designs() if args.logit else designs()).items():
        if name not in args.designs.split(","):
            continue
        if args.logit:
            rec = bench_logit(bb, name, X, y, cus, args)
            rec["source_sha"] = bb._build.source_sha()
            with open(os.path.join(args.out_dir, f"chains_logit_{name}{args.tag}.json"), "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
            s1, c1 = rec["single_call_sweeps_per_s"], rec["cpu_core_oracle_sweeps_per_s"]
            print(f"{name} single call {s1['median']:.0f} sweeps/s [{s1['min']:.0f}, "
                  f"{s1['max']:.0f}]  one CPU core {c1['median']:.0f}", flush=True)
            for r in rec["chains"]:
                a, k, sm = (r["call_sweeps_per_s"], r["kernel_sweeps_per_s"],
                            r["summary_call_sweeps_per_s"])
                print(f"{name} K={r['chains']:5d} call {a['median']:.0f} sweeps/s "
                      f"[{a['min']:.0f}, {a['max']:.0f}]  kernel {k['median']:.0f}  summary "
                      f"{sm['median']:.0f}  x{r['vs_sequential_this_tree']:.0f} sequential"
                      + (f" (x{r['vs_sequential_parent']:.0f} parent)"
                         if "vs_sequential_parent" in r else "")
                      + f"  resident/CU {r['resident_per_cu']}", flush=True)
            continue
        if args.alpha:
            rec = bench_alpha(me, name, X, y, cus, args)
            rec["source_sha"] = bb._build.source_sha()
            stem = "chains_tri_alpha_" if me.tri else "chains_alpha_"
            with open(os.path.join(args.out_dir, f"{stem}{name}{args.tag}.json"), "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
            f1, g1 = rec["single_call_fused_sweeps_per_s"], rec["single_call_general_path_sweeps_per_s"]
            print(f"{name} single call, alpha sampled: general path {g1['median']:.0f} sweeps/s "
                  f"[{g1['min']:.0f}, {g1['max']:.0f}]  fused {f1['median']:.0f} "
                  f"[{f1['min']:.0f}, {f1['max']:.0f}]  "
                  f"x{rec['single_fused_vs_general_path']:.2f}", flush=True)
            for r in rec["chains"]:
                a, k = r["alpha_sampled_call_sweeps_per_s"], r["alpha_sampled_kernel_sweeps_per_s"]
                fb = r.get("fallback_general_path_sweeps_per_s")
                print(f"{name} K={r['chains']:5d} alpha sampled {a['median']:.0f} sweeps/s "
                      f"[{a['min']:.0f}, {a['max']:.0f}]  kernel {k['median']:.0f}  "
                      f"x{r['sampled_vs_known_call']:.2f} known alpha (kernel "
                      f"x{r['sampled_vs_known_kernel']:.2f})"
                      + (f"  x{r['vs_fallback']:.0f} fallback {fb['median']:.0f}" if fb else "")
                      + f"  resident/CU {r['resident_per_cu']}", flush=True)
            continue
        if args.wide:
            rec = bench_wide(me, name, X, y, cus, args)
            rec["source_sha"] = bb._build.source_sha()
            with open(os.path.join(args.out_dir, f"chains_wide_{name}{args.tag}.json"), "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
            g, w = rec["single_call_general_path_sweeps_per_s"], rec["single_call_wide_sweeps_per_s"]
            print(f"{name} single call: general path {g['median']:.0f} sweeps/s [{g['min']:.0f}, "
                  f"{g['max']:.0f}]  wide {w['median']:.0f} [{w['min']:.0f}, {w['max']:.0f}]  "
                  f"x{rec['single_wide_vs_general_path']:.2f}", flush=True)
            for r in rec["chains"]:
                a, k = r["aggregate_sweeps_per_s"], r["kernel_aggregate_sweeps_per_s"]
                print(f"{name} K={r['chains']:5d} aggregate {a['median']:.0f} sweeps/s "
                      f"[{a['min']:.0f}, {a['max']:.0f}]  kernel {k['median']:.0f}  "
                      f"x{r['vs_sequential_general_path']:.1f} sequential  resident/CU "
                      f"{r['resident_per_cu']}", flush=True)
            continue
        if args.summary and args.quantiles:
            rec = bench_summary_quantiles(me, name, X, y, cus, args)
            rec["source_sha"] = bb._build.source_sha()
            stem = "chains_summary_quantiles_tri_" if me.tri else "chains_summary_quantiles_"
            with open(os.path.join(args.out_dir, f"{stem}{name}{args.tag}.json"), "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
            for r in rec["chains"]:
                q, s, t = (r[k + "_call_sweeps_per_s"] for k in ("quantiles", "summary", "trace"))
                print(f"{name} K={r['chains']:5d} quantiles {q['median']:.0f} sweeps/s "
                      f"[{q['min']:.0f}, {q['max']:.0f}]  summary {s['median']:.0f} "
                      f"[{s['min']:.0f}, {s['max']:.0f}]  trace {t['median']:.0f} "
                      f"[{t['min']:.0f}, {t['max']:.0f}]  x{r['quantiles_vs_trace']:.2f} trace  "
                      f"k_trace_hist {100 * r['k_trace_hist_share']:.2f} %", flush=True)
            continue
        if args.summary:
            rec = bench_summary(me, name, X, y, cus, args)
            rec["source_sha"] = bb._build.source_sha()
            stem = "chains_summary_tri_" if me.tri else "chains_summary_"
            with open(os.path.join(args.out_dir, f"{stem}{name}{args.tag}.json"), "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
            for r in rec["chains"]:
                s, t = r["summary_call_sweeps_per_s"], r["trace_call_sweeps_per_s"]
                print(f"{name} K={r['chains']:5d} summary {s['median']:.0f} sweeps/s "
                      f"[{s['min']:.0f}, {s['max']:.0f}]  trace {t['median']:.0f} "
                      f"[{t['min']:.0f}, {t['max']:.0f}]  kernel "
                      f"{r['kernel_aggregate_sweeps_per_s']['median']:.0f}  x"
                      f"{r['summary_vs_trace']:.2f}  k_trace_summary "
                      f"{100 * r['k_trace_summary_share']:.2f} %", flush=True)
            continue
        rec = bench_design(me, name, X, y, cus, args)
        # the two-chains-per-CU instance (bb_set_tuning key 21) where it applies: K >= 2 CUs
        big = [k for k in (2 * cus, 4 * cus) if k <= args.max_chains]
        if big and not me.tri and not args.tuning and bb.set_tuning(21, -1) >= 0:
            bb.set_tuning(21, 1)
            try:
                rec["chains_two_per_cu"] = bench_design(me, name, X, y, cus, args, big)["chains"]
            finally:
                bb.set_tuning(21, 0)
        rec["source_sha"] = bb._build.source_sha()
        stem = "chains_tri_" if me.tri else "chains_"
        path = os.path.join(args.out_dir, f"{stem}{name}{args.tag}.json")
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        for r in rec["chains"]:
            print(f"{name} K={r['chains']:5d} runtime {r['runtime_s']['median']:.4f} s  "
                  f"aggregate {r['aggregate_sweeps_per_s']['median']:.0f} sweeps/s "
                  f"[{r['aggregate_sweeps_per_s']['min']:.0f}, "
                  f"{r['aggregate_sweeps_per_s']['max']:.0f}]  "
                  f"kernel {r['kernel_aggregate_sweeps_per_s']['median']:.0f}  "
                  f"x{r['aggregate_vs_one_chain']:.1f}  resident/CU {r['resident_per_cu']}",
                  flush=True)
        for r in rec.get("chains_two_per_cu", []):
            print(f"{name} two per CU K={r['chains']:5d} aggregate "
                  f"{r['aggregate_sweeps_per_s']['median']:.0f} sweeps/s "
                  f"[{r['aggregate_sweeps_per_s']['min']:.0f}, "
                  f"{r['aggregate_sweeps_per_s']['max']:.0f}]  kernel "
                  f"{r['kernel_aggregate_sweeps_per_s']['median']:.0f}  "
                  f"resident/CU {r['resident_per_cu']}", flush=True)
        for r in rec.get("instances", []):
            k = r["kernel_aggregate_sweeps_per_s"]
            print(f"{name} instance {r['threads']:3d} threads K={r['chains']:5d} kernel "
                  f"{k['median']:.0f} [{k['min']:.0f}, {k['max']:.0f}]  "
                  f"resident/CU {r['resident_per_cu']}", flush=True)
        print(f"{name} single call {rec['single_call_sweeps_per_s']} kernel "
              f"{rec['single_kernel_sweeps_per_s']}", flush=True)


if __name__ == "__main__":
    main()
