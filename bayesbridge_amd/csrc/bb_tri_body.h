// bb_tri_body.h -- the truncated-normal draws of the triangle mixture and the sweep loop of its
// fused chain (gfx950), shared by two translation units: bb_tri.hip (the general update, the
// fused chains with alpha known) and bb_tri_mh.hip (the fused chains with alpha sampled).  They
// are two code objects, so that the out-of-line MH decision of bb_chain_steps.h is no part of the
// known-alpha kernels' code identity (bayesbridge_amd/_kernel_code.py).
#pragma once
#include <hip/hip_runtime.h>

#include "bb_chain_steps.h"

namespace bb {

namespace {

constexpr int kTriNT = 256;
constexpr int kTriE = kTriMaxP / kTriNT;  // coefficients per thread
constexpr long kTnMaxAttempts = 1l << 22;
constexpr unsigned KIND_TRI_OMEGA = 8, KIND_TRI_U = 9, KIND_TRI_Z = 10;

// Attempt 0 of every coordinate's draw is precomputed in parallel before the coordinate
// loop (pre = {r0, r1, Box-Muller normal of (r0, r1)}), so the serial chain only runs
// Philox on a rejection.  Bit-identical to drawing it in place.
struct Pre {
    double r0, r1, x0;
};

__device__ __forceinline__ void attempt(Key key, uint64_t t, uint64_t i, uint64_t it, long k,
                                        const Pre &pre, double &r0, double &r1, double &x0,
                                        bool need_x) {
    if (k == 0) {
        r0 = pre.r0;
        r1 = pre.r1;
        x0 = pre.x0;
    } else {
        U4 r = uniforms(key, t, KIND_TRI_Z, i, it, (uint64_t)k);
        r0 = r.r[0];
        r1 = r.r[1];
        x0 = need_x ? bm_normal(r0, r1) : 0.0;
    }
}

// Force-inlined: the compiler outlined tnorm, and an out-of-line call inside the
// coordinate loop costs its prologue's s_waitcnt vmcnt(0), which drains the row prefetch
// on every coordinate.  k0 > 0 resumes the rejection loop at attempt k0 (k_tri_chain's
// fall-through after its parallel attempts; `pre` is then unused).
// LOST (k_tri_chains): a standardised bound beyond ~1e154 overflows a * a, the threshold is
// NaN and no attempt can be accepted; the draw then takes the loop's outcome (flag 64, the
// bound itself) at once instead of after kTnMaxAttempts rounds on a CU other chains wait for.
template <bool LOST = false>
__device__ __forceinline__ double tn_pos(double a, double b, Key key, uint64_t t, uint64_t i,
                                         uint64_t it, const Pre &pre, uint32_t *err,
                                         long k0 = 0) {
    const double sq = sqrt(a * a + 4.0);
    const double as = 0.5 * (a + sq);
    const double thr = a + 2.0 / (a + sq) * exp(0.5 + 0.25 * (a * a - a * sq));
    if (LOST && thr != thr) {
        atomicOr(err, 64u);
        return a;
    }
    for (long k = k0; k < kTnMaxAttempts; ++k) {
        double r0, r1, x0;
        attempt(key, t, i, it, k, pre, r0, r1, x0, false);
        if (b <= thr) {
            const double x = a + (b - a) * r0;
            if (r1 <= exp(0.5 * (a * a - x * x))) return x;
        } else {
            const double x = a - log(r0) / as;
            const double e = x - as;
            if (x <= b && r1 <= exp(-0.5 * e * e)) return x;
        }
    }
    atomicOr(err, 64u);
    return a;
}

template <bool LOST = false>
__device__ __forceinline__ double tnorm(double lo, double hi, double mu, double sd, Key key,
                                        uint64_t t, uint64_t i, uint64_t it, const Pre &pre,
                                        uint32_t *err, long k0 = 0) {
    const double a = (lo - mu) / sd, b = (hi - mu) / sd;
    if (!(a < b)) {
        atomicOr(err, 128u);
        return lo;
    }
    if (a <= 0.0 && b >= 0.0) {
        const bool wide = (b - a) >= 2.5066282746310002;  // sqrt(2 pi)
        for (long k = k0; k < kTnMaxAttempts; ++k) {
            double r0, r1, x0;
            attempt(key, t, i, it, k, pre, r0, r1, x0, wide);
            if (wide) {
                if (x0 >= a && x0 <= b) return mu + sd * x0;
            } else {
                const double x = a + (b - a) * r0;
                if (r1 <= exp(-0.5 * x * x)) return mu + sd * x;
            }
        }
        atomicOr(err, 64u);
        return lo;
    }
    if (a > 0.0) return mu + sd * tn_pos<LOST>(a, b, key, t, i, it, pre, err, k0);
    return mu - sd * tn_pos<LOST>(-b, -a, key, t, i, it, pre, err, k0);
}

// The same draw with attempts 0 .. K-1 evaluated in parallel, attempt k in lane k from its
// precomputed (r0, r1, x0): the lowest accepted attempt is the sequential loop's answer;
// if none of the K is accepted the loop resumes at attempt K.  lo, hi, mu, sd uniform; every
// lane of the wave calls this.
template <int K, bool LOST>
__device__ __forceinline__ double tnorm_par(double lo, double hi, double mu, double sd,
                                            double r0, double r1, double x0, Key key,
                                            uint64_t t, uint64_t i, uint64_t it, uint32_t *err) {
    const int lane = threadIdx.x & 63;
    const double a = (lo - mu) / sd, b = (hi - mu) / sd;
    if (!(a < b)) {
        atomicOr(err, 128u);
        return lo;
    }
    bool acc = false;
    double val = 0.0;
    if (a <= 0.0 && b >= 0.0) {
        if ((b - a) >= 2.5066282746310002) {  // sqrt(2 pi)
            acc = x0 >= a && x0 <= b;
            val = mu + sd * x0;
        } else {
            const double x = a + (b - a) * r0;
            acc = r1 <= exp(-0.5 * x * x);
            val = mu + sd * x;
        }
    } else {
        const double pa = a > 0.0 ? a : -b, pb = a > 0.0 ? b : -a;  // tn_pos's (a, b)
        const double sq = sqrt(pa * pa + 4.0);
        const double as = 0.5 * (pa + sq);
        const double thr = pa + 2.0 / (pa + sq) * exp(0.5 + 0.25 * (pa * pa - pa * sq));
        double x;
        if (pb <= thr) {
            x = pa + (pb - pa) * r0;
            acc = r1 <= exp(0.5 * (pa * pa - x * x));
        } else {
            x = pa - log(r0) / as;
            const double e = x - as;
            acc = x <= pb && r1 <= exp(-0.5 * e * e);
        }
        val = a > 0.0 ? mu + sd * x : mu - sd * x;
    }
    const uint64_t m = __ballot(acc && lane < K);
    if (m) return readlane_f64(val, __ffsll((unsigned long long)m) - 1);
    return tnorm<LOST>(lo, hi, mu, sd, key, t, i, it, Pre{0.0, 0.0, 0.0}, err, K);
}

// Row-of-16 max / min through DPP (quad xor 1, quad xor 2, half-row mirror, row mirror):
// every lane of a 16-lane row ends with the row's extreme.  v_max_f64 takes no DPP operand
// on gfx9, so each step moves the two halves with v_mov_b32_dpp.  Replaces a 6-step
// ds_bpermute butterfly per value (an LDS round trip per step).
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double row16_max(double v) {
    v = fmax(v, dpp_d<0xB1>(v));
    v = fmax(v, dpp_d<0x4E>(v));
    v = fmax(v, dpp_d<0x141>(v));
    return fmax(v, dpp_d<0x140>(v));
}
__device__ __forceinline__ double row16_min(double v) {
    v = fmin(v, dpp_d<0xB1>(v));
    v = fmin(v, dpp_d<0x4E>(v));
    v = fmin(v, dpp_d<0x141>(v));
    return fmin(v, dpp_d<0x140>(v));
}

// Combine the four row extremes of a wave (every lane holds its row's value) through
// scalar reads of lanes 0, 16, 32, 48: the wave's extreme, uniform in every lane.
__device__ __forceinline__ double rows_max(double v) {
    return fmax(fmax(readlane_f64(v, 0), readlane_f64(v, 16)),
                fmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}
__device__ __forceinline__ double rows_min(double v) {
    return fmin(fmin(readlane_f64(v, 0), readlane_f64(v, 16)),
                fmin(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// ---------------------------------------------------------------------------
// Whole sweeps for small p (the reference's published designs, p = 10, 13): the general
// path's four launches per sweep (S_alpha / X beta partials, tau and sig2, k_tri_update,
// X beta) cost more than the arithmetic.  k_tri_chain keeps the chain in LDS and runs
// `count` sweeps per launch: all 512 threads for S_alpha / rss, two lanes for tau and sig2,
// then wave 0 alone (lane j = coefficient j) for omega, u and the coordinate passes, whose
// bound reductions are DPP + readlane inside the wave (no barrier per coordinate) and whose
// truncated-normal draws test kTcK attempts at once (tnorm_par).  While wave 0 runs the
// serial part, waves 1..7 draw every counter-only variate of the NEXT sweep into the other
// half of a double buffer: the tau / sig2 gamma variates, the omega / u uniforms and
// attempts 0..kTcK-1 of each coordinate's first-pass truncated normal.  The arithmetic is
// k_tri_update's, expression for expression.
// ---------------------------------------------------------------------------
constexpr int kTcNT = 512;
constexpr int kTcK = 16;                // parallel truncated-normal attempts
constexpr size_t kTcXLds = 96 * 1024;  // X staged in LDS up to this size
constexpr int kTcP = kTriChainMaxP;

// The counter-only variates of one sweep, in a buffer of tc_nvar(P) doubles laid out for P
// coefficients (P = kTcP in the static buffers of the 512-thread instances, P = p in the
// compact instance's dynamic LDS):
//   [0] gt, [1] gs             Ga(tau shape, 1), Ga(sig2 shape, 1)
//   om(j, 0..2), uu(j)         omega: r0 and the Ga(1, 1) / Ga(2, 1) variates; u
//   r(i, k, 0..1), x(i, k)     attempt k of coordinate i (pass 0): r0, r1 and its Box-Muller normal
struct TcVariates {
    double *b;
    int P;
    __device__ __forceinline__ double &gt() const { return b[0]; }
    __device__ __forceinline__ double &gs() const { return b[1]; }
    __device__ __forceinline__ double &om(int j, int c) const { return b[2 + 3 * j + c]; }
    __device__ __forceinline__ double &uu(int j) const { return b[2 + 3 * P + j]; }
    __device__ __forceinline__ double &r(int i, int k, int c) const {
        return b[2 + 4 * P + (i * kTcK + k) * 2 + c];
    }
    __device__ __forceinline__ double &x(int i, int k) const {
        return b[2 + (4 + 2 * kTcK) * P + i * kTcK + k];
    }
};
__host__ __device__ constexpr int tc_nvar(int P) { return 2 + (4 + 3 * kTcK) * P; }

// Item e of sweep tt's variates (e < 2 + p (1 + kTcK)).  MH (alpha sampled): tau's gamma variate
// is drawn in the sweep, and item 0 is the two uniforms of the MH step instead (k_alpha_mh's
// counter: ua[0] proposes, ua[1] decides).
template <bool MH = false>
__device__ __forceinline__ void tc_variate(const TcVariates &v, int e, int p, double tau_shape,
                                           double sig2_shape, const Hyper &hy, Key key,
                                           uint64_t tt, uint32_t *err, double *ua = nullptr) {
    if (e == 0) {
        if constexpr (MH) {
            const U4 r = uniforms(key, tt, KIND_ALPHA, 0, 0, 0);
            ua[0] = r.r[0];
            ua[1] = r.r[1];
        } else if (!hy.know_tau) {
            v.gt() = gamma1(tau_shape, key, tt, KIND_TAU, err);
        }
    } else if (e == 1) {
        if (!hy.know_sig2) v.gs() = gamma1(sig2_shape, key, tt, KIND_SIG2, err);
    } else if (e < 2 + p) {
        const int j = e - 2;
        const U4 r = uniforms(key, tt, KIND_TRI_OMEGA, (uint64_t)j, 0, 0);
        v.om(j, 0) = r.r[0];
        v.om(j, 1) = -log(r.r[1]);                // Ga(1, 1)
        v.om(j, 2) = -log(r.r[1]) - log(r.r[2]);  // Ga(2, 1)
        v.uu(j) = uniforms(key, tt, KIND_TRI_U, (uint64_t)j, 0, 0).r[0];
    } else {
        const int q = e - 2 - p, i = q / kTcK, k = q % kTcK;
        const U4 r = uniforms(key, tt, KIND_TRI_Z, (uint64_t)i, 0, (uint64_t)k);
        v.r(i, k, 0) = r.r[0];
        v.r(i, k, 1) = r.r[1];
        v.x(i, k) = bm_normal(r.r[0], r.r[1]);
    }
}

// The whole sweep loop of one chain in one workgroup: k_tri_chain runs it once, k_tri_chains
// once per workgroup on that chain's state, so the arithmetic exists once.
// The sums and the tau / sig2 draws are bb_chain_steps.h's (chain_sums, chain_scalars).
// NT: real threads (64 | NT | kTcNT).  The only order-dependent arithmetic outside wave 0 is the
// S_alpha / rss reduction over kTcNT threads; a narrower workgroup keeps kTcNT VIRTUAL threads
// (chain_sums<NT, kTcNT>), so red[.][0..7] hold the same bits and are summed in the same order.
// The pre-drawn variates depend on their counters alone, so which thread draws them does not
// matter.
// COMPACT: the basis and the variate buffers live in the dynamic LDS behind X, sized by p
// instead of kTcP, so that several workgroups share a CU's LDS.
// LOST: a draw that can never be accepted gives up at once (tn_pos).
// MH: alpha is chain state (uniform over the workgroup in s_alpha), drawn by wave 0 after the
// sweep's last beta with k_alpha_mh's counters and functions (chain_alpha_step) under the prior
// (pr_a, pr_b).  tau's gamma variate, whose shape then moves with alpha, is drawn in the sweep
// by the thread that needs it and leaves the look-ahead; the two MH uniforms, which depend on
// their counter alone, take its place there (item 0, into s_ua).  The alpha step is wave 0's
// alone, so the narrower instances keep the 512-thread one's bits.
template <int NT, bool COMPACT, bool LOST, bool MH = false>
__device__ __forceinline__ void tri_chain_body(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ tVc, const double *__restrict__ tVr,
    const double *__restrict__ av, const double *__restrict__ dv, const double *__restrict__ Gf,
    const double *__restrict__ cv, int ortho, int x_lds, double *beta, double *u, double *omega,
    double *shape, DevScalars *sc, Hyper hy, int betaburn, Key key, uint64_t t0, int count,
    int first_slot, int slot_step, int cap, double *tr_beta, double *tr_u, double *tr_omega,
    double *tr_shape, double *tr_sig2, double *tr_tau, double *tr_alpha, uint32_t *err,
    double pr_a = 0.0, double pr_b = 0.0) {
    static_assert(NT % 64 == 0 && NT >= 128 && kTcNT % NT == 0, "NT divides kTcNT; wave 1 draws sig2");
    extern __shared__ double sX[];
    __shared__ double sT[COMPACT ? 1 : 2 * kTcP * kTcP];
    __shared__ double sV[COMPACT ? 1 : 2 * tc_nvar(kTcP)];
    __shared__ double sb[kTcP];
    __shared__ double red[2][kTcNT / 64];
    __shared__ double s_tau, s_sig2;
    // MH: alpha, log B(pr_a, pr_b), and the two uniforms of the proposal, double-buffered as the
    // variates are
    __shared__ double s_alpha, s_lbc, s_ua[2][2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // variate buffers laid out for VP coefficients; COMPACT: [X | sTc | sTr | vb0 | vb1]
    const int VP = COMPACT ? p : kTcP, TP = COMPACT ? p * p : kTcP * kTcP;
    double *const dyn = sX + (x_lds ? (size_t)n * p : 0);
    double *const sTc = COMPACT ? dyn : sT;
    double *const sTr = sTc + TP;
    double *const vbase = COMPACT ? dyn + 2 * TP : sV;
    auto vbuf = [&](int half) { return TcVariates{vbase + half * tc_nvar(VP), VP}; };
    // orthogonal design: sTc holds the full symmetric Gram X'X (row j contiguous) instead
    for (int e = tid; e < p * p; e += NT) {
        sTc[e] = ortho ? Gf[e] : tVc[e];
        if (!ortho) sTr[e] = tVr[e];
    }
    if (x_lds)
        for (int e = tid; e < n * p; e += NT) sX[e] = X[(size_t)(e % n) + (size_t)(e / n) * ldx];
    const double *Xs = x_lds ? sX : X;
    const int lds_x = x_lds ? n : ldx;
    const bool act = wid == 0 && lane < p;  // wave 0, lane j = coefficient / coordinate j
    double uj = 0.0, om = 0.0, sh = 0.0, aj_c = 0.0, dj_c = 0.0;
    if (tid < p) {
        sb[tid] = beta[tid];
        uj = u[tid];
        aj_c = ortho ? cv[tid] : av[tid];          // ortho: c_j = (X'y)_j
        dj_c = ortho ? Gf[(size_t)tid * p + tid] : dv[tid];  //        G_jj
    }
    if (tid == 0) {
        s_tau = sc->tau;
        s_sig2 = sc->sig2;
        if constexpr (MH) {
            s_alpha = sc->alpha;
            s_lbc = lgamma(pr_a) + lgamma(pr_b) - lgamma(pr_a + pr_b);
        }
    }
    const double alpha0 = sc->alpha;
    const double tau_shape = hy.nu_shape + ((double)p) / alpha0;
    const double sig2_shape = hy.sig2_shape + 0.5 * (double)n;
    const int nvar = 2 + p * (1 + kTcK);
    for (int e = tid; e < nvar; e += NT)  // sweep 0's variates
        tc_variate<MH>(vbuf(0), e, p, tau_shape, sig2_shape, hy, key, t0, err, s_ua[0]);
    __syncthreads();
    for (int k = 0; k < count; ++k) {
        const TcVariates v = vbuf(k & 1);
        const uint64_t t = t0 + (uint64_t)k;
        const int slot = first_slot < 0 ? -1 : (first_slot + k * slot_step) % cap;
        // MH: the alpha of the previous sweep's step (written before that sweep's last barrier)
        double alpha = alpha0;
        if constexpr (MH) alpha = s_alpha;
        chain_sums<NT, kTcNT>(Xs, lds_x, n, p, y, sb, alpha, red);
        __syncthreads();
        // MH: tau's shape moves with alpha, so its gamma variate is drawn here
        const auto tau_gamma = [&] {
            if constexpr (MH)
                return gamma1(hy.nu_shape + ((double)p) / alpha, key, t, KIND_TAU, err);
            else
                return v.gt();
        };
        chain_scalars<kTcNT, !MH>(red, hy, alpha, tau_gamma, &v.gs(), s_tau, s_sig2, slot, tr_tau,
                                  tr_sig2, tr_alpha);
        __syncthreads();
        if (wid > 0) {
            // the next sweep's variates, off wave 0's serial chain
            if (k + 1 < count)
                for (int e = tid - 64; e < nvar; e += NT - 64)
                    tc_variate<MH>(vbuf((k + 1) & 1), e, p, tau_shape, sig2_shape, hy, key, t + 1,
                                   err, s_ua[(k + 1) & 1]);
        } else {
            const double tau = s_tau, sig2 = s_sig2, sig = sqrt(sig2);
            double bj = 0.0;
            if (act) {
                // sample_omega, sample_u, the bound of sample_beta (BridgeRegression.cpp:97-146,
                // :410-412)
                const double betaj = sb[lane];
                const double aj = exp(alpha * log(fabs(betaj) / ((1.0 - uj) * tau)));
                const double prob = alpha / (1.0 + alpha * aj);
                double w;
                if (v.om(lane, 0) > prob) {
                    sh = 1.0;
                    w = v.om(lane, 1);
                } else {
                    sh = 2.0;
                    w = v.om(lane, 2);
                }
                om = w + aj;
                const double right = 1.0 - fabs(betaj) / tau * exp(-1.0 * log(om) / alpha);
                uj = right * v.uu(lane);
                bj = (1.0 - uj) * exp(log(om) / alpha) * tau;
                // A NaN bound (the chain's state is no longer finite) is no truncation
                // interval.  The orthogonal pass reports it (tnorm's flag 128); the general
                // pass would draw NaN after NaN from the flat branch below without a word,
                // so a batch reports it here, in the chain's own flag word.
                if (LOST && bj != bj) atomicOr(err, 128u);
                if (slot >= 0) {
                    tr_omega[(size_t)slot * p + lane] = om;
                    tr_shape[(size_t)slot * p + lane] = sh;
                    tr_u[(size_t)slot * p + lane] = uj;
                }
            }
            if (ortho) {
                // sample_beta_ortho (BridgeRegression.cpp:362-403), one coordinate pass as
                // k_tri_update's: m_j = (c_j - sum_{k != j} G_jk beta_k) / G_jj, sd
                // sqrt(sig2 / G_jj), truncated to |beta_j| <= b_j; attempts 0..kTcK-1 of
                // every coordinate precomputed by waves 1..7 during the previous sweep
                double bl = act ? sb[lane] : 0.0;
                for (int j = 0; j < p; ++j) {
                    const double prod = (act && lane != j) ? sTc[j * p + lane] * bl : 0.0;
                    const double xb = wave_sum_all(prod);  // xor tree: the same bits in every lane
                    const double gjj = readlane_f64(dj_c, j), bnd = readlane_f64(bj, j);
                    const double m = (readlane_f64(aj_c, j) - xb) / gjj;
                    const double sd = sqrt(sig2 / gjj);
                    const int ka = lane < kTcK ? lane : 0;
                    const double zn = tnorm_par<kTcK, LOST>(-1.0 * bnd, bnd, m, sd, v.r(j, ka, 0),
                                                            v.r(j, ka, 1), v.x(j, ka), key, t,
                                                            (uint64_t)j, 0, err);
                    if (lane == j) bl = zn;
                }
                if (act) {
                    sb[lane] = bl;
                    if (slot >= 0) tr_beta[(size_t)slot * p + lane] = bl;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            } else {
            // conditional mean a_i / d_i^2 and sd sigma / d_i of coordinate i (lane i)
            const bool ok = dj_c > 1e-16;
            const double ci = ok ? aj_c / (dj_c * dj_c) : 0.0;
            const double si = ok ? sig / dj_c : -1.0;
            double zr = 0.0;
            for (int it = 0; it <= betaburn; ++it) {
                Pre pr{0.0, 0.0, 0.0};  // attempt 0 of coordinate `lane` (passes >= 1)
                if (it > 0 && act) {
                    const U4 q = uniforms(key, t, KIND_TRI_Z, (uint64_t)lane, (uint64_t)it, 0);
                    pr = Pre{q.r[0], q.r[1], bm_normal(q.r[0], q.r[1])};
                }
                // z = tV beta (:246), then beta_cur = tV' z, in k_tri_update's order
                zr = 0.0;
                if (act)
                    for (int j = 0; j < p; ++j) zr += sTc[lane + j * p] * sb[j];
                double bc = 0.0;
                for (int kk = 0; kk < p; ++kk) {
                    const double zk = readlane_f64(zr, kk);
                    if (act) bc += sTr[kk * p + lane] * zk;
                }
                for (int i = 0; i < p; ++i) {  // :250-283
                    const double vi = act ? sTr[i * p + lane] : 0.0;
                    const double zi = readlane_f64(zr, i);
                    double lmax = -1.0 * 1.7976931348623157e308, rmin = 1.7976931348623157e308;
                    if (act) {
                        const double rji = bc - vi * zi;
                        const double dif = bj - rji, sum = bj + rji;
                        const double left = (vi > 0 ? -sum : -dif) / fabs(vi);
                        const double right = (vi > 0 ? dif : sum) / fabs(vi);
                        lmax = lmax > left ? lmax : left;
                        rmin = rmin < right ? rmin : right;
                    }
                    const double L = rows_max(row16_max(lmax));
                    const double R = rows_min(row16_min(rmin));
                    const double sdi = readlane_f64(si, i);
                    double zn;
                    if (it == 0) {
                        const int ka = lane < kTcK ? lane : 0;
                        if (sdi > 0.0)
                            zn = tnorm_par<kTcK, LOST>(L, R, readlane_f64(ci, i), sdi,
                                                       v.r(i, ka, 0), v.r(i, ka, 1), v.x(i, ka),
                                                       key, t, (uint64_t)i, 0, err);
                        else
                            zn = L + (R - L) * v.r(i, 0, 0);
                    } else {
                        const Pre pi{readlane_f64(pr.r0, i), readlane_f64(pr.r1, i),
                                     readlane_f64(pr.x0, i)};
                        if (sdi > 0.0)
                            zn = tnorm<LOST>(L, R, readlane_f64(ci, i), sdi, key, t, (uint64_t)i,
                                             (uint64_t)it, pi, err);
                        else
                            zn = L + (R - L) * pi.r0;
                    }
                    bc += vi * (zn - zi);
                    if (lane == i) zr = zn;
                }
                // beta = tV' z (:285)
                double bn = 0.0;
                for (int kk = 0; kk < p; ++kk) {
                    const double zk = readlane_f64(zr, kk);
                    if (act) bn += sTr[kk * p + lane] * zk;
                }
                if (act) sb[lane] = bn;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // sb read by other lanes next
            }
            if (act && slot >= 0) tr_beta[(size_t)slot * p + lane] = sb[lane];
            }
            // ---- alpha | beta, tau: the lanes of wave 0 hold the beta they just wrote ----
            if constexpr (MH)
                chain_alpha_step(p, sb, tau, alpha, s_ua[k & 1], pr_a, pr_b, s_lbc, s_alpha, slot,
                                 tr_alpha);
        }
        __syncthreads();
    }
    if (act) {
        beta[lane] = sb[lane];
        u[lane] = uj;
        omega[lane] = om;
        shape[lane] = sh;
    }
    if (tid == 0) {
        sc->tau = s_tau;
        sc->sig2 = s_sig2;
        if constexpr (MH) sc->alpha = s_alpha;
    }
}

}  // namespace

// dynamic LDS of a launch: X when it fits under kTcXLds, and for a compact instance the basis
// and the two variate buffers behind it, all sized by p
inline size_t tri_chain_shm(bool compact, int n, int p, int *x_lds) {
    const size_t xbytes = (size_t)n * p * sizeof(double);
    *x_lds = xbytes <= kTcXLds;
    const size_t extra = compact ? (2 * (size_t)p * p + 2 * tc_nvar(p)) * sizeof(double) : 0;
    return (*x_lds ? xbytes : 0) + extra;
}
// the most a launch asks for (X at kTcXLds, p = kTcP): a kernel's one-time opt-in above 64 KB
inline int tri_chain_shm_max(bool compact) {
    const size_t extra = compact ? (2 * kTcP * kTcP + 2 * tc_nvar(kTcP)) * sizeof(double) : 0;
    return (int)(kTcXLds + extra);
}

// bb_tri_mh.hip: the launch of `blocks` workgroups of the alpha-sampling instance of `threads`
// threads (the single chain's, batch == 0 and 512 threads, or the batch's), and that batch
// instance for occupancy queries (nullptr: none of that many threads); the launch returns -1 if
// there is no such instance
int tri_mh_launch(int batch, int threads, int blocks, hipStream_t s, const ChainDesign &d,
                   const ChainState &c, const ChainTraces &tr, const ChainRun &r);
const void *tri_mh_batch_kernel(int threads);

}  // namespace bb
