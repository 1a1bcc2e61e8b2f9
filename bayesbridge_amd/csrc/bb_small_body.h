// bb_small_body.h -- the sweep loop of the fused small-p chain (bb_small.hip's header comment),
// shared by its two translation units: bb_small.hip (alpha known) and bb_small_mh.hip (alpha
// sampled).  They are two code objects, so that the out-of-line MH decision below is no part of
// the known-alpha kernels' code identity (bayesbridge_amd/_kernel_code.py).  The sweep's first
// steps (sums, tau and sig2, lambda, the orthogonal beta) are bb_chain_steps.h's, shared with
// the wide and the triangle chains; the look-ahead, the factor and solves and the MH step are
// here.
#pragma once
#include <hip/hip_runtime.h>

#include "bb_chain_steps.h"

namespace bb {

namespace {

constexpr int kSmallMaxP = kSmallChainMaxP;
constexpr size_t kSmallXLds = 112 * 1024;  // X staged in LDS up to this size
constexpr int kSmallPre = 32;  // sweeps of counter-only variates drawn ahead

// alpha_mh_accept (bb_sampler.h) out of line: one thread's scalar work, whose registers are
// then not the sweep loop's (inlined, the MH instances spill 122-125 VGPRs and take 504-520 B
// of scratch per lane; so, 5-8 and 40-56).
[[maybe_unused]] __device__ __noinline__ double alpha_mh_decide(double a_old, double a_new, double d_new,
                                               double Sn, double So, double pp, double pr_a,
                                               double pr_b, double lbc, double u1) {
    return alpha_mh_accept(a_old, a_new, d_new, Sn, So, pp, pr_a, pr_b, lbc, u1);
}

}  // namespace

// bb_small.hip defines SMALL_PHASE when built with BB_SMALL_PHASES (its phase timing)
#ifndef SMALL_PHASE
#define SMALL_PHASE(i) \
    do {               \
    } while (0)
#endif

// L lanes per coefficient in the lambda draw (stable_spec_draw<L, I>).  Dynamic LDS holds X
// (n x p, column-major) when it fits, else X is read from HBM each sweep.
// small_chain_body is the whole sweep loop of one chain in one workgroup: k_small_chain runs
// it once, k_small_chains once per workgroup on that chain's state, so the arithmetic exists
// once.
// LOST: a chain whose state is no longer finite skips its lambda draws (k_small_chains).
// MH: alpha is chain state (uniform over the workgroup in s_alpha), drawn after beta with
// k_alpha_mh's counters and the same two functions (bb_sampler.h: alpha_propose,
// alpha_mh_accept) under the prior (pr_a, pr_b); tau's gamma variate, whose shape then moves
// with alpha, is drawn in the sweep.
template <int NT, int L, int I, bool LOST, bool MH = false>
__device__ __forceinline__ void small_chain_body(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, int x_lds, double *beta, double *lam,
    DevScalars *sc, Hyper hy, Key key, uint64_t t0, int count, int first_slot,
    int slot_step, int cap, double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau,
    double *tr_alpha, uint32_t *err, double pr_a = 0.0, double pr_b = 0.0) {
    extern __shared__ double sX[];
    __shared__ double sU[kSmallMaxP][kSmallMaxP + 1];  // U, row-major (U[k][j])
    __shared__ double sG[kSmallMaxP][kSmallMaxP + 1];
    __shared__ double sb[kSmallMaxP], sl[kSmallMaxP], sc_[kSmallMaxP], sgd[kSmallMaxP];
    // Ga(shape, 1) variates of tau and sig2 and the beta normals of the next kSmallPre
    // sweeps: their shapes are constant along the chain (alpha known), so they depend on
    // their counters alone and come off the serial chain
    __shared__ double s_gt[kSmallPre], s_gs[kSmallPre], s_z[kSmallPre][kSmallMaxP];
    __shared__ double red[2][NT / 64];
    __shared__ double s_tau, s_sig2;
    // MH: alpha, log B(pr_a, pr_b), and the two uniforms of each look-ahead sweep's proposal
    __shared__ double s_alpha, s_lbc, s_ua[MH ? kSmallPre : 1][2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int e = tid; e < p * p; e += NT) {
        const int r = e % p, c = e / p;
        const int lo = r < c ? r : c, hi = r < c ? c : r;  // G holds its upper triangle
        sG[r][c] = ortho ? 0.0 : G[(size_t)lo + (size_t)hi * ldg];
    }
    if (x_lds)
        for (int e = tid; e < n * p; e += NT) sX[e] = X[(size_t)(e % n) + (size_t)(e / n) * ldx];
    const double *Xs = x_lds ? sX : X;
    const int lds_x = x_lds ? n : ldx;
    if (tid < p) {
        sb[tid] = beta[tid];
        sc_[tid] = cvec[tid];
        sgd[tid] = ortho ? gdiag[tid] : 0.0;
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
#ifdef BB_SMALL_PHASES
    unsigned long long ph_t = 0;
#endif
    __syncthreads();
    const double tau_shape = hy.nu_shape + ((double)p) / alpha0;
    const double sig2_shape = hy.sig2_shape + 0.5 * (double)n;
    // upper-triangle entries owned by this thread: e = tid, tid + NT, ..., e = j (j + 1) / 2 + i
    // (two per thread at NT = 512, three at NT = 256)
    constexpr int H = (kSmallMaxP * (kSmallMaxP + 1) / 2 + NT - 1) / NT;
    bool own[H];
    int oi[H], oj[H];
    double av[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        av[h] = 0.0;
        const int e = tid + h * NT;
        own[h] = !ortho && e < p * (p + 1) / 2;
        int j = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
        while ((j + 1) * (j + 2) / 2 <= e) ++j;
        while (j * (j + 1) / 2 > e) --j;
        oj[h] = j;
        oi[h] = e - j * (j + 1) / 2;
    }
    for (int k = 0; k < count; ++k) {
        if (k % kSmallPre == 0) {
            // wave 0: tau's gamma variates, wave 1: sig2's, waves 2..: the normals
            const int nb = count - k < kSmallPre ? count - k : kSmallPre;
            if (MH && wid == 0 && lane < nb) {
                const U4 u = uniforms(key, t0 + (uint64_t)(k + lane), KIND_ALPHA, 0, 0, 0);
                s_ua[lane][0] = u.r[0];
                s_ua[lane][1] = u.r[1];
            } else if (!MH && wid == 0 && lane < nb && !hy.know_tau)
                s_gt[lane] = gamma1(tau_shape, key, t0 + (uint64_t)(k + lane), KIND_TAU, err);
            else if (wid == 1 && lane < nb && !hy.know_sig2)
                s_gs[lane] = gamma1(sig2_shape, key, t0 + (uint64_t)(k + lane), KIND_SIG2, err);
            for (int e = tid - 128; e >= 0 && e < nb * p; e += NT - 128) {
                const int kk = e / p, j = e % p;
                s_z[kk][j] = normal_at(key, t0 + (uint64_t)(k + kk), KIND_BETA_Z, (uint64_t)j);
            }
            __syncthreads();
        }
        const int kp = k % kSmallPre;
        SMALL_PHASE(0);
        const uint64_t t = t0 + (uint64_t)k;
        const int slot = first_slot < 0 ? -1 : (first_slot + k * slot_step) % cap;
        // MH: the alpha of the previous sweep's step (written before that sweep's last barrier)
        double alpha = alpha0;
        if constexpr (MH) alpha = s_alpha;
        chain_sums<NT, NT>(Xs, lds_x, n, p, y, sb, alpha, red);
        __syncthreads();
        SMALL_PHASE(1);
        // MH: tau's shape moves with alpha, so its gamma variate is drawn here
        const auto tau_gamma = [&] {
            if constexpr (MH)
                return gamma1(hy.nu_shape + ((double)p) / alpha, key, t, KIND_TAU, err);
            else
                return s_gt[kp];
        };
        chain_scalars<NT, !MH>(red, hy, alpha, tau_gamma, &s_gs[kp], s_tau, s_sig2, slot, tr_tau,
                               tr_sig2, tr_alpha);
        __syncthreads();
        SMALL_PHASE(2);
        const double tau = s_tau, sig2 = s_sig2;
        chain_lambda<NT, L, I, LOST>(p, sb, sl, tau, alpha, key, t, slot, tr_lam, err);
        __syncthreads();
        SMALL_PHASE(3);
        // ---- beta | rest ----
        if (ortho) {
            chain_beta_ortho(p, sb, sc_, sgd, sl, s_z[kp], tau, sig2);
        } else {
            // A = G + diag(lambda sig2 / tau^2), factored right-looking as A = U'U with one
            // thread per upper-triangle entry (i, j) (two for the last 16 at p = 32): per
            // pivot k the owner of (k, k) takes the square root, the owners of row k divide
            // (row k of U goes to LDS), every trailing owner subtracts U(k, i) U(k, j) -- the
            // reference's operations entry by entry (BridgeRegression.cpp:560), two barriers
            // per pivot and no register arrays.  (One barrier per pivot -- trailing owners
            // subtracting a_ki a_kj / a_kk from a published unscaled row, one reciprocal square
            // root per pivot -- measured the same at C1 in three alternations, 27 176-27 186
            // against 27 152-27 188 sweeps/s, gpurun_out/r04q_*: the factor is not what bounds
            // the chain.)
            const double dl = tau * tau;
#pragma unroll
            for (int h = 0; h < H; ++h)
                if (own[h]) {
                    const int i = oi[h], j = oj[h];
                    av[h] = sG[i][j] + (i == j ? sl[i] * sig2 / dl : 0.0);
                }
            for (int kk = 0; kk < p; ++kk) {
#pragma unroll
                for (int h = 0; h < H; ++h)
                    if (own[h] && oi[h] == kk && oj[h] == kk) {
                        if (!(av[h] > 0.0)) atomicOr(err, 8u);
                        av[h] = sqrt(av[h]);
                        sU[kk][kk] = av[h];
                    }
                __syncthreads();
                const double d = sU[kk][kk];
#pragma unroll
                for (int h = 0; h < H; ++h)
                    if (own[h] && oi[h] == kk && oj[h] > kk) {
                        av[h] = av[h] / d;
                        sU[kk][oj[h]] = av[h];
                    }
                __syncthreads();
#pragma unroll
                for (int h = 0; h < H; ++h)
                    if (own[h] && oi[h] > kk) av[h] -= sU[kk][oi[h]] * sU[kk][oj[h]];
            }
            if (wid == 0) {
                // m: U'v = c (forward), U m = v (backward); x: U x = z; lane j holds entry j
                double w = lane < p ? sc_[lane] : 0.0;
                double z = lane < p ? s_z[kp][lane] : 0.0;
                for (int kk = 0; kk < p; ++kk) {
                    const double vk = readlane_f64(w, kk) / sU[kk][kk];
                    if (lane > kk && lane < p) w -= sU[kk][lane] * vk;
                    if (lane == kk) w = vk;
                }
                for (int kk = p - 1; kk >= 0; --kk) {
                    const double ukk = sU[kk][kk];
                    const double mk = readlane_f64(w, kk) / ukk;
                    const double xk = readlane_f64(z, kk) / ukk;
                    if (lane < kk) {
                        const double ulk = sU[lane][kk];
                        w -= ulk * mk;
                        z -= ulk * xk;
                    }
                    if (lane == kk) {
                        w = mk;
                        z = xk;
                    }
                }
                if (lane < p) sb[lane] = w + sqrt(sig2) * z;
            }
        }
        if constexpr (MH) {
            // ---- alpha | beta, tau: the lanes of wave 0 hold the beta they just wrote ----
            if (wid == 0) {
                const double a_old = alpha;
                double d_new;
                const double a_new = alpha_propose(a_old, s_ua[kp][0], d_new);
                double sn = 0.0, so = 0.0;
                if (lane < p) {
                    const double si = log(fabs(sb[lane] / tau));
                    sn = exp(a_new * si);
                    so = exp(a_old * si);
                }
                sn = wave_sum_all(sn);
                so = wave_sum_all(so);
                if (lane == 0) {
                    const double an = alpha_mh_decide(a_old, a_new, d_new, sn, so, (double)p, pr_a,
                                                      pr_b, s_lbc, s_ua[kp][1]);
                    s_alpha = an;
                    if (slot >= 0) tr_alpha[slot] = an;
                }
            }
        }
        __syncthreads();
        SMALL_PHASE(4);
        if (slot >= 0 && tid < p) tr_beta[(size_t)slot * p + tid] = sb[tid];
    }
    if (tid < p) {
        beta[tid] = sb[tid];
        lam[tid] = sl[tid];
    }
    if (tid == 0) {
        sc->tau = s_tau;
        sc->sig2 = s_sig2;
        if constexpr (MH) sc->alpha = s_alpha;
    }
}

// dynamic LDS of a launch: X when it fits, and no more than X needs -- a CU holds as many
// chains as its 160 KB allow
inline size_t small_chain_shm(int n, int p, int *x_lds) {
    const size_t xbytes = (size_t)n * p * sizeof(double);
    *x_lds = xbytes <= kSmallXLds;
    return *x_lds ? xbytes : 0;
}

// bb_small_mh.hip: the launch of `blocks` workgroups of the alpha-sampling instance for d.p (the
// single chain's or the batch's; 512 threads), and that batch instance for occupancy queries
void small_mh_launch(int batch, int blocks, size_t shm, int x_lds, hipStream_t s,
                     const ChainDesign &d, const ChainState &c, const ChainTraces &tr,
                     const ChainRun &r);
const void *small_mh_batch_kernel(int p);

}  // namespace bb
