// bb_small_body.h -- the sweep loop of the fused small-p chain (bb_small.hip's header comment),
// shared by its two translation units: bb_small.hip (alpha known) and bb_small_mh.hip (alpha
// sampled).  They are two code objects, so that the out-of-line MH decision below is no part of
// the known-alpha kernels' code identity (bayesbridge_amd/_kernel_code.py).  The sweep's steps
// are bb_chain_steps.h's: the first (sums, tau and sig2, lambda, the orthogonal beta) shared
// with the wide and the triangle chains, the last (the factor and the MH step) with the logistic
// chain.  Here are the staging of X and G, the look-ahead, the entries of A, the order and
// barriers of the sweep, and two steps written out that restate bb_chain_steps.h's templates
// (entry ownership and the solves: called, they cost these kernels speed).
#pragma once
#include <hip/hip_runtime.h>

#include "bb_chain_steps.h"

namespace bb {

namespace {

constexpr size_t kSmallXLds = 112 * 1024;  // X staged in LDS up to this size
constexpr int kSmallPre = 32;  // sweeps of counter-only variates drawn ahead

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
    // upper-triangle entries of A owned by this thread (none: orthogonal design).  Written out:
    // chain_tri_owners<NT>(p, !ortho, own, oi, oj, av) restated (bb_chain_steps.h; called, the
    // packed instances ran 0.4-0.7 % slower)
    constexpr int H = kTriOwned<NT>;
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
            // A = G + diag(lambda sig2 / tau^2), an upper-triangle entry (i, j) per thread (two
            // for the last 16 at p = 32), factored as A = U'U; wave 0 solves for the mean and
            // the draw
            const double dl = tau * tau;
#pragma unroll
            for (int h = 0; h < H; ++h)
                if (own[h]) {
                    const int i = oi[h], j = oj[h];
                    av[h] = sG[i][j] + (i == j ? sl[i] * sig2 / dl : 0.0);
                }
            chain_factor(p, own, oi, oj, av, sU, err);
            if (wid == 0) {
                // written out: chain_solves(p, sU, sc_, s_z[kp], w, z) restated (called, the
                // single chains ran 0.5-1.4 % slower, the packed instances 1.1-1.3 %)
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
            if (wid == 0)
                chain_alpha_step(p, sb, tau, alpha, s_ua[kp], pr_a, pr_b, s_lbc, s_alpha, slot,
                                 tr_alpha);
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
