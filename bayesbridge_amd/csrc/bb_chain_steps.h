// bb_chain_steps.h -- the steps the fused chain sweeps share, written once (gfx950).
//
// small_chain_body (bb_small_body.h), wide_chain_body (bb_wide.hip) and tri_chain_body
// (bb_tri.hip) run one chain in one workgroup, in the reference's order
// (Code/C/BridgeWrapper.cpp:266-298).  Their first steps are the same arithmetic:
//   chain_sums        S_alpha = sum |beta_j|^alpha and rss = |y - X beta|^2, per wave, into red
//   chain_scalars     tau | beta and sig2 | beta      BridgeRegression.cpp:453-465, :436-450
//   chain_lambda      lambda | beta, tau              :506-510 (stable mixture: small, wide)
//   chain_beta_ortho  beta | rest, orthogonal design  :514-521 (small, wide)
// small_chain_body and k_logit_chains (bb_logit_chain.hip) factor a system of p <= kSmallMaxP
// entry by entry and end their sweeps with the same steps:
//   chain_tri_owners  the upper-triangle entries a thread owns
//   chain_factor      A = U'U, right-looking            :560
//   chain_solves      U'v = c, U m = v, U x = z in wave 0
//   chain_alpha_step  alpha | beta, tau in wave 0 (the instances that sample alpha)
// The bodies keep what differs: the staging of X and G, the look-ahead of counter-only
// variates, how A is formed, the wide and triangle factorisations and solves, the triangle's
// wave-0 update.
// All are force-inlined into the caller's sweep loop and hold no LDS declaration; but for
// chain_factor's two barriers per pivot they hold no barrier either: the barriers between the
// steps stay in the body, where the LDS they order is declared.
#pragma once
#include <hip/hip_runtime.h>

#include "bb_kernels.h"
#include "bb_sampler.h"
#include "bb_wave.h"

namespace bb {

// The two sums over VT virtual threads, of which this workgroup has NT real ones: real thread
// tid accumulates one separate partial for each virtual thread tid + q NT (q < VT / NT), so a
// virtual wave lies in one real wave at the same lanes, its xor tree gives the same bits and
// lands in red[.][wid + q NT / 64]: red is the same for every NT that divides VT.  S_alpha's
// terms (p <= NT) lie in the virtual threads q = 0; the others' sums are +0.
template <int NT, int VT>
__device__ __forceinline__ void chain_sums(const double *Xs, int lds_x, int n, int p,
                                           const double *__restrict__ y, const double *sb,
                                           double alpha, double (&red)[2][VT / 64]) {
    static_assert(NT % 64 == 0 && VT % NT == 0, "whole waves; NT divides VT");
    constexpr int Q = VT / NT;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double sa = 0.0, rs[Q];
    if (tid < p) sa = exp(alpha * log(fabs(sb[tid])));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        rs[q] = 0.0;
        for (int i = tid + q * NT; i < n; i += VT) {
            double xb = 0.0;
            for (int j = 0; j < p; ++j) xb += Xs[(size_t)i + (size_t)j * lds_x] * sb[j];
            const double r = y[i] - xb;
            rs[q] += r * r;
        }
    }
    sa = wave_sum_all(sa);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        rs[q] = wave_sum_all(rs[q]);
        if (lane == 0) {
            red[0][wid + q * (NT / 64)] = q == 0 ? sa : 0.0;
            red[1][wid + q * (NT / 64)] = rs[q];
        }
    }
}

// tau (thread 0) and sig2 (thread 64) are independent draws from red's sums, added in wave
// order; each writes its trace slot (slot < 0: none).  tau's Ga(shape, 1) variate comes from
// tau_gamma(), called only where it is needed (a look-ahead buffer's entry, or the draw itself
// when the shape moves with a sampled alpha); sig2's is read through its pointer inside the
// branch.  TR_ALPHA: the sweep's alpha is traced here (a body that samples it writes it later).
template <int VT, bool TR_ALPHA, class TauGamma>
__device__ __forceinline__ void chain_scalars(const double (&red)[2][VT / 64], const Hyper &hy,
                                              double alpha, TauGamma tau_gamma,
                                              const double *sig2_gamma, double &s_tau,
                                              double &s_sig2, int slot, double *tr_tau,
                                              double *tr_sig2, double *tr_alpha) {
    const int tid = threadIdx.x;
    if (tid == 0 || tid == 64) {
        double S = red[tid == 0 ? 0 : 1][0];
#pragma unroll
        for (int w = 1; w < VT / 64; ++w) S += red[tid == 0 ? 0 : 1][w];
        if (tid == 0) {
            if (!hy.know_tau) {
                const double nu = tau_gamma() / (hy.nu_rate + S);
                s_tau = exp(-1.0 * log(nu) / alpha);
            }
            if (slot >= 0) {
                tr_tau[slot] = s_tau;
                if constexpr (TR_ALPHA) tr_alpha[slot] = alpha;
            }
        } else {
            if (!hy.know_sig2) s_sig2 = (hy.sig2_scale + 0.5 * S) / *sig2_gamma;
            if (slot >= 0) tr_sig2[slot] = s_sig2;
        }
    }
}

// lambda_j = 2 retstable(beta_j^2 / tau^2, alpha / 2, 1), L lanes per coefficient
// (stable_spec_draw<L, I>), NT / L coefficients a pass; into sl and the trace slot.
template <int NT, int L, int I, bool LOST>
__device__ __forceinline__ void chain_lambda(int p, const double *sb, double *sl, double tau,
                                             double alpha, Key key, uint64_t t, int slot,
                                             double *tr_lam, uint32_t *err) {
    const int tid = threadIdx.x;
    for (int jb = 0; jb < p; jb += NT / L) {
        const int j = jb + tid / L;
        const bool act = j < p;
        const double b = act ? sb[j] : 0.0;
        // A NaN tilt (the chain's state is no longer finite) fails every test of the
        // rejection sampler, which then gives up after BB_MAX_STABLE_ROUNDS rounds --
        // seconds per sweep -- with error bit 2 and a NaN draw.  A batch takes that outcome
        // at once (LOST): a lost chain must not hold a CU that other chains wait for.
        const double h = b * b / (tau * tau);
        const bool lost = LOST && act && h != h;
        double x = stable_spec_draw<L, I>(act && !lost, h, 0.5 * alpha, 1.0, key, t, (uint64_t)j,
                                          err);
        if (lost) {
            x = __builtin_nan("");
            if ((tid % L) == 0) atomicOr(err, 2u);
        }
        if (act && (tid % L) == 0) {
            sl[j] = 2 * x;
            if (slot >= 0) tr_lam[(size_t)slot * p + j] = 2 * x;
        }
    }
}

// beta | rest of an orthogonal design (BridgeRegression.cpp:514-521), thread j coefficient j:
// gd = diag(X'X), c = X'y, z the sweep's normals.
__device__ __forceinline__ void chain_beta_ortho(int p, double *sb, const double *c,
                                                 const double *gd, const double *sl,
                                                 const double *z, double tau, double sig2) {
    const int tid = threadIdx.x;
    if (tid < p) {
        const double uu = gd[tid] + sl[tid] * sig2 / (tau * tau);
        const double sd = sqrt(sig2 / uu);
        const double m = c[tid] / uu;
        sb[tid] = m + sd * z[tid];
    }
}

namespace {

constexpr int kSmallMaxP = kSmallChainMaxP;

// alpha_mh_accept (bb_sampler.h) out of line: one thread's scalar work, whose registers are
// then not the sweep loop's (inlined, the MH instances spill 122-125 VGPRs and take 504-520 B
// of scratch per lane; so, 5-8 and 40-56).  Internal linkage: a code object that does not call
// it does not hold it, and keeps its kernels' identity (bayesbridge_amd/_kernel_code.py).
[[maybe_unused]] __device__ __noinline__ double alpha_mh_decide(double a_old, double a_new, double d_new,
                                               double Sn, double So, double pp, double pr_a,
                                               double pr_b, double lbc, double u1) {
    return alpha_mh_accept(a_old, a_new, d_new, Sn, So, pp, pr_a, pr_b, lbc, u1);
}

}  // namespace

// Upper-triangle entries of a kSmallMaxP system that a thread of NT owns (two at NT = 512,
// three at NT = 256).
template <int NT>
constexpr int kTriOwned = (kSmallMaxP * (kSmallMaxP + 1) / 2 + NT - 1) / NT;

// The entries owned by this thread: e = tid, tid + NT, ..., e = j (j + 1) / 2 + i -> (oi, oj) =
// (i, j), owned where `on` and e lies in the triangle of p; av, the entries' values, zeroed.
template <int NT, int H>
__device__ __forceinline__ void chain_tri_owners(int p, bool on, bool (&own)[H], int (&oi)[H],
                                                 int (&oj)[H], double (&av)[H]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        av[h] = 0.0;
        const int e = tid + h * NT;
        own[h] = on && e < p * (p + 1) / 2;
        int j = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
        while ((j + 1) * (j + 2) / 2 <= e) ++j;
        while (j * (j + 1) / 2 > e) --j;
        oj[h] = j;
        oi[h] = e - j * (j + 1) / 2;
    }
}

// A (its upper triangle in the owners' av) factored right-looking as A = U'U with one thread
// per entry (i, j): per pivot k the owner of (k, k) takes the square root, the owners of row k
// divide (row k of U goes to LDS, sU row-major), every trailing owner subtracts U(k, i) U(k, j)
// -- the reference's operations entry by entry (BridgeRegression.cpp:560), two barriers per
// pivot, which every thread of the workgroup reaches, and no register arrays.  A pivot that is
// not positive sets error bit 8.  (One barrier per pivot -- trailing owners subtracting
// a_ki a_kj / a_kk from a published unscaled row, one reciprocal square root per pivot --
// measured the same at C1 in three alternations, 27 176-27 186 against 27 152-27 188 sweeps/s:
// the factor is not what bounds the chain.)
template <int H>
__device__ __forceinline__ void chain_factor(int p, const bool (&own)[H], const int (&oi)[H],
                                             const int (&oj)[H], double (&av)[H],
                                             double (*sU)[kSmallMaxP + 1], uint32_t *err) {
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
}

// Wave 0, lane j holding entry j: w = m with U'v = c (forward), U m = v (backward), and z = x
// with U x = z_in.  The caller forms beta = m + (its scale) x.
__device__ __forceinline__ void chain_solves(int p, double (*sU)[kSmallMaxP + 1],
                                             const double *c, const double *z_in, double &w,
                                             double &z) {
    const int lane = threadIdx.x & 63;
    w = lane < p ? c[lane] : 0.0;
    z = lane < p ? z_in[lane] : 0.0;
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
}

// alpha | beta, tau in wave 0, whose lanes hold the beta they just wrote to sb: the proposal
// from ua[0], the two sums over the coefficients, the decision on lane 0 (out of line) from
// ua[1] under the prior (pr_a, pr_b), lbc = log B(pr_a, pr_b); into s_alpha and the trace slot.
__device__ __forceinline__ void chain_alpha_step(int p, const double *sb, double tau,
                                                 double alpha, const double (&ua)[2], double pr_a,
                                                 double pr_b, const double &lbc, double &s_alpha,
                                                 int slot, double *tr_alpha) {
    const int lane = threadIdx.x & 63;
    const double a_old = alpha;
    double d_new;
    const double a_new = alpha_propose(a_old, ua[0], d_new);
    double sn = 0.0, so = 0.0;
    if (lane < p) {
        const double si = log(fabs(sb[lane] / tau));
        sn = exp(a_new * si);
        so = exp(a_old * si);
    }
    sn = wave_sum_all(sn);
    so = wave_sum_all(so);
    if (lane == 0) {
        const double an =
            alpha_mh_decide(a_old, a_new, d_new, sn, so, (double)p, pr_a, pr_b, lbc, ua[1]);
        s_alpha = an;
        if (slot >= 0) tr_alpha[slot] = an;
    }
}

}  // namespace bb
