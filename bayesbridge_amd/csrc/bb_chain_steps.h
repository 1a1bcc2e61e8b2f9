// bb_chain_steps.h -- the steps every fused chain sweep opens with, written once (gfx950).
//
// small_chain_body (bb_small_body.h), wide_chain_body (bb_wide.hip) and tri_chain_body
// (bb_tri.hip) run one chain in one workgroup, in the reference's order
// (Code/C/BridgeWrapper.cpp:266-298).  Their first steps are the same arithmetic:
//   chain_sums        S_alpha = sum |beta_j|^alpha and rss = |y - X beta|^2, per wave, into red
//   chain_scalars     tau | beta and sig2 | beta      BridgeRegression.cpp:453-465, :436-450
//   chain_lambda      lambda | beta, tau              :506-510 (stable mixture: small, wide)
//   chain_beta_ortho  beta | rest, orthogonal design  :514-521 (small, wide)
// The bodies keep what differs: the staging of X and G, the look-ahead of counter-only
// variates, the factorisations and solves, the triangle's wave-0 update and the alpha step.
// All are force-inlined into the caller's sweep loop and hold no barrier: the barriers between
// the steps stay in the body, where the LDS they order is declared.
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

}  // namespace bb
