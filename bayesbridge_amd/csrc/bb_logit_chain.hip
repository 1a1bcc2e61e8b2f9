// bb_logit_chain.hip -- K independent logistic-bridge chains of a small design in one launch,
// a workgroup per chain (gfx950).
//
// The general logistic path (bb_engine.cpp, method 6) is built for n = 10 000, p = 1000: at a
// few hundred rows and tens of columns its launches are nearly empty.  k_logit_chains runs
// `count` whole sweeps of chain c = blockIdx.x under the key (k0, k1 + c), in the oracle's
// order (oracle/gibbs.py logit_sweep) and on the general path's counters:
//   psi = X beta, S_alpha = sum |beta_j|^alpha        one pass over X (beta is the same for both)
//   tau | beta                                         chain_scalars' tau branch; sig2 == 1
//   lambda | beta, tau                                 chain_lambda
//   omega_i ~ PG(1, psi_i)                             pg::pg1, a row per thread
//   A = X' Omega X + diag(lambda / tau^2)              an upper-triangle entry per thread
//   beta | rest                                        A = U'U, U'v = c, U m = v, U x = z
//   alpha | beta, tau (MH instances)                   alpha_propose, alpha_mh_accept
// Omega changes every sweep, so the p x p system is formed in the workgroup every sweep: the
// thread that owns entry (i, j) of the factorisation sums x_ri omega_r x_rj over the rows r in
// ascending order into four interleaved partial sums (r mod 4), added as (s0 + s1) + (s2 + s3).
// The sum is one thread's own: no atomics, and its order depends on n alone, not on K or on
// how many workgroups share a CU.
//
// Dynamic LDS: omega (psi before it; n doubles), then X when it fits beside it, ROW-major with
// an odd stride ldp = p | 1.  The threads of a wave read different columns of one row in the
// Gram sum and one column of different rows in the psi pass; with the odd row stride both are
// free of bank conflicts, which the design's own column-major layout (stride n) is not.  An X
// that does not fit stays in memory: the psi pass reads it in place (a row per thread,
// coalesced), and the Gram sum stages it through the same LDS region in chunks of `rows_lds`
// rows (a multiple of 4, so the four interleaved partial sums take the same rows in the same
// order as over a resident X).
//
// The entry ownership, the factor, the solves and the alpha step are bb_chain_steps.h's, shared
// with small_chain_body (bb_small_body.h, whose look-ahead depth and LDS budget this file takes
// too); sig2 = 1.
#include <hip/hip_runtime.h>

#include "bb_pg.h"
#include "bb_small_body.h"

namespace bb {

namespace {

// Dynamic LDS of a launch: omega, and X beside it (padded to the odd stride) when both fit
// small_chain_shm's budget -- *rows_lds = n -- else as many rows of X as the budget holds, a
// multiple of 4 (at least 224 at p = 32, n = kLogitChainMaxN).
inline size_t logit_chain_shm(int n, int p, int *rows_lds) {
    const size_t om = (size_t)n * sizeof(double);
    const size_t row = (size_t)(p | 1) * sizeof(double);
    const size_t fit = (kSmallXLds - om) / row;
    *rows_lds = fit >= (size_t)n ? n : (int)(fit & ~(size_t)3);
    return om + (size_t)*rows_lds * row;
}

// omega ~ PG(1, psi).  (Out of line it costs more: the call keeps the sweep's live values in
// scratch, 472-504 B per lane against 232-264 inlined.)  A
// non-finite psi is a lost chain (bb_chain_steps.h, chain_lambda): pg1 on a NaN would walk its
// whole attempt budget while other chains wait for this CU, so it gives NaN and error bit 32 at
// once.
__device__ __forceinline__ double logit_pg_draw(double psi, Key key, uint64_t t, uint64_t i,
                                                uint32_t *err) {
    if (!(fabs(psi) <= 1.7976931348623157e308)) {
        atomicOr(err, 32u);
        return __builtin_nan("");
    }
    bool fail = false;
    const double w = pg::pg1(psi, key, t, i, &fail);
    if (fail) atomicOr(err, 32u);
    return w;
}

}  // namespace

// L, I: lanes per coefficient of the lambda draw (chain_lambda).  MH: alpha is chain state,
// drawn after beta under the prior (pr_a, pr_b); tau's gamma variate is then drawn in the sweep.
// omega_out: the chain's omega of the last sweep (n doubles), for bb_chains_get_omega.
template <int NT, int L, int I, bool MH>
__global__ __launch_bounds__(NT, 2) void k_logit_chains(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ cvec,
    int rows_lds, double *beta_, double *lam_, DevScalars *sc_all, Hyper hy, Key key0, uint64_t t0,
    int count, int first_slot, int slot_step, int cap, double *tr_beta_, double *tr_lam_,
    double *tr_sig2_, double *tr_tau_, double *tr_alpha_, uint32_t *err_, double *omega_out_,
    double pr_a, double pr_b) {
    extern __shared__ double s_dyn[];
    __shared__ double sU[kSmallMaxP][kSmallMaxP + 1];  // U, row-major (U[k][j])
    __shared__ double sb[kSmallMaxP], sl[kSmallMaxP], sc_[kSmallMaxP];
    __shared__ double s_gt[kSmallPre], s_z[kSmallPre][kSmallMaxP];
    __shared__ double red[2][1];
    __shared__ double s_tau, s_sig2;
    __shared__ double s_alpha, s_lbc, s_ua[MH ? kSmallPre : 1][2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const size_t c = blockIdx.x;
    const Key key{key0.k0, key0.k1 + (uint64_t)c};
    const size_t ring = c * (size_t)cap;
    double *beta = beta_ + c * p, *lam = lam_ + c * p;
    DevScalars *sc = sc_all + c;
    uint32_t *err = err_ + c;
    double *tr_beta = tr_beta_ + ring * p, *tr_lam = tr_lam_ + ring * p;
    double *tr_sig2 = tr_sig2_ + ring, *tr_tau = tr_tau_ + ring, *tr_alpha = tr_alpha_ + ring;

    double *s_om = s_dyn;    // psi, then omega
    double *sX = s_dyn + n;  // X, row-major with stride ldp
    const int ldp = p | 1;
    const bool x_lds = rows_lds >= n;
    if (x_lds)
        for (int e = tid; e < n * p; e += NT) {
            const int r = e % n, j = e / n;
            sX[(size_t)r * ldp + j] = X[(size_t)r + (size_t)j * ldx];
        }
    // element (r, j) of the design at Xs[r xr + j xc] for the psi pass; the index stays below
    // (n + 511) p < 2^18, and 32-bit index arithmetic halves what the sweep loop spills
    const double *Xs = x_lds ? sX : X;
    const int xr = x_lds ? ldp : 1, xc = x_lds ? 1 : ldx;
    if (tid < p) {
        sb[tid] = beta[tid];
        sl[tid] = lam[tid];
        sc_[tid] = cvec[tid];
    }
    if (tid == 0) {
        s_tau = sc->tau;
        s_sig2 = sc->sig2;
        red[1][0] = 0.0;
        if constexpr (MH) {
            s_alpha = sc->alpha;
            s_lbc = lgamma(pr_a) + lgamma(pr_b) - lgamma(pr_a + pr_b);
        }
    }
    const double alpha0 = sc->alpha;
    __syncthreads();
    const double tau_shape = hy.nu_shape + ((double)p) / alpha0;
    // upper-triangle entries of A owned by this thread
    constexpr int H = kTriOwned<NT>;
    bool own[H];
    int oi[H], oj[H];
    double av[H];
    chain_tri_owners<NT>(p, true, own, oi, oj, av);
    for (int k = 0; k < count; ++k) {
        if (k % kSmallPre == 0) {
            // the counter-only variates of the next kSmallPre sweeps: wave 0 tau's gamma
            // variates (alpha known) or the MH uniforms, the other waves the normals
            const int nb = count - k < kSmallPre ? count - k : kSmallPre;
            if (MH && wid == 0 && lane < nb) {
                const U4 u = uniforms(key, t0 + (uint64_t)(k + lane), KIND_ALPHA, 0, 0, 0);
                s_ua[lane][0] = u.r[0];
                s_ua[lane][1] = u.r[1];
            } else if (!MH && wid == 0 && lane < nb && !hy.know_tau)
                s_gt[lane] = gamma1(tau_shape, key, t0 + (uint64_t)(k + lane), KIND_TAU, err);
            for (int e = tid - 64; e >= 0 && e < nb * p; e += NT - 64) {
                const int kk = e / p, j = e % p;
                s_z[kk][j] = normal_at(key, t0 + (uint64_t)(k + kk), KIND_BETA_Z, (uint64_t)j);
            }
            __syncthreads();
        }
        const int kp = k % kSmallPre;
        const uint64_t t = t0 + (uint64_t)k;
        const int slot = first_slot < 0 ? -1 : (first_slot + k * slot_step) % cap;
        double alpha = alpha0;
        if constexpr (MH) alpha = s_alpha;
        // ---- psi = X beta (a row per thread) and S_alpha (wave 0, chain_sums' tree) ----
        for (int i = tid; i < n; i += NT) {
            double xb = 0.0;
            for (int j = 0; j < p; ++j) xb += Xs[i * xr + j * xc] * sb[j];
            s_om[i] = xb;
        }
        if (wid == 0) {
            double sa = 0.0;
            if (lane < p) sa = exp(alpha * log(fabs(sb[lane])));
            sa = wave_sum_all(sa);
            if (lane == 0) red[0][0] = sa;
        }
        __syncthreads();
        // ---- tau | beta; the sig2 slot of the trace is the constant 1 ----
        const auto tau_gamma = [&] {
            if constexpr (MH)
                return gamma1(hy.nu_shape + ((double)p) / alpha, key, t, KIND_TAU, err);
            else
                return s_gt[kp];
        };
        chain_scalars<64, !MH>(red, hy, alpha, tau_gamma, &s_sig2, s_tau, s_sig2, slot, tr_tau,
                               tr_sig2, tr_alpha);
        __syncthreads();
        const double tau = s_tau;
        // ---- lambda | beta, tau, then omega | beta with no barrier between: the waves the
        // lambda draw leaves idle start on their rows at once ----
        chain_lambda<NT, L, I, true>(p, sb, sl, tau, alpha, key, t, slot, tr_lam, err);
        for (int i = tid; i < n; i += NT)
            s_om[i] = logit_pg_draw(s_om[i], key, t, (uint64_t)i, err);
        __syncthreads();
        // ---- A = X' Omega X + diag(lambda / tau^2): each owner sums its entry over the rows
        // in ascending order, four interleaved partial sums ----
        {
            double acc[H][4];
#pragma unroll
            for (int h = 0; h < H; ++h)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[h][q] = 0.0;
            for (int r0 = 0; r0 < n; r0 += rows_lds) {
                const int rc = n - r0 < rows_lds ? n - r0 : rows_lds;
                if (!x_lds) {  // stage rows r0 .. r0 + rc (uniform over the workgroup)
                    __syncthreads();
                    for (int e = tid; e < rc * p; e += NT) {
                        const int r = e % rc, j = e / rc;
                        sX[r * ldp + j] = X[(size_t)(r0 + r) + (size_t)j * ldx];
                    }
                    __syncthreads();
                }
                const double *om = s_om + r0;
                const int rc4 = rc & ~3;  // rc is a multiple of 4 in every chunk but the last
                for (int r = 0; r < rc4; r += 4) {
#pragma unroll
                    for (int h = 0; h < H; ++h)
                        if (own[h]) {
                            const double *xi = sX + r * ldp + oi[h];
                            const double *xj = sX + r * ldp + oj[h];
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                acc[h][q] += (xi[q * ldp] * om[r + q]) * xj[q * ldp];
                        }
                }
#pragma unroll
                for (int q = 0; q < 3; ++q) {  // the last n mod 4 rows
                    const int r = rc4 + q;
#pragma unroll
                    for (int h = 0; h < H; ++h)
                        if (own[h] && r < rc)
                            acc[h][q] += (sX[r * ldp + oi[h]] * om[r]) * sX[r * ldp + oj[h]];
                }
            }
            const double dl = tau * tau;
#pragma unroll
            for (int h = 0; h < H; ++h)
                if (own[h]) {
                    const double g = (acc[h][0] + acc[h][1]) + (acc[h][2] + acc[h][3]);
                    av[h] = g + (oi[h] == oj[h] ? sl[oi[h]] / dl : 0.0);
                }
        }
        // ---- beta | rest: A = U'U, then wave 0's solves; sig2 = 1 ----
        chain_factor(p, own, oi, oj, av, sU, err);
        if (wid == 0) {
            double w, z;
            chain_solves(p, sU, sc_, s_z[kp], w, z);
            if (lane < p) sb[lane] = w + z;
            // ---- alpha | beta, tau: the lanes of wave 0 hold the beta they just wrote ----
            if constexpr (MH)
                chain_alpha_step(p, sb, tau, alpha, s_ua[kp], pr_a, pr_b, s_lbc, s_alpha, slot,
                                 tr_alpha);
        }
        __syncthreads();
        if (slot >= 0 && tid < p) tr_beta[(size_t)slot * p + tid] = sb[tid];
    }
    if (tid < p) {
        beta[tid] = sb[tid];
        lam[tid] = sl[tid];
    }
    if (count > 0)
        for (int i = tid; i < n; i += NT) omega_out_[c * (size_t)n + i] = s_om[i];
    if (tid == 0) {
        sc->tau = s_tau;
        if constexpr (MH) sc->alpha = s_alpha;
    }
}

namespace {

using LogitChainsKernel = decltype(&k_logit_chains<512, 64, 16, false>);

// the instance for p coefficients (lanes per coefficient as the small chain's), alpha known or
// sampled; dynamic LDS above 64 KB opted in once for every instance
LogitChainsKernel logit_chain_instance(int p, int mh) {
    static const LogitChainsKernel inst[6] = {
        k_logit_chains<512, 64, 16, false>, k_logit_chains<512, 32, 8, false>,
        k_logit_chains<512, 16, 8, false>,  k_logit_chains<512, 64, 16, true>,
        k_logit_chains<512, 32, 8, true>,   k_logit_chains<512, 16, 8, true>};
    static const bool optin = [] {
        for (LogitChainsKernel k : inst)
            (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kSmallXLds);
        return true;
    }();
    (void)optin;
    static_assert(kSmallMaxP == 32, "instances above cover p <= 32");
    return inst[(mh ? 3 : 0) + (p <= 8 ? 0 : p <= 16 ? 1 : 2)];
}

}  // namespace

int launch_logit_chains(hipStream_t s, int nchains, const ChainDesign &d, const ChainState &c,
                        const ChainTraces &tr, const ChainRun &r, double *omega) {
    if (d.p < 1 || d.p > kSmallChainMaxP || d.n < d.p || d.n > kLogitChainMaxN || d.ldx < d.n ||
        (long long)d.ldx * d.p > (1ll << 30))
        return -1;
    if (r.count <= 0 || nchains <= 0) return 0;
    int rows_lds = 0;
    const size_t shm = logit_chain_shm(d.n, d.p, &rows_lds);
    logit_chain_instance(d.p, !d.hy.know_alpha)<<<nchains, 512, shm, s>>>(
        d.X, d.ldx, d.n, d.p, d.cvec, rows_lds, c.beta, c.lam, c.sc, d.hy, Key{r.k0, r.k1}, r.t0,
        r.count, r.first_slot, r.slot_step, r.cap, tr.beta, tr.lam, tr.sig2, tr.tau, tr.alpha,
        c.err, omega, r.pr_a, r.pr_b);
    return 0;
}

int logit_chains_resident_per_cu(int n, int p, int mh) {
    if (p < 1 || p > kSmallChainMaxP || n < p || n > kLogitChainMaxN) return -1;
    int rows_lds = 0, blocks = 0;
    const size_t shm = logit_chain_shm(n, p, &rows_lds);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &blocks, (const void *)logit_chain_instance(p, mh), 512, shm) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return blocks;
}

}  // namespace bb
