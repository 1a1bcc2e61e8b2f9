// bb_tri.hip -- triangle-mixture Gibbs update for bridge.reg.tri (gfx950).
//
// Reference: Code/C/BridgeRegression.cpp:97-147 (sample_u, sample_omega with shape),
// :405-433 (sample_beta), :235-286 (rtnorm_gibbs); driver BridgeWrapper.cpp:80-204.
//
// rtnorm_gibbs is a sequential coordinate sweep over the p coordinates z = V'beta; each
// step needs the tightest bounds over all p box constraints |beta_j| <= b_j.  One
// workgroup of 256 threads runs the whole update: thread j owns coefficients
// j + 256 k (b_j and beta_cur_j = (tV' z)_j stay in registers), the row v_i. of tV is
// prefetched one coordinate ahead, the bounds are DPP-reduced per 16-lane row, then per
// wave (max/min are exact, so any tree gives the CPU checker's value) and every lane
// evaluates the same truncated-normal draw redundantly: one barrier per coordinate.
// beta_cur is kept up to date incrementally
// (beta_cur_j += v_ij dz_i) instead of recomputing dot(v_j, z) per coordinate as :254-258
// does: the same quantity in O(p^2) instead of O(p^3) per pass (oracle/bb_oracle.c
// bbo_tri_update uses the identical update order).
//
// r.tnorm comes from the un-vendored RNG library; it is restated from Robert (1995):
// normal or uniform rejection when the standardised interval holds 0, else Robert's
// uniform / translated-exponential proposal.  Counter kinds 8 (omega), 9 (u), 10 (z_i).
// The draws and the fused chain's sweep body are bb_tri_body.h's, shared with bb_tri_mh.hip.
#include <hip/hip_runtime.h>

#include "bb_tri_body.h"

namespace bb {

namespace {

// tVc: tV column-major (tVc[i + j p] = tV(i, j)); tVr: its transpose (tVr[i p + j] =
// tV(i, j)), so row i of tV is contiguous for the coordinate loop.
__global__ __launch_bounds__(kTriNT) void k_tri_update(
    double *beta, double *u, double *omega, double *shape, int p, const double *tVc,
    const double *tVr, const double *av, const double *dv, const double *Gf, const double *cv,
    int ortho, const DevScalars *sc, int betaburn, Key key, uint64_t t, double *tr_beta,
    double *tr_u, double *tr_omega, double *tr_shape, uint32_t *err) {
    __shared__ double sz[kTriMaxP];
    __shared__ double sb[kTriMaxP];
    __shared__ double sbnd[kTriMaxP];
    __shared__ Pre spre[kTriMaxP];
    // per-coordinate constants staged once: a global load inside the serial loop would put
    // a full memory latency on every coordinate's critical path
    __shared__ double sav[kTriMaxP], sdv[kTriMaxP];
    // per-wave partials, double-buffered by coordinate parity: one barrier per coordinate
    __shared__ double shmax[2][kTriNT / 64], shmin[2][kTriNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double tau = sc->tau, sig2 = sc->sig2, alpha = sc->alpha;

    double bj[kTriE], bcur[kTriE];
#pragma unroll
    for (int e = 0; e < kTriE; ++e) {
        const int j = tid + e * kTriNT;
        bj[e] = 0.0;
        if (j < p) {
            const double betaj = beta[j];
            // sample_omega (BridgeRegression.cpp:130-146)
            const double aj = exp(alpha * log(fabs(betaj) / ((1.0 - u[j]) * tau)));
            const double prob = alpha / (1.0 + alpha * aj);
            U4 r = uniforms(key, t, KIND_TRI_OMEGA, (uint64_t)j, 0, 0);
            double w, sh;
            if (r.r[0] > prob) {
                sh = 1.0;
                w = -log(r.r[1]);  // Ga(1, 1)
            } else {
                sh = 2.0;
                w = -log(r.r[1]) - log(r.r[2]);  // Ga(2, 1)
            }
            const double om = w + aj;
            // sample_u (:97-111): flat(0, right)
            const double right = 1.0 - fabs(betaj) / tau * exp(-1.0 * log(om) / alpha);
            U4 r2 = uniforms(key, t, KIND_TRI_U, (uint64_t)j, 0, 0);
            const double uj = right * r2.r[0];
            bj[e] = (1.0 - uj) * exp(log(om) / alpha) * tau;  // sample_beta :410-412
            sbnd[j] = bj[e];
            omega[j] = om;
            shape[j] = sh;
            u[j] = uj;
            if (tr_omega) tr_omega[j] = om;
            if (tr_shape) tr_shape[j] = sh;
            if (tr_u) tr_u[j] = uj;
            sb[j] = betaj;
            sav[j] = ortho ? cv[j] : av[j];
            sdv[j] = ortho ? Gf[(size_t)j * p + j] : dv[j];
        }
    }
    __syncthreads();
    const double sig = sqrt(sig2);
    // Every thread reduces the per-wave partials in the same order and evaluates the same
    // draw (uniform control flow, no divergence), so no broadcast barrier is needed; the
    // owner of a coefficient keeps the state it alone reads later.
    auto precompute = [&](int it) {
        for (int i = tid; i < p; i += kTriNT) {
            U4 r = uniforms(key, t, KIND_TRI_Z, (uint64_t)i, (uint64_t)it, 0);
            spre[i] = Pre{r.r[0], r.r[1], bm_normal(r.r[0], r.r[1])};
        }
    };
    if (ortho) {
        // sample_beta_ortho (BridgeRegression.cpp:362-403): coordinate Gibbs on beta itself,
        // m_j = (c_j - sum_{k != j} G_jk beta_k) / G_jj, one pass (its burn defaults to 0).
        // Gf is the full symmetric Gram, row j contiguous.
        precompute(0);
        __syncthreads();
        double gn[kTriE];
#pragma unroll
        for (int e = 0; e < kTriE; ++e) gn[e] = tid + e * kTriNT < p ? Gf[tid + e * kTriNT] : 0.0;
        for (int j = 0; j < p; ++j) {
            double g[kTriE];
#pragma unroll
            for (int e = 0; e < kTriE; ++e) g[e] = gn[e];
            if (j + 1 < p) {
#pragma unroll
                for (int e = 0; e < kTriE; ++e) {
                    const int k = tid + e * kTriNT;
                    gn[e] = k < p ? Gf[(size_t)(j + 1) * p + k] : 0.0;
                }
            }
            double part = 0.0;
#pragma unroll
            for (int e = 0; e < kTriE; ++e) {
                const int k = tid + e * kTriNT;
                if (k < p && k != j) part += g[e] * sb[k];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if (lane == 0) shmax[j & 1][wv] = part;
            __syncthreads();
            double xb = 0.0;
#pragma unroll
            for (int w = 0; w < kTriNT / 64; ++w) xb += shmax[j & 1][w];
            if (tid == (j % kTriNT)) {  // the owner draws and keeps beta_j
                const double gjj = sdv[j];
                const double m = (sav[j] - xb) / gjj;
                const double v = sig2 / gjj;
                const double bnd = sbnd[j];
                sb[j] = tnorm(-1.0 * bnd, bnd, m, sqrt(v), key, t, (uint64_t)j, 0, spre[j], err);
            }
        }
        __syncthreads();
    } else {
        // the conditional mean a_i / d_i^2 and sd sigma / d_i of every coordinate, off the
        // serial chain (same expressions, so the same bits); sd < 0 flags d_i <= 1e-16
        for (int i = tid; i < p; i += kTriNT) {
            const double di = sdv[i];
            const bool ok = di > 1e-16;
            sav[i] = ok ? sav[i] / (di * di) : 0.0;
            sdv[i] = ok ? sig / di : -1.0;
        }
        __syncthreads();
    }
    for (int it = 0; it <= (ortho ? -1 : betaburn); ++it) {
        precompute(it);
        // z = tV beta (:246)
        for (int i = tid; i < p; i += kTriNT) {
            double s = 0.0;
            for (int j = 0; j < p; ++j) s += tVc[i + (size_t)j * p] * sb[j];
            sz[i] = s;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kTriE; ++e) {
            const int j = tid + e * kTriNT;
            double s = 0.0;
            if (j < p)
                for (int k = 0; k < p; ++k) s += tVr[(size_t)k * p + j] * sz[k];
            bcur[e] = s;
        }
        double vn[kTriE];
#pragma unroll
        for (int e = 0; e < kTriE; ++e) {
            const int j = tid + e * kTriNT;
            vn[e] = j < p ? tVr[j] : 0.0;
        }
        for (int i = 0; i < p; ++i) {  // :250-283
            double v[kTriE];
#pragma unroll
            for (int e = 0; e < kTriE; ++e) v[e] = vn[e];
            if (i + 1 < p) {
#pragma unroll
                for (int e = 0; e < kTriE; ++e) {
                    const int j = tid + e * kTriNT;
                    vn[e] = j < p ? tVr[(size_t)(i + 1) * p + j] : 0.0;
                }
            }
            const double zi = sz[i];
            double lmax = -1.0 * 1.7976931348623157e308, rmin = 1.7976931348623157e308;
#pragma unroll
            for (int e = 0; e < kTriE; ++e) {
                const int j = tid + e * kTriNT;
                if (j < p) {
                    const double vji = v[e];
                    const double rji = bcur[e] - vji * zi;
                    const double dif = bj[e] - rji, sum = bj[e] + rji;
                    const double left = (vji > 0 ? -sum : -dif) / fabs(vji);
                    const double right = (vji > 0 ? dif : sum) / fabs(vji);
                    lmax = lmax > left ? lmax : left;
                    rmin = rmin < right ? rmin : right;
                }
            }
            lmax = rows_max(row16_max(lmax));
            rmin = rows_min(row16_min(rmin));
            if (lane == 0) {  // one partial per wave
                shmax[i & 1][wv] = lmax;
                shmin[i & 1][wv] = rmin;
            }
            // LDS-only barrier: __syncthreads() would also drain the row prefetch (vmcnt(0))
            // LDS writes visible, then the barrier, in ONE asm statement with a memory
            // clobber so no LDS access can be scheduled across the pair
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            double L = shmax[i & 1][0], R = shmin[i & 1][0];
#pragma unroll
            for (int w = 1; w < kTriNT / 64; ++w) {
                L = L > shmax[i & 1][w] ? L : shmax[i & 1][w];
                R = R < shmin[i & 1][w] ? R : shmin[i & 1][w];
            }
            const double sdi = sdv[i];
            double zn;
            if (sdi > 0.0) {
                zn = tnorm(L, R, sav[i], sdi, key, t, (uint64_t)i, (uint64_t)it, spre[i], err);
            } else {
                zn = L + (R - L) * spre[i].r0;
            }
            const double dz = zn - zi;
            if (tid == 0) sz[i] = zn;  // read again only after the loop's closing barrier
#pragma unroll
            for (int e = 0; e < kTriE; ++e) bcur[e] += v[e] * dz;
        }
        __syncthreads();
        // beta = tV' z (:285)
#pragma unroll
        for (int e = 0; e < kTriE; ++e) {
            const int j = tid + e * kTriNT;
            if (j < p) {
                double s = 0.0;
                for (int k = 0; k < p; ++k) s += tVr[(size_t)k * p + j] * sz[k];
                sb[j] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < kTriE; ++e) {
        const int j = tid + e * kTriNT;
        if (j < p) {
            beta[j] = sb[j];
            if (tr_beta) tr_beta[j] = sb[j];
        }
    }
}

__global__ __launch_bounds__(kTcNT) void k_tri_chain(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ tVc, const double *__restrict__ tVr,
    const double *__restrict__ av, const double *__restrict__ dv, const double *__restrict__ Gf,
    const double *__restrict__ cv, int ortho, int x_lds, double *beta,
    double *u, double *omega, double *shape, DevScalars *sc, Hyper hy, int betaburn, Key key,
    uint64_t t0, int count, int first_slot, int slot_step, int cap, double *tr_beta,
    double *tr_u, double *tr_omega, double *tr_shape, double *tr_sig2, double *tr_tau,
    double *tr_alpha, uint32_t *err) {
    tri_chain_body<kTcNT, false, false>(X, ldx, n, p, y, tVc, tVr, av, dv, Gf, cv, ortho, x_lds,
                                        beta, u, omega, shape, sc, hy, betaburn, key, t0, count,
                                        first_slot, slot_step, cap, tr_beta, tr_u, tr_omega,
                                        tr_shape, tr_sig2, tr_tau, tr_alpha, err);
}

// K independent chains, one workgroup each (blockIdx.x = chain c): the design, the basis (or
// Gf, cv), the hyper-parameters and betaburn are shared and read-only; the state (beta, u,
// omega, shape: stride p; sc, err: one per chain), the trace rings ([chain][slot][p],
// [chain][slot]) and the Philox key (key.k0, key.k1 + c) are the chain's own.  No workgroup
// waits for another, so K may exceed what the device holds at once.
// (two waves per SIMD: at most 256 VGPRs, what the 512-thread single chain is built with, so
// that 512 / NT workgroups share a CU's registers)
template <int NT, bool COMPACT>
__global__ __launch_bounds__(NT, 2) void k_tri_chains(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ tVc, const double *__restrict__ tVr,
    const double *__restrict__ av, const double *__restrict__ dv, const double *__restrict__ Gf,
    const double *__restrict__ cv, int ortho, int x_lds, double *beta,
    double *u, double *omega, double *shape, DevScalars *sc, Hyper hy, int betaburn, Key key,
    uint64_t t0, int count, int first_slot, int slot_step, int cap, double *tr_beta,
    double *tr_u, double *tr_omega, double *tr_shape, double *tr_sig2, double *tr_tau,
    double *tr_alpha, uint32_t *err) {
    const size_t c = blockIdx.x;
    const Key ck{key.k0, key.k1 + (uint64_t)c};
    const size_t ring = c * (size_t)cap;
    tri_chain_body<NT, COMPACT, true>(
        X, ldx, n, p, y, tVc, tVr, av, dv, Gf, cv, ortho, x_lds, beta + c * p, u + c * p,
        omega + c * p, shape + c * p, sc + c, hy, betaburn, ck, t0, count, first_slot, slot_step,
        cap, tr_beta + ring * p, tr_u + ring * p, tr_omega + ring * p, tr_shape + ring * p,
        tr_sig2 + ring, tr_tau + ring, tr_alpha + ring, err + c);
}

// Truncated normal / exponential batches behind the .C utilities rtnorm_left, rtnorm_both,
// rtnorm, rtexpon_rate_left, rtexpon_rate_both, rtexpon_rate (BridgeWrapper.cpp:762-935):
// one lane per draw; draw i uses counters (0, 10 << 56 | i, 0, k) for truncated-normal
// attempts and (0, 12 << 56 | i, 0, 0) for the exponential / untruncated normal.
constexpr unsigned KIND_TRUNC = 12;

__device__ double texpon(double left, double right, double rate, double u) {
    if (isinf(right)) return left - log(u) / rate;  // memoryless left truncation
    return left - log1p(u * expm1(-rate * (right - left))) / rate;  // inversion on [l, r]
}

__global__ __launch_bounds__(256) void k_trunc_batch(int mode, int num, double *x,
                                                     const double *p0, const double *p1,
                                                     const double *p2, const double *p3, Key key,
                                                     uint32_t *err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num) return;
    const double inf = __builtin_inf();
    U4 r = uniforms(key, 0, KIND_TRI_Z, (uint64_t)i, 0, 0);
    const Pre pre{r.r[0], r.r[1], bm_normal(r.r[0], r.r[1])};
    const U4 e = uniforms(key, 0, KIND_TRUNC, (uint64_t)i, 0, 0);
    double out;
    switch (mode) {
        case 0:  // rtnorm_left(left, mu, sig)
            out = tnorm(p0[i], inf, p1[i], p2[i], key, 0, i, 0, pre, err);
            break;
        case 1:  // rtnorm_both(left, right, mu, sig)
            out = tnorm(p0[i], p1[i], p2[i], p3[i], key, 0, i, 0, pre, err);
            break;
        case 2: {  // rtnorm(left, right, mu, sig), USE_R branch (:904-919)
            const double l = p0[i], rt = p1[i], mu = p2[i], sg = p3[i];
            if (isnan(l) || isnan(rt) || isnan(mu) || isnan(sg)) {
                out = __builtin_nan("");
            } else if (!isinf(l) && !isinf(rt)) {
                out = tnorm(l, rt, mu, sg, key, 0, i, 0, pre, err);
            } else if (!isinf(l) && rt == inf) {
                out = tnorm(l, inf, mu, sg, key, 0, i, 0, pre, err);
            } else if (l == -inf && !isinf(rt)) {
                out = -1.0 * tnorm(-1.0 * rt, inf, -1.0 * mu, sg, key, 0, i, 0, pre, err);
            } else if (l == -inf && rt == inf) {
                out = mu + sg * bm_normal(e.r[0], e.r[1]);
            } else {
                out = __builtin_nan("");
            }
            break;
        }
        case 3:  // rtexpon_rate_left(left, rate)
            out = texpon(p0[i], inf, p1[i], e.r[0]);
            break;
        case 4:  // rtexpon_rate_both(left, right, rate)
            out = texpon(p0[i], p1[i], p2[i], e.r[0]);
            break;
        default: {  // rtexpon_rate(left, right, rate) (:805-830)
            // the reference sets x = NaN and prints for a non-finite input, then the draw
            // below overwrites it (no else): a non-finite right means left truncation only
            const double l = p0[i], rt = p1[i], rate = p2[i];
            if (isnan(l) || isnan(rt) || isnan(rate) || isinf(l))
                atomicOr(err, 256u);  // the host prints the reference's stderr line
            out = texpon(l, isfinite(rt) ? rt : inf, rate, e.r[0]);
            break;
        }
    }
    x[i] = out;
}

// Right-truncated gamma (rrtgamma_rate, BridgeWrapper.cpp:944-962): Y = rate x ~ Ga(a, 1)
// restricted to (0, T], T = rate right_t; the four exact rejection regimes of
// oracle/bb_oracle.c bbo_rtgamma_std, attempt k on counters (0, 13 << 56 | i, k, 0).
constexpr unsigned KIND_RTGAMMA = 13;

__device__ double rtgamma_std(double a, double T, Key key, uint64_t i, uint32_t *err) {
    for (long k = 0; k < kTnMaxAttempts; ++k) {
        const U4 r = uniforms(key, 0, KIND_RTGAMMA, i, (uint64_t)k, 0);
        if (T >= a) {  // Marsaglia-Tsang draw, accept if it lands below T
            const double ap = a < 1.0 ? a + 1.0 : a;
            const double d = ap - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * d);
            const double x = bm_normal(r.r[0], r.r[1]);
            double v = 1.0 + cc * x;
            if (v <= 0.0) continue;
            v = v * v * v;
            const double x2 = x * x;
            if (!(r.r[2] < 1.0 - 0.0331 * x2 * x2) &&
                !(log(r.r[2]) < 0.5 * x2 + d * (1.0 - v + log(v))))
                continue;
            double y = d * v;
            if (a < 1.0) y *= pow(r.r[3], 1.0 / a);
            if (y <= T) return y;
        } else if (a <= 1.0) {  // power proposal, accept w.p. e^-y
            const double y = T * pow(r.r[0], 1.0 / a);
            if (r.r[1] <= exp(-y)) return y;
        } else if (T <= a - 1.0) {  // increasing log-concave: tangent envelope at T
            const double c = (a - 1.0) / T - 1.0;
            const double z = c > 0.0 ? -log1p(r.r[0] * expm1(-c * T)) / c : T * r.r[0];
            const double y = T - z;
            if (y > 0.0 && log(r.r[1]) <= (a - 1.0) * log(y / T) + z + c * z) return y;
        } else {  // mode inside (0, T): uniform proposal bounded at the mode
            const double m = a - 1.0;
            const double y = T * r.r[0];
            if (log(r.r[1]) <= (a - 1.0) * log(y / m) - (y - m)) return y;
        }
    }
    atomicOr(err, 64u);
    return T;
}

__global__ __launch_bounds__(256) void k_rrtgamma_batch(int num, double *x, const double *shape,
                                                        const double *rate,
                                                        const double *right_t, Key key,
                                                        uint32_t *err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num) return;
    x[i] = rtgamma_std(shape[i], rate[i] * right_t[i], key, (uint64_t)i, err) / rate[i];
}

}  // namespace

void launch_rrtgamma_batch(hipStream_t s, int num, double *x, const double *shape,
                           const double *rate, const double *right_t, uint64_t k0, uint64_t k1,
                           uint32_t *err) {
    if (num <= 0) return;
    hipLaunchKernelGGL(k_rrtgamma_batch, dim3((num + 255) / 256), dim3(256), 0, s, num, x, shape,
                       rate, right_t, Key{k0, k1}, err);
}

void launch_trunc_batch(hipStream_t s, int mode, int num, double *x, const double *p0,
                        const double *p1, const double *p2, const double *p3, uint64_t k0,
                        uint64_t k1, uint32_t *err) {
    if (num <= 0) return;
    hipLaunchKernelGGL(k_trunc_batch, dim3((num + 255) / 256), dim3(256), 0, s, mode, num, x, p0,
                       p1, p2, p3, Key{k0, k1}, err);
}

void launch_tri_update(hipStream_t s, double *beta, double *u, double *omega, double *shape,
                       int p, const double *tVc, const double *tVr, const double *a,
                       const double *d, const double *Gf, const double *c, int ortho,
                       const DevScalars *sc, int betaburn, uint64_t k0, uint64_t k1, uint64_t t,
                       double *tr_beta, double *tr_u, double *tr_omega, double *tr_shape,
                       uint32_t *err) {
    if (p < 1 || p > kTriMaxP) return;  // the engine checks p at setup
    hipLaunchKernelGGL(k_tri_update, dim3(1), dim3(kTriNT), 0, s, beta, u, omega, shape, p, tVc,
                       tVr, a, d, Gf, c, ortho, sc, betaburn, Key{k0, k1}, t, tr_beta, tr_u,
                       tr_omega, tr_shape, err);
}

namespace {

using TriChainsKernel = decltype(&k_tri_chains<kTcNT, false>);
struct TriChainsInstance {
    TriChainsKernel kern;
    int nt;
    bool compact;
};

// The batch instance of `threads` threads (nullptr: none), its >64 KB LDS opt-in made once.
const TriChainsInstance *tri_chains_instance(int threads) {
    static const TriChainsInstance inst[] = {{k_tri_chains<kTcNT, false>, kTcNT, false},
                                             {k_tri_chains<256, true>, 256, true},
                                             {k_tri_chains<128, true>, 128, true}};
    static const bool optin = [] {
        for (const TriChainsInstance &i : inst)
            (void)hipFuncSetAttribute((const void *)i.kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      tri_chain_shm_max(i.compact));
        return true;
    }();
    (void)optin;
    for (const TriChainsInstance &i : inst)
        if (i.nt == threads) return &i;
    return nullptr;
}

// `blocks` workgroups of instance i (k_tri_chain has the kernels' type too): the structs
// unpacked into its arguments
void tri_launch(const TriChainsInstance &i, int blocks, hipStream_t s, const ChainDesign &d,
                const ChainState &c, const ChainTraces &tr, const ChainRun &r) {
    int x_lds = 0;
    const size_t shm = tri_chain_shm(i.compact, d.n, d.p, &x_lds);
    i.kern<<<blocks, i.nt, shm, s>>>(
        d.X, d.ldx, d.n, d.p, d.y, d.tVc, d.tVr, d.a, d.d, d.Gf, d.cvec, d.ortho, x_lds, c.beta,
        c.u, c.lam, c.shape, c.sc, d.hy, d.betaburn, Key{r.k0, r.k1}, r.t0, r.count, r.first_slot,
        r.slot_step, r.cap, tr.beta, tr.u, tr.lam, tr.shape, tr.sig2, tr.tau, tr.alpha, c.err);
}

}  // namespace

// d.hy.know_alpha == 0 (engines and batches created under bb_set_tuning key 27): the instances
// of bb_tri_mh.hip, which sample alpha in the sweep.
void launch_tri_chain(hipStream_t s, const ChainDesign &d, const ChainState &c,
                      const ChainTraces &tr, const ChainRun &r) {
    if (r.count <= 0 || d.p < 1 || d.p > kTriChainMaxP) return;  // the engine checks p at setup
    if (!d.hy.know_alpha) {
        (void)tri_mh_launch(0, kTcNT, 1, s, d, c, tr, r);  // the 512-thread instance exists
        return;
    }
    static const hipError_t attr = hipFuncSetAttribute(  // one-time opt-in above 64 KB
        (const void *)k_tri_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTcXLds);
    (void)attr;
    tri_launch({k_tri_chain, kTcNT, false}, 1, s, d, c, tr, r);
}

int launch_tri_chains(hipStream_t s, int nchains, int threads, const ChainDesign &d,
                      const ChainState &c, const ChainTraces &tr, const ChainRun &r) {
    const TriChainsInstance *inst = tri_chains_instance(threads);
    if (!inst || d.p < 1 || d.p > kTriChainMaxP) return -1;  // the batch checks both at creation
    if (r.count <= 0 || nchains <= 0) return 0;
    if (!d.hy.know_alpha) return tri_mh_launch(1, threads, nchains, s, d, c, tr, r);
    tri_launch(*inst, nchains, s, d, c, tr, r);
    return 0;
}

// The instance for a batch of `nchains` on a device of `cus` compute units: the widest one
// that holds every chain at once (a wider workgroup leaves wave 0 more of its SIMD), else the
// one that holds the most.  Every instance gives the same bits, so this is a matter of speed
// alone.
int tri_chains_threads(int n, int p, int nchains, int cus, int mh) {
    int best = kTcNT, best_r = 0;
    for (int nt : {kTcNT, 256, 128}) {
        const int r = tri_chains_resident_per_cu(n, p, nt, mh);
        if (r <= best_r) continue;
        best = nt;
        best_r = r;
        if ((long)nchains <= (long)r * cus) break;
    }
    return best;
}

int tri_chains_resident_per_cu(int n, int p, int threads, int mh) {
    const TriChainsInstance *inst = tri_chains_instance(threads);
    if (!inst) return -1;
    // the kernel that will run: the MH instances have their own registers and LDS
    const void *kern = mh ? tri_mh_batch_kernel(threads) : (const void *)inst->kern;
    int x_lds = 0, blocks = 0;
    const size_t shm = tri_chain_shm(inst->compact, n, p, &x_lds);
    if (!kern ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kern, inst->nt, shm) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return blocks;
}

}  // namespace bb
