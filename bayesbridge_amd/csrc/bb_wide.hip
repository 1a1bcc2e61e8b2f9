// bb_wide.hip -- the whole stable Gibbs sweep for 32 < p <= 128 in ONE workgroup (gfx950).
//
// The published protocol's wider designs (diabetes and Boston with interactions, 442 x 64 and
// 506 x 103) are past bb_small.hip's p <= 32: there neither X nor a padded p x p pair (G, U)
// fits the LDS.  k_wide_chain runs `count` consecutive sweeps in one launch, in bb_small.hip's
// -- the reference's -- order (Code/C/BridgeWrapper.cpp:266-298):
//   S_alpha and rss = |y - X beta|^2  X read from memory (shared by every chain, L2-resident)
//   tau | beta and sig2 | beta        BridgeRegression.cpp:453-465, :436-450
//   lambda | beta, tau                :506-510 (16-lane groups, NT / 16 coefficients a pass)
//   beta | rest                       :552-575 (A = G + diag(lambda sig2 / tau^2) = U'U,
//                                     m = U^-1 U'^-1 c, beta = m + sig U^-1 z; the forward
//                                     solve inside the factor, the backward ones a wave each,
//                                     MAXP / 64 entries per lane) or the orthogonal design's
//                                     :514-521
// with the counters of the general path (t = t0 + k per sweep), so both draw the same chain up
// to summation order.  alpha known (the MH step runs on the general path).  The sums and the
// orthogonal beta draw are bb_chain_steps.h's, which leaves these kernels' code as it was.  The
// tau / sig2 draws and the lambda draw are chain_scalars and chain_lambda written out: called
// instead, the same arithmetic is scheduled otherwise, and the p <= 64 batch then ran 0.8-1.0 %
// slower (lambda alone written out: 1.5-1.9 % slower; the scalars alone: the p <= 64 single
// chain 2.4 % slower; the spread between rounds is 0.2-0.5 %).
//
// LDS: U alone, as its packed upper triangle of p (p + 1) / 2 doubles (dynamic: 66 KB at p =
// 128); G is read-only and shared, so every sweep reads the owned entries of its upper triangle
// through L2 straight into the registers the factor works in.
#include <hip/hip_runtime.h>

#include "bb_chain_steps.h"

namespace bb {

namespace {

constexpr int kWidePre = 16;  // sweeps of counter-only variates drawn ahead (16 KB at MAXP = 128)
constexpr int kWideL = 16, kWideI = 8;  // lanes per coefficient of the lambda draw

// entry kk of a vector held as lane + 64 q in v[q] (kk uniform over the wave)
template <int E>
__device__ __forceinline__ double entry_of(const double (&v)[E], int kk) {
    double r = 0.0;
#pragma unroll
    for (int q = 0; q < E; ++q)
        if ((kk >> 6) == q) r = readlane_f64(v[q], kk & 63);
    return r;
}

}  // namespace

// The whole sweep loop of one chain in one workgroup of NT threads, p <= MAXP: k_wide_chain runs
// it once, k_wide_chains once per workgroup on that chain's state, so the arithmetic exists
// once.  U(k, j), k <= j < p, is sU[k (2 p - k - 1) / 2 + j] (rows of the upper triangle, packed).
// LOST: a chain whose state is no longer finite skips its lambda draws (k_wide_chains).
template <int MAXP, int NT, bool LOST>
__device__ __forceinline__ void wide_chain_body(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, double *beta, double *lam, DevScalars *sc,
    Hyper hy, Key key, uint64_t t0, int count, int first_slot, int slot_step, int cap,
    double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau, double *tr_alpha,
    uint32_t *err) {
    static_assert(MAXP % 64 == 0 && NT % 64 == 0 && NT > 128 && MAXP <= NT && (NT / 16) % 16 == 0,
                  "instance shape");
    extern __shared__ double sU[];
    __shared__ double sb[MAXP], sl[MAXP], sc_[MAXP], sgd[MAXP], s_v[MAXP];
    // Ga(shape, 1) variates of tau and sig2 and the beta normals of the next kWidePre sweeps:
    // their shapes are constant along the chain (alpha known), so they depend on their
    // counters alone and come off the serial chain
    __shared__ double s_gt[kWidePre], s_gs[kWidePre], s_z[kWidePre][MAXP];
    __shared__ double red[2][NT / 64];
    __shared__ double s_tau, s_sig2;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid < p) {
        sb[tid] = beta[tid];
        sc_[tid] = cvec[tid];
        sgd[tid] = ortho ? gdiag[tid] : 0.0;
    }
    if (tid == 0) {
        s_tau = sc->tau;
        s_sig2 = sc->sig2;
    }
    const double alpha = sc->alpha;
    __syncthreads();
    const double tau_shape = hy.nu_shape + ((double)p) / alpha;
    const double sig2_shape = hy.sig2_shape + 0.5 * (double)n;
    // The upper triangle is dealt out cyclically over a 16 x NT / 16 grid of threads: thread
    // (ti, tj) owns the entries (ti + 16 a, tj + TJ b) with i <= j < p, so every thread works
    // until the last pivots.  Blocks (a, b) wholly below the diagonal (16 a > TJ b + TJ - 1)
    // hold nothing.
    constexpr int TI = 16, TJ = NT / TI, NA = MAXP / TI, NB = MAXP / TJ;
    const int p2 = 2 * p - 1;
    for (int k = 0; k < count; ++k) {
        if (k % kWidePre == 0) {
            // wave 0: tau's gamma variates, wave 1: sig2's, waves 2..: the normals
            const int nb = count - k < kWidePre ? count - k : kWidePre;
            // (one call, inlined: an out-of-line gamma1 would bring a stack frame, the only
            // private memory of the kernel)
            if (wid < 2 && lane < nb && !(wid ? hy.know_sig2 : hy.know_tau)) {
                double g;
                [[clang::always_inline]] g =
                    gamma1(wid ? sig2_shape : tau_shape, key, t0 + (uint64_t)(k + lane),
                           wid ? KIND_SIG2 : KIND_TAU, err);
                (wid ? s_gs : s_gt)[lane] = g;
            }
            for (int e = tid - 128; e >= 0 && e < nb * p; e += NT - 128) {
                const int kk = e / p, j = e % p;
                s_z[kk][j] = normal_at(key, t0 + (uint64_t)(k + kk), KIND_BETA_Z, (uint64_t)j);
            }
            __syncthreads();
        }
        const int kp = k % kWidePre;
        const uint64_t t = t0 + (uint64_t)k;
        const int slot = first_slot < 0 ? -1 : (first_slot + k * slot_step) % cap;
        // X is read from memory: shared by every chain, L2-resident
        chain_sums<NT, NT>(X, ldx, n, p, y, sb, alpha, red);
        __syncthreads();
        // tau (thread 0) and sig2 (thread 64): chain_scalars<NT, true>, written out (see above)
        if (tid == 0 || tid == 64) {
            double S = red[tid == 0 ? 0 : 1][0];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) S += red[tid == 0 ? 0 : 1][w];
            if (tid == 0) {
                if (!hy.know_tau) {
                    const double nu = s_gt[kp] / (hy.nu_rate + S);
                    s_tau = exp(-1.0 * log(nu) / alpha);
                }
                if (slot >= 0) {
                    tr_tau[slot] = s_tau;
                    tr_alpha[slot] = alpha;
                }
            } else {
                if (!hy.know_sig2) s_sig2 = (hy.sig2_scale + 0.5 * S) / s_gs[kp];
                if (slot >= 0) tr_sig2[slot] = s_sig2;
            }
        }
        __syncthreads();
        const double tau = s_tau, sig2 = s_sig2;
        // ---- lambda: chain_lambda<NT, kWideL, kWideI, LOST>, written out (see above) ----
        for (int jb = 0; jb < p; jb += NT / kWideL) {
            const int j = jb + tid / kWideL;
            const bool act = j < p;
            const double b = act ? sb[j] : 0.0;
            const double h = b * b / (tau * tau);
            const bool lost = LOST && act && h != h;
            double x = stable_spec_draw<kWideL, kWideI>(act && !lost, h, 0.5 * alpha, 1.0, key, t,
                                                        (uint64_t)j, err);
            if (lost) {
                x = __builtin_nan("");
                if ((tid % kWideL) == 0) atomicOr(err, 2u);
            }
            if (act && (tid % kWideL) == 0) {
                sl[j] = 2 * x;
                if (slot >= 0) tr_lam[(size_t)slot * p + j] = 2 * x;
            }
        }
        __syncthreads();
        // ---- beta | rest ----
        if (ortho) {
            chain_beta_ortho(p, sb, sc_, sgd, sl, s_z[kp], tau, sig2);
        } else {
            // A = G + diag(lambda sig2 / tau^2), read through L2 into the owners' registers and
            // factored right-looking as A = U'U: per pivot k the owner of (k, k) takes the
            // square root, the owners of row k divide (row k of U goes to LDS), every trailing
            // owner subtracts U(k, i) U(k, j) -- the reference's operations entry by entry
            // (BridgeRegression.cpp:560), two barriers per pivot.  c rides along as one more
            // column, held by the threads tj == 0: its row-k division is v_k = (U'^-1 c)_k and
            // its trailing update the forward solve's, operation for operation.
            // The pivots run as ka = k / 16 (unrolled) and kt = k % 16, so which blocks (a, b)
            // a pivot still touches, and that rows a > ka are wholly below it, is static.
            // (the thread's place in the grid is taken afresh each sweep, so that the indices,
            // predicates and addresses derived from it are not kept in registers across the
            // lambda draws, which need them all)
            int ft = tid;
            asm volatile("" : "+v"(ft));
            const int ti = ft % TI, tj = ft / TI;
            const double dl = tau * tau;
            double av[NA][NB], cw[NA];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int i = ti + TI * a;
                cw[a] = tj == 0 && i < p ? sc_[i] : 0.0;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (TI * a > TJ * b + TJ - 1) continue;
                    const int j = tj + TJ * b;
                    av[a][b] = 0.0;
                    if (i <= j && j < p)
                        av[a][b] =
                            G[(size_t)i + (size_t)j * ldg] + (i == j ? sl[i] * sig2 / dl : 0.0);
                }
            }
#pragma unroll
            for (int ka = 0; ka < NA; ++ka) {
                const int kb = ka * TI / TJ;  // the block column of the pivots ka TI .. ka TI + 15
                for (int kt = 0; kt < TI && ka * TI + kt < p; ++kt) {
                    const int kk = ka * TI + kt;
                    double *urow = sU + kk * (p2 - kk) / 2;  // urow[j] = U(kk, j)
                    if (ti == kt && tj == kk % TJ) {
                        if (!(av[ka][kb] > 0.0)) atomicOr(err, 8u);
                        av[ka][kb] = sqrt(av[ka][kb]);
                        urow[kk] = av[ka][kb];
                    }
                    __syncthreads();
                    const double d = urow[kk];
                    if (ti == kt) {
#pragma unroll
                        for (int b = kb; b < NB; ++b) {
                            const int j = tj + TJ * b;
                            if (j > kk && j < p) {
                                av[ka][b] = av[ka][b] / d;
                                urow[j] = av[ka][b];
                            }
                        }
                        if (tj == 0) {
                            cw[ka] = cw[ka] / d;
                            s_v[kk] = cw[ka];
                        }
                    }
                    __syncthreads();
                    // U(kk, j) of the owned columns and U(kk, i) of the owned rows, once each
                    double uj[NB];
#pragma unroll
                    for (int b = kb; b < NB; ++b) {
                        const int j = tj + TJ * b;
                        uj[b] = j < p ? urow[j] : 0.0;
                    }
                    const double vk = s_v[kk];
#pragma unroll
                    for (int a = ka; a < NA; ++a) {
                        const int i = ti + TI * a;
                        const double ui = i < p ? urow[i] : 0.0;
                        const bool below = a > ka || ti > kt;  // row i > kk
#pragma unroll
                        for (int b = kb; b < NB; ++b) {
                            if (TI * a > TJ * b + TJ - 1) continue;
                            const int j = tj + TJ * b;
                            const bool upper = TI * a + TI - 1 <= TJ * b || i <= j;
                            if (below && upper && j < p) av[a][b] -= ui * uj[b];
                        }
                        if (tj == 0 && below && i < p) cw[a] -= ui * vk;
                    }
                }
            }
            __syncthreads();
            if (wid < 2) {
                // backward solves, a wave each: U m = v (wave 0, into sb) and U x = z (wave 1,
                // in place); lane l holds the entries l, l + 64, ... and U's diagonal at them
                constexpr int E = MAXP / 64;
                double w[E], dg[E];
                double *out = wid ? s_z[kp] : sb;
#pragma unroll
                for (int q = 0; q < E; ++q) {
                    const int j = lane + 64 * q;
                    w[q] = j < p ? (wid ? s_z[kp][j] : s_v[j]) : 0.0;
                    dg[q] = j < p ? sU[j * (p2 - j) / 2 + j] : 1.0;
                }
                for (int kk = p - 1; kk >= 0; --kk) {
                    const double mk = entry_of<E>(w, kk) / entry_of<E>(dg, kk);
#pragma unroll
                    for (int q = 0; q < E; ++q) {
                        const int j = lane + 64 * q;
                        if (j < kk) w[q] -= sU[j * (p2 - j) / 2 + kk] * mk;
                        if (j == kk) w[q] = mk;
                    }
                }
#pragma unroll
                for (int q = 0; q < E; ++q) {
                    const int j = lane + 64 * q;
                    if (j < p) out[j] = w[q];
                }
            }
            __syncthreads();
            if (tid < p) sb[tid] = sb[tid] + sqrt(sig2) * s_z[kp][tid];
        }
        __syncthreads();
        if (slot >= 0 && tid < p) tr_beta[(size_t)slot * p + tid] = sb[tid];
    }
    if (tid < p) {
        beta[tid] = sb[tid];
        lam[tid] = sl[tid];
    }
    if (tid == 0) {
        sc->tau = s_tau;
        sc->sig2 = s_sig2;
    }
}

// (two waves per SIMD: at most 256 VGPRs, so that two 256-thread workgroups share a CU; the
// single chain takes the same bound and so the same code)
template <int MAXP, int NT>
__global__ __launch_bounds__(NT, 2) void k_wide_chain(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, double *beta, double *lam, DevScalars *sc,
    Hyper hy, Key key, uint64_t t0, int count, int first_slot, int slot_step, int cap,
    double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau, double *tr_alpha,
    uint32_t *err) {
    wide_chain_body<MAXP, NT, false>(X, ldx, n, p, y, G, ldg, cvec, gdiag, ortho, beta, lam, sc, hy,
                                     key, t0, count, first_slot, slot_step, cap, tr_beta, tr_lam,
                                     tr_sig2, tr_tau, tr_alpha, err);
}

// K independent chains, one workgroup each (blockIdx.x = chain c), laid out as k_small_chains
// lays them out: the design, G, c and the hyper-parameters are shared and read-only; the state
// (beta, lam: stride p; sc, err: one per chain), the trace rings ([chain][slot][p],
// [chain][slot]) and the Philox key (key.k0, key.k1 + c) are the chain's own.  No workgroup
// waits for another, so K may exceed what the device holds at once.
template <int MAXP, int NT>
__global__ __launch_bounds__(NT, 2) void k_wide_chains(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, double *beta, double *lam, DevScalars *sc,
    Hyper hy, Key key, uint64_t t0, int count, int first_slot, int slot_step, int cap,
    double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau, double *tr_alpha,
    uint32_t *err) {
    const size_t c = blockIdx.x;
    const Key ck{key.k0, key.k1 + (uint64_t)c};
    const size_t ring = c * (size_t)cap;
    wide_chain_body<MAXP, NT, true>(X, ldx, n, p, y, G, ldg, cvec, gdiag, ortho, beta + c * p,
                                    lam + c * p, sc + c, hy, ck, t0, count, first_slot, slot_step,
                                    cap, tr_beta + ring * p, tr_lam + ring * p, tr_sig2 + ring,
                                    tr_tau + ring, tr_alpha + ring, err + c);
}

namespace {

using WideChainsKernel = decltype(&k_wide_chains<64, 256>);  // k_wide_chain's type too

// dynamic LDS of a launch: the packed upper triangle of U
size_t wide_chain_shm(int p) { return tri_count(p) * sizeof(double); }

// The instance for p coefficients (nullptr: none), of the single chain (batch == 0) or of the
// batch: MAXP = 64 in 256 threads, MAXP = 128 in 512.  Dynamic LDS above the 64 KB default
// needs a per-kernel opt-in: made once for every instance (thread-safe static init), with the
// launch error checked by the caller.
WideChainsKernel wide_chain_instance(int batch, int p, int *nt) {
    static const WideChainsKernel inst[4] = {k_wide_chain<64, 256>, k_wide_chain<128, 512>,
                                             k_wide_chains<64, 256>, k_wide_chains<128, 512>};
    static const bool optin = [] {
        for (WideChainsKernel k : inst)
            (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)wide_chain_shm(kWideChainMaxP));
        return true;
    }();
    (void)optin;
    static_assert(kWideChainMaxP == 128, "instances above cover p <= 128");
    if (p < 1 || p > kWideChainMaxP) return nullptr;
    *nt = p <= 64 ? 256 : 512;
    return inst[(batch ? 2 : 0) + (p <= 64 ? 0 : 1)];
}

// `blocks` workgroups of that instance: the structs unpacked into the kernel's arguments
int wide_launch(int batch, int blocks, hipStream_t s, const ChainDesign &d, const ChainState &c,
                const ChainTraces &tr, const ChainRun &r) {
    int nt = 0;
    const WideChainsKernel kern = wide_chain_instance(batch, d.p, &nt);
    if (!kern) return -1;
    if (r.count <= 0 || blocks <= 0) return 0;
    kern<<<blocks, nt, wide_chain_shm(d.p), s>>>(
        d.X, d.ldx, d.n, d.p, d.y, d.G, d.ldg, d.cvec, d.gdiag, d.ortho, c.beta, c.lam, c.sc, d.hy,
        Key{r.k0, r.k1}, r.t0, r.count, r.first_slot, r.slot_step, r.cap, tr.beta, tr.lam, tr.sig2,
        tr.tau, tr.alpha, c.err);
    return 0;
}

}  // namespace

int launch_wide_chain(hipStream_t s, const ChainDesign &d, const ChainState &c,
                      const ChainTraces &tr, const ChainRun &r) {
    return wide_launch(0, 1, s, d, c, tr, r);
}

int launch_wide_chains(hipStream_t s, int nchains, const ChainDesign &d, const ChainState &c,
                       const ChainTraces &tr, const ChainRun &r) {
    return wide_launch(1, nchains, s, d, c, tr, r);
}

int wide_chains_resident_per_cu(int p) {
    int blocks = 0, nt = 0;
    const WideChainsKernel kern = wide_chain_instance(1, p, &nt);
    if (!kern ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void *)kern, nt,
                                                     wide_chain_shm(p)) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return blocks;
}

int wide_chains_threads(int p) { return p <= 64 ? 256 : 512; }

}  // namespace bb
