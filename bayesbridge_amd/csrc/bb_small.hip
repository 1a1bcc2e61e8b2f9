// bb_small.hip -- the whole stable Gibbs sweep for small p in ONE workgroup (gfx950).
//
// For the reference's published designs (diabetes 442 x 10, Boston 506 x 13: SURVEY.md s6)
// a sweep is a few microseconds of arithmetic, and a launch per step (~12 per sweep on the
// general path, with the p x p system padded to a 256 x 256 Cholesky) costs far more than
// the work.  k_small_chain runs `count` consecutive sweeps in one launch with the chain
// state in LDS, in the reference's order (Code/C/BridgeWrapper.cpp:266-298):
//   tau | beta and sig2 | beta       BridgeRegression.cpp:453-465, :436-450 (thread 0)
//   lambda | beta, tau               :506-510 (16-lane groups, retstable.cpp:94-271)
//   beta | rest                      :552-575 (A = G + diag(lambda sig2 / tau^2), A = U'U,
//                                    m = U^-1 U'^-1 c, beta = m + sig U^-1 z; one wave)
//                                    or the orthogonal design's :514-521
// with the same counters as the general path (t = t0 + k per sweep), so both draw the same
// chain up to summation order.  alpha known, or (the *_mh instances; opt-in, bb_set_tuning
// key 26; bb_small_mh.hip) sampled by the reference's random-walk MH step after beta:
//   alpha | beta, tau                :469-503 (sums in wave 0, the decision in thread 0:
//                                    bb_sampler.h's alpha_propose and alpha_mh_accept)
#include <hip/hip_runtime.h>

#include "bb_kernels.h"
#include "bb_sampler.h"

namespace bb {

// tools/small_phase_bench.cpp builds this file with BB_SMALL_PHASES: thread 0 accumulates
// the realtime-clock ticks of each phase of the sweep into g_small_phase_ticks.
#ifdef BB_SMALL_PHASES
__device__ unsigned long long g_small_phase_ticks[4];
#define SMALL_PHASE(i)                                                  \
    do {                                                                \
        if (tid == 0) {                                                 \
            const unsigned long long now = wall_clock64();              \
            if ((i) > 0) g_small_phase_ticks[(i) - 1] += now - ph_t;    \
            ph_t = now;                                                 \
        }                                                               \
    } while (0)
// read (and zero) the accumulated ticks from the host
void small_phase_ticks(unsigned long long out[4]) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_small_phase_ticks), 4 * sizeof(*out));
    const unsigned long long zero[4] = {0, 0, 0, 0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_small_phase_ticks), zero, sizeof(zero));
}
#endif

}  // namespace bb

#include "bb_small_body.h"

namespace bb {

template <int NT, int L, int I>
__global__ __launch_bounds__(NT) void k_small_chain(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, int x_lds, double *beta, double *lam,
    DevScalars *sc, Hyper hy, Key key, uint64_t t0, int count, int first_slot, int slot_step,
    int cap, double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau, double *tr_alpha,
    uint32_t *err) {
    small_chain_body<NT, L, I, false>(X, ldx, n, p, y, G, ldg, cvec, gdiag, ortho, x_lds, beta, lam, sc,
                               hy, key, t0, count, first_slot, slot_step, cap, tr_beta, tr_lam,
                               tr_sig2, tr_tau, tr_alpha, err);
}

// K independent chains, one workgroup each (blockIdx.x = chain c): the design, G, c and the
// hyper-parameters are shared and read-only; the state (beta, lam: stride p; sc, err: one per
// chain), the trace rings ([chain][slot][p], [chain][slot]) and the Philox key
// (key.k0, key.k1 + c) are the chain's own.  No workgroup waits for another, so K may exceed
// what the device holds at once: later workgroups start as earlier ones end.
// (two waves per SIMD: at most 256 VGPRs, so that two 256-thread workgroups share a CU)
template <int NT, int L, int I>
__global__ __launch_bounds__(NT, 2) void k_small_chains(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, int x_lds, double *beta, double *lam,
    DevScalars *sc, Hyper hy, Key key, uint64_t t0, int count, int first_slot, int slot_step,
    int cap, double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau, double *tr_alpha,
    uint32_t *err) {
    const size_t c = blockIdx.x;
    const Key ck{key.k0, key.k1 + (uint64_t)c};
    const size_t ring = c * (size_t)cap;
    small_chain_body<NT, L, I, true>(X, ldx, n, p, y, G, ldg, cvec, gdiag, ortho, x_lds, beta + c * p,
                               lam + c * p, sc + c, hy, ck, t0, count, first_slot, slot_step, cap,
                               tr_beta + ring * p, tr_lam + ring * p, tr_sig2 + ring,
                               tr_tau + ring, tr_alpha + ring, err + c);
}

namespace {

using SmallChainsKernel = decltype(&k_small_chains<512, 64, 16>);  // k_small_chain's type too

// The instance for p coefficients, with as many lanes per coefficient as the workgroup allows
// for p of them at once: of the single chain (batch == 0), of the batch, or of the packed
// batch.  Dynamic LDS above the 64 KB default needs a per-kernel opt-in: made once for every
// instance (thread-safe static init), with the launch error checked by the caller.
SmallChainsKernel small_chain_instance(int batch, int p, int packed, int *nt) {
    static const SmallChainsKernel inst[8] = {
        k_small_chain<512, 64, 16>,  k_small_chain<512, 32, 8>,  k_small_chain<512, 16, 8>,
        k_small_chains<512, 64, 16>, k_small_chains<512, 32, 8>, k_small_chains<512, 16, 8>,
        k_small_chains<256, 32, 8>,  k_small_chains<256, 16, 8>};
    static const bool optin = [] {
        for (SmallChainsKernel k : inst)
            (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kSmallXLds);
        return true;
    }();
    (void)optin;
    static_assert(kSmallMaxP == 32, "instances above cover p <= 32");
    *nt = batch && packed ? 256 : 512;
    if (batch && packed) return inst[p <= 8 ? 6 : 7];  // p > 16: the lambda draws in two passes
    return inst[(batch ? 3 : 0) + (p <= 8 ? 0 : p <= 16 ? 1 : 2)];
}

// `blocks` workgroups of that instance: the structs unpacked into the kernel's arguments
void small_launch(int batch, int blocks, int packed, hipStream_t s, const ChainDesign &d,
                  const ChainState &c, const ChainTraces &tr, const ChainRun &r) {
    if (r.count <= 0 || blocks <= 0) return;
    int x_lds = 0, nt = 0;
    const size_t shm = small_chain_shm(d.n, d.p, &x_lds);
    if (!d.hy.know_alpha) {  // the engine or batch was created under key 26
        small_mh_launch(batch, blocks, shm, x_lds, s, d, c, tr, r);
        return;
    }
    const SmallChainsKernel kern = small_chain_instance(batch, d.p, packed, &nt);
    kern<<<blocks, nt, shm, s>>>(
        d.X, d.ldx, d.n, d.p, d.y, d.G, d.ldg, d.cvec, d.gdiag, d.ortho, x_lds, c.beta, c.lam,
        c.sc, d.hy, Key{r.k0, r.k1}, r.t0, r.count, r.first_slot, r.slot_step, r.cap, tr.beta,
        tr.lam, tr.sig2, tr.tau, tr.alpha, c.err);
}

}  // namespace

void launch_small_chain(hipStream_t s, const ChainDesign &d, const ChainState &c,
                        const ChainTraces &tr, const ChainRun &r) {
    small_launch(0, 1, 0, s, d, c, tr, r);
}

void launch_small_chains(hipStream_t s, int nchains, int packed, const ChainDesign &d,
                         const ChainState &c, const ChainTraces &tr, const ChainRun &r) {
    small_launch(1, nchains, packed, s, d, c, tr, r);
}

int small_chains_resident_per_cu(int n, int p, int packed, int mh) {
    int x_lds = 0, blocks = 0, nt = 512;
    const size_t shm = small_chain_shm(n, p, &x_lds);
    const void *kern =
        mh ? small_mh_batch_kernel(p) : (const void *)small_chain_instance(1, p, packed, &nt);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kern, nt, shm) !=
        hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return blocks;
}

}  // namespace bb
