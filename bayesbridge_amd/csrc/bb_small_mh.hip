// bb_small_mh.hip -- the fused small-p chain with alpha sampled (gfx950; opt-in, bb_set_tuning
// key 26): bb_small.hip's kernels over the MH instance of the one sweep body (bb_small_body.h),
// under the Beta prior (pr_a, pr_b) of the launch's phase.  Single chain and batch, the three
// 512-thread lane splits; no packed 256-thread instance.
#include "bb_small_body.h"

namespace bb {

template <int NT, int L, int I>
__global__ __launch_bounds__(NT) void k_small_chain_mh(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, int x_lds, double *beta, double *lam,
    DevScalars *sc, Hyper hy, Key key, uint64_t t0, int count, int first_slot, int slot_step,
    int cap, double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau, double *tr_alpha,
    uint32_t *err, double pr_a, double pr_b) {
    small_chain_body<NT, L, I, false, true>(X, ldx, n, p, y, G, ldg, cvec, gdiag, ortho, x_lds,
                                            beta, lam, sc, hy, key, t0, count, first_slot,
                                            slot_step, cap, tr_beta, tr_lam, tr_sig2, tr_tau,
                                            tr_alpha, err, pr_a, pr_b);
}

template <int NT, int L, int I>
__global__ __launch_bounds__(NT, 2) void k_small_chains_mh(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ G, int ldg, const double *__restrict__ cvec,
    const double *__restrict__ gdiag, int ortho, int x_lds, double *beta, double *lam,
    DevScalars *sc, Hyper hy, Key key, uint64_t t0, int count, int first_slot, int slot_step,
    int cap, double *tr_beta, double *tr_lam, double *tr_sig2, double *tr_tau, double *tr_alpha,
    uint32_t *err, double pr_a, double pr_b) {
    const size_t c = blockIdx.x;
    const Key ck{key.k0, key.k1 + (uint64_t)c};
    const size_t ring = c * (size_t)cap;
    small_chain_body<NT, L, I, true, true>(
        X, ldx, n, p, y, G, ldg, cvec, gdiag, ortho, x_lds, beta + c * p, lam + c * p, sc + c, hy,
        ck, t0, count, first_slot, slot_step, cap, tr_beta + ring * p, tr_lam + ring * p,
        tr_sig2 + ring, tr_tau + ring, tr_alpha + ring, err + c, pr_a, pr_b);
}

namespace {

// the instance for p coefficients of the single chain (batch == 0) or of the batch, as
// bb_small.hip's small_chain_instance
using SmallChainsMhKernel = decltype(&k_small_chains_mh<512, 64, 16>);
SmallChainsMhKernel small_chain_mh_instance(int batch, int p) {
    static const SmallChainsMhKernel inst[6] = {
        k_small_chain_mh<512, 64, 16>,  k_small_chain_mh<512, 32, 8>,
        k_small_chain_mh<512, 16, 8>,   k_small_chains_mh<512, 64, 16>,
        k_small_chains_mh<512, 32, 8>,  k_small_chains_mh<512, 16, 8>};
    static const bool optin = [] {
        for (SmallChainsMhKernel k : inst)
            (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kSmallXLds);
        return true;
    }();
    (void)optin;
    return inst[(batch ? 3 : 0) + (p <= 8 ? 0 : p <= 16 ? 1 : 2)];
}

}  // namespace

void small_mh_launch(int batch, int blocks, size_t shm, int x_lds, hipStream_t s,
                     const ChainDesign &d, const ChainState &c, const ChainTraces &tr,
                     const ChainRun &r) {
    small_chain_mh_instance(batch, d.p)<<<blocks, 512, shm, s>>>(
        d.X, d.ldx, d.n, d.p, d.y, d.G, d.ldg, d.cvec, d.gdiag, d.ortho, x_lds, c.beta, c.lam,
        c.sc, d.hy, Key{r.k0, r.k1}, r.t0, r.count, r.first_slot, r.slot_step, r.cap, tr.beta,
        tr.lam, tr.sig2, tr.tau, tr.alpha, c.err, r.pr_a, r.pr_b);
}

const void *small_mh_batch_kernel(int p) { return (const void *)small_chain_mh_instance(1, p); }

}  // namespace bb
