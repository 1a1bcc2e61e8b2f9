// bb_tri_mh.hip -- the fused triangle-mixture chain with alpha sampled (gfx950; opt-in,
// bb_set_tuning key 27): bb_tri.hip's chain kernels over the MH instance of the one sweep body
// (bb_tri_body.h), under the Beta prior (pr_a, pr_b) of the launch's phase.  The single chain and
// the batch's three instances (512 threads; 256 and 128 compact), which give the same bits.
#include "bb_tri_body.h"

namespace bb {

namespace {

__global__ __launch_bounds__(kTcNT) void k_tri_chain_mh(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ tVc, const double *__restrict__ tVr,
    const double *__restrict__ av, const double *__restrict__ dv, const double *__restrict__ Gf,
    const double *__restrict__ cv, int ortho, int x_lds, double *beta,
    double *u, double *omega, double *shape, DevScalars *sc, Hyper hy, int betaburn, Key key,
    uint64_t t0, int count, int first_slot, int slot_step, int cap, double *tr_beta,
    double *tr_u, double *tr_omega, double *tr_shape, double *tr_sig2, double *tr_tau,
    double *tr_alpha, uint32_t *err, double pr_a, double pr_b) {
    tri_chain_body<kTcNT, false, false, true>(
        X, ldx, n, p, y, tVc, tVr, av, dv, Gf, cv, ortho, x_lds, beta, u, omega, shape, sc, hy,
        betaburn, key, t0, count, first_slot, slot_step, cap, tr_beta, tr_u, tr_omega, tr_shape,
        tr_sig2, tr_tau, tr_alpha, err, pr_a, pr_b);
}

// K independent chains, a workgroup each, as k_tri_chains (bb_tri.hip)
template <int NT, bool COMPACT>
__global__ __launch_bounds__(NT, 2) void k_tri_chains_mh(
    const double *__restrict__ X, int ldx, int n, int p, const double *__restrict__ y,
    const double *__restrict__ tVc, const double *__restrict__ tVr,
    const double *__restrict__ av, const double *__restrict__ dv, const double *__restrict__ Gf,
    const double *__restrict__ cv, int ortho, int x_lds, double *beta,
    double *u, double *omega, double *shape, DevScalars *sc, Hyper hy, int betaburn, Key key,
    uint64_t t0, int count, int first_slot, int slot_step, int cap, double *tr_beta,
    double *tr_u, double *tr_omega, double *tr_shape, double *tr_sig2, double *tr_tau,
    double *tr_alpha, uint32_t *err, double pr_a, double pr_b) {
    const size_t c = blockIdx.x;
    const Key ck{key.k0, key.k1 + (uint64_t)c};
    const size_t ring = c * (size_t)cap;
    tri_chain_body<NT, COMPACT, true, true>(
        X, ldx, n, p, y, tVc, tVr, av, dv, Gf, cv, ortho, x_lds, beta + c * p, u + c * p,
        omega + c * p, shape + c * p, sc + c, hy, betaburn, ck, t0, count, first_slot, slot_step,
        cap, tr_beta + ring * p, tr_u + ring * p, tr_omega + ring * p, tr_shape + ring * p,
        tr_sig2 + ring, tr_tau + ring, tr_alpha + ring, err + c, pr_a, pr_b);
}

using TriChainsMhKernel = decltype(&k_tri_chain_mh);
struct TriChainsMhInstance {
    TriChainsMhKernel kern;
    int batch, nt;
    bool compact;
};

// The single chain's instance (batch == 0) or the batch's of `threads` threads (nullptr: none),
// their >64 KB LDS opt-in made once.
const TriChainsMhInstance *tri_mh_instance(int batch, int threads) {
    static const TriChainsMhInstance inst[] = {{k_tri_chain_mh, 0, kTcNT, false},
                                               {k_tri_chains_mh<kTcNT, false>, 1, kTcNT, false},
                                               {k_tri_chains_mh<256, true>, 1, 256, true},
                                               {k_tri_chains_mh<128, true>, 1, 128, true}};
    static const bool optin = [] {
        for (const TriChainsMhInstance &i : inst)
            (void)hipFuncSetAttribute((const void *)i.kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      tri_chain_shm_max(i.compact));
        return true;
    }();
    (void)optin;
    for (const TriChainsMhInstance &i : inst)
        if (i.batch == (batch != 0) && i.nt == threads) return &i;
    return nullptr;
}

}  // namespace

int tri_mh_launch(int batch, int threads, int blocks, hipStream_t s, const ChainDesign &d,
                  const ChainState &c, const ChainTraces &tr, const ChainRun &r) {
    const TriChainsMhInstance *i = tri_mh_instance(batch, threads);
    if (!i) return -1;
    int x_lds = 0;
    const size_t shm = tri_chain_shm(i->compact, d.n, d.p, &x_lds);
    i->kern<<<blocks, i->nt, shm, s>>>(
        d.X, d.ldx, d.n, d.p, d.y, d.tVc, d.tVr, d.a, d.d, d.Gf, d.cvec, d.ortho, x_lds, c.beta,
        c.u, c.lam, c.shape, c.sc, d.hy, d.betaburn, Key{r.k0, r.k1}, r.t0, r.count, r.first_slot,
        r.slot_step, r.cap, tr.beta, tr.u, tr.lam, tr.shape, tr.sig2, tr.tau, tr.alpha, c.err,
        r.pr_a, r.pr_b);
    return 0;
}

const void *tri_mh_batch_kernel(int threads) {
    const TriChainsMhInstance *i = tri_mh_instance(1, threads);
    return i ? (const void *)i->kern : nullptr;
}

}  // namespace bb
