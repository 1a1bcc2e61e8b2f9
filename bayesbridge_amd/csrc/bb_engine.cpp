// bb_engine.cpp -- host side of the MI355X BayesBridge drop-in: the Gibbs driver
// (restating Code/C/BridgeWrapper.cpp:207-313 and :434-537) over the HIP kernels of
// bb_kernels.hip, the chain batch, RCCL for column-sharded multi-GPU runs, and the engine,
// chain-batch, group and .C sampler entry points declared in include/bayesbridge.h.  The
// kernel-level entry points and the EM solver are in bb_prims.cpp; bb_host.h holds what the
// two share.
#include <dlfcn.h>

#include <chrono>
#include <cxxabi.h>
#include <cmath>
#include <cstring>
#include <atomic>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <thread>

#include "../../include/bayesbridge.h"
#include "bb_host.h"
#include "bb_ozaki.h"

using namespace bb;

namespace bb {

thread_local std::string g_last_error;
int g_device = 0;
int g_verbose = 1;

}  // namespace bb

namespace {

std::mutex g_mu;
uint64_t g_seed = 0xB4E5B41D6EULL;
uint64_t g_stream = 0;
int g_use_r_rng = 1;
// bb_debug_fail_member: member `g_debug_fail_member` of the next RCCL group run throws
// before its sweep `g_debug_fail_sweep` (test hook for the group's failure handling)
std::atomic<int> g_debug_fail_member{-1}, g_debug_fail_sweep{-1};

// R's RNG, resolved at run time when this library is loaded inside R.
struct RRng {
    void (*get)(void) = nullptr;
    void (*put)(void) = nullptr;
    double (*unif)(void) = nullptr;
    bool tried = false;
    bool ok() {
        if (!tried) {
            tried = true;
            get = (void (*)(void))dlsym(RTLD_DEFAULT, "GetRNGstate");
            put = (void (*)(void))dlsym(RTLD_DEFAULT, "PutRNGstate");
            unif = (double (*)(void))dlsym(RTLD_DEFAULT, "unif_rand");
        }
        return get && put && unif;
    }
} g_rrng;

}  // namespace

void bb::next_call_key(uint64_t *k0, uint64_t *k1, int count) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_use_r_rng && g_rrng.ok()) {
        g_rrng.get();
        uint64_t a = (uint64_t)(g_rrng.unif() * 4294967296.0);
        uint64_t b = (uint64_t)(g_rrng.unif() * 4294967296.0);
        uint64_t c = (uint64_t)(g_rrng.unif() * 4294967296.0);
        g_rrng.put();
        *k0 = (a << 32) ^ b;
        *k1 = c;
        return;
    }
    *k0 = g_seed;
    *k1 = g_stream;
    g_stream += (uint64_t)count;
}

// ---------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------
enum Phase {
    PH_PRE, PH_SCALARS, PH_LAMBDA, PH_PG, PH_OZPREP, PH_GRAM, PH_XU, PH_REDUCE, PH_FORM, PH_CHOL,
    PH_SOLVE, PH_BETA, PH_XB, PH_ALPHA, PH_NID, PH_EAPPLY, PH_END, PH_COUNT
};
// "gram" times the Gram GEMM kernel alone (k_gram, or k_oz_gemm after "ozprep" = row scales
// + residues); "reduce" is the split/slab combine (k_slab_sum or the CRT k_oz_crt); "nid" the
// near-identity decision, X u and Chebyshev recurrences, "eapply" its passes over X
// (bb_nid.hip).

// Chebyshev iterations the near-identity solve may take per sweep (bb_set_tuning key 6; 0
// turns the path off: every sweep forms the Gram and factors it)
int g_nid_kmax = 16;
// bb_set_tuning key 8: an unsharded engine decides like a shard (the host waits for each
// sweep's decision, then launches only that path: 1, the default) or launches both paths
// gated with the hint of nid_launch_count (0).  Measured at the driver's settings (round 4,
// gpurun_out/r04f_*): C3 1781 against 1746-1749 sweeps/s, C2 5840 against 5519, C5 1672
// against 1636 -- the host's wake-up and first launch cost less than the gated no-ops.
int g_nid_sync = 1;
// bb_set_tuning key 9 (testing): an engine with world == 1 that owns a communicator (a 1-rank
// RCCL comm) or belongs to an on-device shard group runs the world > 1 near-identity stage
// sequence (bound-sum exchange, k_nid_decide_from, X u and per-product exchanges), so every
// exchange call site of that protocol executes on a one-GPU box
int g_shard_proto = 0;
// bb_set_tuning key 10: the mixed-precision near-identity plan of unsharded
// dense engines: products over an fp32 copy of X with one fp64 residual pass (1, the default)
// or fp64 products only (0)
int g_nid_mixed = 1;
// bb_set_tuning key 11: the host learns a synchronous decision by polling its tag word in
// coherent host memory (1, the default) or by an event recorded behind the decision kernel
// (0).  The event's marker left the device idle ~4 us per sweep: C3 at the driver's settings
// 2010 against 1995 sweeps/s, 1000 sweeps after 100 1370 against 1367 (gpurun_out/ab_*).
int g_nid_poll = 1;
// bb_set_tuning key 17: under the synchronous protocol the split lambda launch (key 7 = 3)
// forms the decision's bound sums in its stream role, k_nid_reduce adds them and decides
// (1, the default); 2: unsharded, the launch's last stream workgroup reduces and decides too;
// 0: k_nid_sums + k_nid_reduce after the launch
int g_nid_fold = 1;
// bb_set_tuning key 24: beta of a certified near-identity sweep from the banked X'x dots and one
// pass over the fp32 copy of X (unsharded dense engines holding X32): 0 never,
// 1 where certified and the cost model says the halved pass pays (the default), 2 wherever
// certified (tests at small shapes)
int g_nid_b32 = 1;
// bb_set_tuning key 29: the residual-certified mixed plan (unsharded dense engines
// holding X32 that decide under the synchronous protocol with the polled tag): the first solve
// on a guessed interval, K2 from the fp64 residual.  0 never (the plan search of s6.6 / s6.7 bit
// for bit), 1 where the cost model says an fp32 pass is worth several launches (the default),
// 2 wherever a first solve qualifies (tests at small shapes), 2 + v the same with the guess
// factor phi = 8 / 16^v (tests: a wrong guess, the redo)
int g_nid_resid = 1;
// bb_set_tuning key 21: chain batches of at least 2 x CUs chains created from now on run the
// 256-thread instance, two chains per CU (faster in aggregate there; its chains
// match the oracle but are not bit for bit those of sequential calls)
int g_chains_packed = 0;
// bb_set_tuning key 25: stable-mixture engines and chain batches created from now on with
// 32 < p <= 128 (alpha known, Cholesky or orthogonal draw, one device) run whole sweeps in the
// fused kernels of bb_wide.hip instead of the general path
int g_chains_wide = 0;
// bb_set_tuning key 26: stable-mixture engines and chain batches created from now on with
// p <= 32 and alpha unknown (Cholesky or orthogonal draw, one device) run the fused sweeps of
// bb_small.hip with the alpha MH step inside (bb_small_mh.hip's instances, 512 threads) instead
// of the general path
int g_fused_alpha = 0;
// bb_set_tuning key 27: triangle-mixture engines and chain batches created from now on with
// p <= 32, p <= n and alpha unknown (general or orthogonal design, one device) run the fused
// sweeps of bb_tri.hip with the alpha MH step inside (bb_tri_mh.hip's instances) instead of the
// general path
int g_fused_tri_alpha = 0;
static const char *kPhaseNames[PH_COUNT] = {"pre", "scalars", "lambda", "pg", "ozprep", "gram",
                                            "xu", "reduce", "form", "chol", "solve", "beta",
                                            "xb", "alpha", "nid", "eapply", "end"};

// The sampler an engine runs (bb_engine_method exports the values; bb_config::method names the
// same ones, with AUTO = Cholesky if p <= n, else Woodbury): the p x p Cholesky draw, the dense
// Woodbury draw, the orthogonal-design draw, the triangle mixture, the sparse Woodbury draw and
// the logistic (Polya-Gamma) bridge.
enum Method { AUTO = 0, CHOL = 1, WOODBURY = 2, ORTHO = 3, TRI = 4, SPARSE = 5, LOGIT = 6 };

// The fused chain path, decided in one place: chain_plan says which kernel
// family runs a configuration, ChainPath carries that choice and dispatches on it, ChainView is
// the host's one view of a chain's state and rings.  bb_chain_kernel exports the kinds.
enum ChainKernel { CK_NONE = 0, CK_SMALL = 1, CK_WIDE = 2, CK_TRI = 3, CK_LOGIT = 4 };
// mh: the family's alpha-sampling instances run; refusal: why not (CK_NONE), for the batch
struct ChainPlan { ChainKernel kind; bool mh; const char *refusal; };

// Which fused kernel family runs `c` as a single engine (batch false) or as a chain batch, under
// the switches of bb_set_tuning keys 25, 26 and 27 (by default their current values).  No device
// is needed.  Where the batch's rule differs from the engine's, the condition reads `batch` and
// says so.  The refusals keep the order the batch reports them in.
ChainPlan chain_plan(const bb_config &c, bool batch, int wide_on = g_chains_wide,
                     int mh_on = g_fused_alpha, int tri_mh_on = g_fused_tri_alpha) {
    const bool know_alpha = c.true_alpha > 0;
    auto no = [](const char *why) { return ChainPlan{CK_NONE, false, why}; };
    if (c.n <= 0 || c.p <= 0) return no("n and p must be positive");
    if (c.world > 1) return no("a chain batch runs on one device (world == 1)");
    // batch only: an engine with world == 1 never looked at p_local
    if (batch && c.p_local > 0 && c.p_local != c.p)
        return no("a chain batch holds every column (p_local == p)");
    if (c.method == TRI) {  // bb_tri.hip; key 27: bb_tri_mh.hip's instances sample alpha
        static_assert(kTriChainMaxP == 32, "the message below says 32");
        if (c.p > kTriChainMaxP) return no("a triangle chain batch needs p <= 32");
        if (c.p > c.n) return no("a triangle chain batch needs p <= n");  // no such engine exists
        if (!know_alpha && !tri_mh_on)
            return no("a chain batch needs alpha known (true_alpha > 0)");
        return {CK_TRI, !know_alpha, nullptr};
    }
    if (c.method == LOGIT) {  // bb_logit_chain.hip, alpha known or sampled
        // batch only: the kernel has no single-chain twin, an engine keeps the general path
        if (!batch) return no("a logistic engine runs the general path");
        static_assert(kSmallChainMaxP == 32 && kLogitChainMaxN == 4096, "the messages say so");
        if (c.p > kSmallChainMaxP) return no("a logistic chain batch needs p <= 32");
        if (c.p > c.n) return no("a logistic chain batch needs p <= n");
        if (c.n > kLogitChainMaxN) return no("a logistic chain batch needs n <= 4096");
        return {CK_LOGIT, !know_alpha, nullptr};
    }
    // batch only: with ortho set an engine runs the orthogonal draw, fused, under every other
    // method value too (2, 3, 5); the batch takes methods 0 and 1 alone
    if (c.method != AUTO && c.method != CHOL && (batch || !c.ortho))
        return no("a chain batch runs the stable mixture's Cholesky or orthogonal draw (method 0 or "
                  "1), the triangle mixture (method 4) or the logistic bridge (method 6)");
    if (wide_on) {  // key 25: bb_wide.hip's kernel above 32
        static_assert(kWideChainMaxP == 128, "the message below says 128");
        if (c.p > kWideChainMaxP) return no("a chain batch needs p <= 128 (wide fused chains on)");
    } else if (c.p > kSmallChainMaxP) {
        return no("a chain batch needs p <= 32");
    }
    if (c.p > c.n && !c.ortho) return no("a chain batch needs p <= n (or the orthogonal design)");
    // key 26: bb_small_mh.hip's instances sample alpha, at p <= 32 alone
    if (!know_alpha && !(mh_on && c.p <= kSmallChainMaxP))
        return no("a chain batch needs alpha known (true_alpha > 0)");
    return {c.p <= kSmallChainMaxP ? CK_SMALL : CK_WIDE, !know_alpha, nullptr};
}

// A chain's state and trace rings as the kernels take them, with the host's widths: p
// coefficients, `cap` ring slots, the logistic omega's n rows.  at(c): chain c of a batch.
struct ChainView {
    ChainState st{};
    ChainTraces tr{};
    int p = 0, cap = 1, n = 0;
    double *omega = nullptr;

    ChainView at(int c) const {
        ChainView v = *this;
        auto skip = [](std::initializer_list<double **> qs, size_t k) {
            for (double **q : qs)
                if (*q) *q += k;  // an array the family does not have stays null
        };
        skip({&v.st.beta, &v.st.lam, &v.st.u, &v.st.shape}, (size_t)c * p);
        skip({&v.tr.beta, &v.tr.lam, &v.tr.u, &v.tr.shape}, (size_t)c * cap * p);
        skip({&v.tr.sig2, &v.tr.tau, &v.tr.alpha}, (size_t)c * cap);
        skip({&v.omega}, (size_t)c * n);
        v.st.sc += c;
        v.st.err += c;
        return v;
    }
    SummaryRing ring() const {
        return {.beta = tr.beta, .sig2 = tr.sig2, .tau = tr.tau, .alpha = tr.alpha, .p = p,
                .cap = cap};
    }
};

// The plan's kind as an engine or a batch stores it (a batch: with its instance), and every
// choice that follows from it.  A new family adds its case to each switch.
struct ChainPath {
    ChainKernel kind = CK_NONE;
    int packed = 0;     // small batches: the 256-thread instance (key 21 and K >= 2 CUs)
    int threads = 512;  // triangle batches: the instance, by its threads per workgroup

    // `count` sweeps of the K chains of a batch, or (K == 0) of an engine's own chain
    void launch(hipStream_t s, int K, const ChainDesign &d, const ChainView &v,
                const ChainRun &r) const {
        const char *none = nullptr;  // the family has no instance for this shape
        if (kind == CK_SMALL) {
            K ? launch_small_chains(s, K, packed, d, v.st, v.tr, r)
              : launch_small_chain(s, d, v.st, v.tr, r);
        } else if (kind == CK_WIDE) {
            if ((K ? launch_wide_chains(s, K, d, v.st, v.tr, r)
                   : launch_wide_chain(s, d, v.st, v.tr, r)) != 0)
                none = K ? "no wide chain-batch instance for this p"
                         : "no wide fused chain instance for this p";
        } else if (kind == CK_TRI) {
            if (K == 0) launch_tri_chain(s, d, v.st, v.tr, r);
            else if (launch_tri_chains(s, K, threads, d, v.st, v.tr, r) != 0)
                none = "no triangle chain-batch instance of that many threads";
        } else if (kind == CK_LOGIT && K) {
            if (launch_logit_chains(s, K, d, v.st, v.tr, r, v.omega) != 0)
                none = "no logistic chain-batch instance for this design";
        } else {
            none = "no fused chain kernel on this path";
        }
        if (none) throw HipError(none);
    }
    // workgroups of the batch's instance resident on one CU (-1: the query failed)
    int resident_per_cu(int n, int p, int mh) const {
        return kind == CK_TRI     ? tri_chains_resident_per_cu(n, p, threads, mh)
               : kind == CK_LOGIT ? logit_chains_resident_per_cu(n, p, mh)
               : kind == CK_WIDE  ? wide_chains_resident_per_cu(p)
                                  : small_chains_resident_per_cu(n, p, packed, mh);
    }
    // threads per workgroup of the batch's instance
    int block_threads(int p) const {
        if (kind == CK_WIDE) return wide_chains_threads(p);
        return kind == CK_TRI ? threads : packed ? 256 : 512;
    }
    // Sweeps per launch, and per interrupt poll, of a .C call.  BridgeWrapper.cpp:273-275,
    // 295-297 poll every 10 sweeps.  A fused launch runs a whole block at ~15-30 us per sweep,
    // so it polls every 50 (< 2 ms) and pays the launch and LDS-staging prologue once per 50
    // sweeps instead of per 10.  The wide kernel's sweeps are ~100 us: kWideBlock of them keep
    // the poll near the general path's 10 sweeps in time.
    int block() const { return kind == CK_NONE ? 10 : kind == CK_WIDE ? kWideBlock : 50; }
};

struct bb_engine {
    bb_config cfg{};
    int n = 0, p = 0, p_loc = 0, n_pad = 0, p_pad = 0;
    // p x p systems (methods 1, 6): factored at round_up(p, 64) inside the p_pad-strided
    // buffers, so a p = 64 design is one block step, not p_pad / 64 = 4
    int chol_m = 0;
    Method method = AUTO;
    int group = 1;
    ChainPath path;  // whole sweeps in one launch: chain_plan's kernel family at creation
    SparseDesign spd;  // method 5: CSC/CSR design and the Gram pair list
    Hyper hy{};
    hipStream_t stream = nullptr;
    std::vector<void *> owned;

    double *X = nullptr, *y = nullptr;
    double *beta = nullptr, *lam = nullptr, *D = nullptr, *u = nullptr;
    DevScalars *sc = nullptr;
    uint32_t *err = nullptr;
    double *xb_part = nullptr, *red1 = nullptr;
    double *red3 = nullptr;  // sharded alpha MH: [S(alpha_new), S(alpha_old)]
    int nparts = 0, nbS = 0;
    bool xb_stale = false;  // a fused run left the X beta partials behind beta
    // woodbury
    double *slabs = nullptr, *xu_part = nullptr, *red2 = nullptr, *M = nullptr, *w = nullptr,
           *Wd = nullptr;
    unsigned int *flags = nullptr;
    int S = 1;
    size_t slab_stride = 0;
    // Ozaki-II Gram (gram_mode 1)
    int n_oz = 0, oz_b = 0, oz_S = 1;
    double *oz_xmax = nullptr, *oz_rscale = nullptr;
    double *oz_rowmax = nullptr;  // per chunk-group row maxima (launch_oz_scale scratch)
    int *oz_escale = nullptr;
    int8_t *oz_R = nullptr, *oz_P = nullptr;
    // logistic: X' resident for X'Omega X, omega, kappa = y - 1/2, the per-sweep Gram
    double *Xt = nullptr, *omega = nullptr, *kappa = nullptr, *Gw = nullptr;
    // chol / ortho
    double *G = nullptr, *cvec = nullptr, *A = nullptr, *Y2 = nullptr, *W2 = nullptr,
           *gdiag = nullptr;
    // triangle mixture: design basis (bb_tri.hip), omega in lam, shape in D, u in u
    double *tVc = nullptr, *tVr = nullptr, *tri_a = nullptr, *tri_d = nullptr,
           *tri_G = nullptr;
    double *tr_u = nullptr, *tr_shape = nullptr;
    std::vector<double> h_tV, h_a, h_d;
    // traces
    double *tr_beta = nullptr, *tr_lam = nullptr, *tr_sig2 = nullptr, *tr_tau = nullptr,
           *tr_alpha = nullptr;
    int cap = 1;
    // near-identity solve of the Woodbury system (bb_nid.hip): column norms,
    // the device decision word, Chebyshev vectors (x is w), E-apply partials, the host-mapped
    // eps of the latest decided sweep (the launch hint) and the enqueue throttle
    double *cn = nullptr;
    NidState *nid = nullptr;
    double *ch_r = nullptr, *ch_d = nullptr, *ea_part = nullptr, *sp_s = nullptr,
           *nid_xu = nullptr;
    double *eps_host = nullptr;  // ring of kNidRing: eps of sweep q in slot q % kNidRing
    // the mixed-precision plan (unsharded dense engines): X rounded to fp32 (n_pad x p_loc,
    // ld n_pad; nullptr when not held), the right-hand side kept for the residual pass, and the
    // correction iterates the latest sweep's decision asked for (0: the fp64 plan)
    float *X32 = nullptr;
    double *ch_b = nullptr;
    int nid_k2 = 0;
    // the fp32 beta pass (engines holding X32): the banked dots X_j' x_{K-1}
    // (p_loc), the mixed plan's correction and the summed X u (n_pad), and whether the latest
    // decision set NidState::b32
    double *gb = nullptr, *ch_c = nullptr, *ch_xu = nullptr;
    bool nid_b32 = false;
    // the residual-certified plan: the partials of |b|^2 and |r|^2 (nid_sqn of
    // each), whether the latest decision took it, and the second decisions launched with a tag
    double *nid_sq = nullptr;
    int nid_sqn = 0;
    bool nid_resid = false;
    unsigned long long nid_kseq = 0;
    double nid_cost[3] = {0.0, 0.0, 0.0};  // NidState c64, c32, cstep (s)
    int ea_parts = 1;
    int nid_kmax = 0;  // iterations beyond which the Gram + Cholesky path is cheaper (model)
    double lambda_x = 0.0;  // certified lambda_max(X X') bound (0: none)
    // decided-sweep events (after the decision of sweep q, slot q % kNidRing) and the number of
    // Woodbury sweeps enqueued since init_state (q)
    hipEvent_t nid_ev[8] = {};
    long nid_seq = 0;
    // column shards (world > 1): the bound sums exchanged before the decision, the reduced
    // X u / E d vector, the decision event the host waits on, whether this sweep took the
    // Chebyshev path, and membership of an on-device shard group (its exchanges are the
    // group's reduce; RCCL ranks and RCCL group members exchange through their communicator)
    double *nid_red = nullptr, *nid_sum = nullptr, *nid_wg = nullptr;
    hipEvent_t nid_sev = nullptr;
    bool nid_only = false;
    bool group_member = false;
    int nid_last = -1;  // the previous sweep's decided K (-1: none since init_state)
    // communicator (own_comm false: lent by an RCCL shard group, which destroys it)
    ncclComm_t comm = nullptr;
    bool own_comm = true;
    // timing: per-sweep event marks at phase starts, on the engine stream
    bool timing = false;
    int timing_level = 2;  // 1: one phase's bracket only (timed_phase), 2: every phase
    int timed_phase = PH_GRAM;
    int timing_stride = 1;  // level 1: bracket every timing_stride-th sweep
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::vector<std::pair<int, int>>> sweep_marks;  // (phase, event)
    size_t ev_next = 0;

    void mark(int phase) {
        if (!timing) return;
        // level 1: only the timed phase's bracket (its start and the next mark), so a timed
        // run carries two events per sweep instead of one per phase
        if (timing_level == 1) {
            if ((sweep_marks.size() - 1) % (size_t)timing_stride != 0) return;
            const bool open = !sweep_marks.back().empty() &&
                              sweep_marks.back().back().first == timed_phase;
            if (phase != timed_phase && !open) return;
        }
        int e0 = ev();
        HIPCHECK(hipEventRecord(ev_pool[e0], stream));
        sweep_marks.back().push_back({phase, e0});
    }

    ~bb_engine() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (comm && own_comm) ncclCommDestroy(comm);
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        for (auto e : nid_ev)
            if (e) (void)hipEventDestroy(e);
        if (nid_sev) (void)hipEventDestroy(nid_sev);
        if (eps_host) (void)hipHostFree(eps_host);
        for (void *q : owned) (void)hipFree(q);
        if (stream) (void)hipStreamDestroy(stream);
    }

    int ev() {
        if (ev_next == ev_pool.size()) {
            hipEvent_t e;
            HIPCHECK(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
        return (int)ev_next++;
    }

    void allreduce(double *buf, size_t count) {
        if (cfg.world <= 1 && !comm) return;  // a 1-rank communicator still runs (testing)
        if (!comm) throw HipError("world > 1 but no communicator (call bb_engine_comm_init)");
        NCCLCHECK(ncclAllReduce(buf, buf, count, ncclFloat64, ncclSum, comm, stream));
    }

    double *slot_ptr(double *base, int slot, int stride) {
        if (slot < 0 || base == nullptr) return nullptr;
        return base + (size_t)(slot % cap) * stride;
    }

    bool woodbury() const { return method == WOODBURY || method == SPARSE; }
    bool dense() const { return method == WOODBURY; }  // Woodbury over the dense X
    bool sparse() const { return method == SPARSE; }   // Woodbury over the CSC / CSR X
    bool ortho() const { return method == ORTHO; }
    bool tri() const { return method == TRI; }
    bool logit() const { return method == LOGIT; }
    bool pxp() const { return method == CHOL || method == LOGIT; }  // factors a p x p system

    // the near-identity path: an unsharded Woodbury engine (a one-member RCCL group included:
    // nothing is exchanged) decides on the device against a launch hint; column shards
    // (world > 1, exchanging through a communicator or an on-device group) decide from the
    // reduced bound sums and the host waits for that decision (nid_sync)
    bool nid_enabled() const {
        return nid != nullptr && (cfg.world == 1 || comm != nullptr || group_member) &&
               std::min(g_nid_kmax, nid_kmax) > 0;
    }
    // this engine runs the column-shard protocol of the near-identity solve (exchanged bound
    // sums, the decision from them, exchanged X u and products): world > 1, or world == 1 with
    // a communicator / in a group when forced for testing (g_shard_proto)
    bool sharded() const {
        return cfg.world > 1 || (g_shard_proto && (comm != nullptr || group_member));
    }
    bool nid_sync() const { return (sharded() || g_nid_sync) && nid_enabled(); }
    // the mixed-precision plan may be chosen by this engine's decision: an unsharded dense
    // engine that holds X32 (shards and shard-group members decide the fp64 plan only, so
    // every rank runs the same collectives)
    bool mixed_ok() const {
        return X32 != nullptr && g_nid_mixed && !sharded() && !group_member && dense();
    }
    // the sweep's decision may set b32: the engine can run the mixed plan (so it holds X32 and
    // keeps b), decides under the synchronous protocol (the host learns the flag with the
    // decision) and has the fused beta pass's shape
    bool b32_ok() const { return gb != nullptr && g_nid_b32 && mixed_ok() && nid_sync(); }
    // the decision may take the residual-certified plan: a mixed-plan engine whose host polls
    // the decision tags; by default only where an fp32 pass costs more than four step launches
    // (the plan adds a launch and a second host wake-up to save such passes: C3's shape, not
    // the 2048 x 6250 and smaller designs whose tests pin the a-priori plan and its beta32 rule)
    bool resid_ok() const {
        return nid_sq != nullptr && g_nid_resid && g_nid_poll && mixed_ok() && nid_sync() &&
               (g_nid_resid >= 2 || nid_cost[1] > 4.0 * nid_cost[2]);
    }
    int allow_mask() const {
        return (mixed_ok() ? kAllowMixed : 0) |
               (b32_ok() ? kAllowBeta32 | (g_nid_b32 == 2 ? kBeta32AnyCost : 0) : 0) |
               (resid_ok() ? kAllowResid | (g_nid_resid >= 2 ? kResidAnyCost : 0) |
                                 (std::max(g_nid_resid - 2, 0) << kResidPhiShift)
                           : 0);
    }
    double *bank() const { return b32_ok() ? gb : nullptr; }
    Beta32Vecs b32_vecs() const {
        return b32_ok() ? Beta32Vecs{ch_c, ch_b, ch_xu, xb_part} : Beta32Vecs{};
    }
    // the exchanged vectors are single n-vectors on a shard; an unsharded engine in the
    // synchronous mode reads the partials directly
    bool nid_vec() const { return sharded() || sparse(); }

    // Cost model of the two exact solves, from the round-3/4 measured rates:
    // a Chebyshev solve of K iterates reads X K times (the X u pass and K - 1 products, ~6 TB/s
    // dense, ~3 TB/s for the sparse gathers, plus ~10 us of launches and the recurrence per
    // pass); the Gram + Cholesky path costs the Gram (Ozaki int8 GEMM at ~2.6 POP/s and its
    // 24 B per X element of residue traffic at ~5 TB/s; the fp64 MFMA Gram at ~33 TF/s; the
    // sparse pair stream at ~4 TB/s) plus ~19 us per 64-column block step of the factor and
    // solve.  Returns the largest K for which the Chebyshev solve is the cheaper one.
    int nid_kmax_model() const {
        double t_pass, t_chol;
        const double steps = n_pad / 64.0;
        if (sparse()) {
            t_pass = 24.0 * (double)spd.nnz / 3.0e12 + 10e-6;
            t_chol = 10.0 * (double)spd.pairs / 4.0e12 + steps * 21e-6 + 60e-6;
        } else {
            t_pass = 8.0 * n_pad * (double)p_loc / 6.0e12 + 10e-6;
            const double gram = cfg.gram_mode == 1
                ? 16.0 * (double)n_pad * n_pad * p_pad / 2.6e15 + 24.0 * (double)n_pad * p_pad / 5.0e12
                : 2.0 * (double)n_pad * n_pad * p_pad / 33e12;
            t_chol = gram + steps * 19e-6 + 40e-6;
        }
        if (cfg.world > 1) {
            // shards: an n-vector all-reduce per pass; the packed Gram's all-reduce (~100 GB/s
            // effective over xGMI rings) and the replicated factor on the other side
            t_pass += 25e-6;
            t_chol += 8.0 * (double)red2_count() / 100e9 + 25e-6;
        }
        return (int)std::min(64.0, std::floor(t_chol / t_pass));
    }

    // Chebyshev iterations to launch for Woodbury sweep q: from eps of sweep q - kNidLag
    // (host-mapped ring; the host waits for that sweep's decision, so it stays at most
    // kNidLag sweeps ahead of the device -- no bubble, the device has that many queued) with
    // an 8x growth margin; the first kNidLag sweeps after init_state: the maximum; beyond the
    // maximum: 0 (only the Gram + Cholesky path is launched).  The device decides sweep q
    // itself (k_nid_reduce): K iterates needed > launched makes it take the Gram + Cholesky
    // path, never a wrong w.  The hint is eps of a fixed earlier sweep, so the path a sweep
    // takes -- and its bits -- depend only on the chain, not on host / device timing.
    static constexpr int kNidRing = 8, kNidLag = 3;
    int nid_launch_count() {
        const int kmax = std::min(g_nid_kmax, nid_kmax);
        if (nid_seq < kNidLag) return kmax;
        const long q = nid_seq - kNidLag;
        wait_event(nid_ev[q % kNidRing]);
        const double h = ((volatile double *)eps_host)[q % kNidRing];
        if (!(h >= 0.0)) return kmax;
        return cheb_iterations(8.0 * h, kmax, kNidTol);
    }

    // decision kernel of a Woodbury sweep (eps is tracked even when only the Gram + Cholesky
    // path is launched, so the hint follows the chain back into the near-identity regime)
    int nid_begin(int kl) {
        if (!nid_enabled()) return 0;
        mark(PH_NID);
        const long q = nid_seq++;
        launch_nid_sums(stream, D, cn, p_loc, sc, nid, kl, kl > 0, 1, nid_wg, nid_red,
                        eps_dev + q % kNidRing);
        hipEvent_t &ev = nid_ev[q % kNidRing];
        if (!ev) HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(ev, stream));
        return kl;
    }
    double *eps_dev = nullptr;  // device view of eps_host

    // the Chebyshev solve (kl iterations launched, the device runs mode of them); x is w
    void nid_solve(uint64_t t, int kl) {
        mark(PH_NID);
        if (sparse())
            launch_cheb_init(stream, nid_xu, 1, n, n_pad, y, sc, cfg.seed, cfg.stream, t, nid, w,
                             ch_r, ch_d);
        else
            launch_cheb_init(stream, nid_xu, xu_fused ? xu_fused : ea_parts, n, n_pad, y, sc,
                             cfg.seed, cfg.stream, t, nid, w, ch_r, ch_d);
        for (int j = 1; j < kl; ++j) {
            mark(PH_EAPPLY);
            if (sparse())
                launch_sp_eapply(stream, spd.colptr, spd.rowidx, spd.cval, spd.rowptr, spd.colidx,
                                 spd.rval, p_loc, n_pad, D, ch_d, nid, j, sp_s, ea_part);
            else
                launch_eapply(stream, X, n_pad, n_pad, p_loc, D, ch_d, nid, j, ea_part);
            mark(PH_NID);
            launch_cheb_step(stream, ea_part, sparse() ? 1 : ea_parts, n_pad, sc, nid, j, w,
                             ch_r, ch_d);
        }
    }

    // ---- column shards (nid_sync): the stages between the exchanges of a Woodbury sweep ----
    static constexpr int kNidRed = kNidTS + 2;
    // this shard's bound sums into nid_red (exchanged: kNidRed doubles); an unsharded engine
    // decides in the same launch (its sums need no exchange)
    // folded: the split lambda launch formed the sums (1: its nstream partials in nid_wg, reduced
    // here; 2: reduced and decided as well)
    void nidx_partials(int folded = 0, int nstream = 0) {
        mark(PH_NID);
        if (folded == 2) return;
        if (folded == 1 && sharded())
            launch_nid_reduce(stream, nid_wg, nstream, sc, nid, nid_red);
        else if (folded == 1)
            launch_nid_reduce(stream, nid_wg, nstream, sc, nid, nid_red,
                              std::min(g_nid_kmax, nid_kmax), eps_dev + kNidRing,
                              allow_mask(), ++nid_dseq);
        else if (sharded())
            launch_nid_sums(stream, D, cn, p_loc, sc, nid, 0, 0, 0, nid_wg, nid_red, nullptr);
        else
            launch_nid_sums_decide(stream, D, cn, p_loc, sc, nid, std::min(g_nid_kmax, nid_kmax),
                                   nid_wg, nid_red, eps_dev + kNidRing, allow_mask(),
                                   ++nid_dseq);
    }
    // the decision from the reduced sums (identical on every rank), then wait for it
    void nidx_decide_launch() {
        if (sharded())
            launch_nid_decide_from(stream, nid_red, sc, std::min(g_nid_kmax, nid_kmax), nid,
                                   eps_dev + kNidRing, ++nid_dseq);
        if (g_nid_poll) return;
        if (!nid_sev) HIPCHECK(hipEventCreateWithFlags(&nid_sev, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(nid_sev, stream));
    }
    int nidx_decide_read() {
        int mode, k2;
        if (g_nid_poll) {
            const unsigned long long tag = wait_tag(nid_dseq);
            mode = (int)((tag >> 8) & 0x7f);
            nid_resid = ((tag >> 15) & 1) != 0;  // mode <= 64: resid rides in its bit 7
            k2 = (int)(tag & 0xff);
        } else {
            nid_resid = false;
            wait_event(nid_sev);
            mode = (int)((volatile double *)eps_host)[kNidRing + 1];
            k2 = (int)((volatile double *)eps_host)[kNidRing + 2];
        }
        nid_b32 = b32_ok() && (k2 & 128) != 0;  // b32 rides in bit 7 of k2 (nid_finish)
        k2 &= 127;
        nid_k2 = mixed_ok() ? k2 : 0;
        nid_only = mode > 0;
        nid_last = mode;
        return mode;
    }
    // Poll the decision's tag word (host2[3]: seq << 16 | mode << 8 | k2, one 64-bit store by
    // the decision kernel into coherent host memory) until it carries decision seq.  Every
    // 1024 polls the stream is queried: a device error surfaces as the HIP error, and a drained
    // stream without the tag is an error (never a silent wrong path); a shard-group member
    // gives up when another member failed (wait_event).
    // slot 4 / shift 24: the residual-certified plan's second decision (k_nid_k2)
    unsigned long long wait_tag(unsigned long long seq, int slot = 3, int shift = 16) {
        const unsigned long long *tp = (const unsigned long long *)(eps_host + kNidRing + slot);
        const unsigned long long want = seq & (~0ull >> shift);
        for (long spin = 0;; ++spin) {
            const unsigned long long v = __atomic_load_n(tp, __ATOMIC_ACQUIRE);
            if ((v >> shift) == want) return v;
            if ((spin & 1023) != 1023) {
                __builtin_ia32_pause();
                continue;
            }
            if (stop && stop->load(std::memory_order_relaxed))
                throw HipError("stopped: another member of the shard group failed");
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                const unsigned long long w = __atomic_load_n(tp, __ATOMIC_ACQUIRE);
                if ((w >> shift) == want) return w;
                throw HipError("near-identity decision tag not written by the drained stream");
            }
            if (q != hipErrorNotReady) HIPCHECK(q);
            if (spin > 65536) std::this_thread::yield();
        }
    }
    unsigned long long nid_dseq = 0;  // decisions launched with a tag
    // Block the host until ev completes.  A member of an RCCL group (stop != nullptr) polls
    // instead, so that it gives up when another member failed: that member's all-reduces are
    // never posted, so an event behind them never completes (the group then aborts the
    // communicators once every member thread has returned, bb_group_run).
    void wait_event(hipEvent_t ev) {
        if (!stop) {
            HIPCHECK(hipEventSynchronize(ev));
            return;
        }
        for (long spin = 0;; ++spin) {
            const hipError_t q = hipEventQuery(ev);
            if (q == hipSuccess) return;
            if (q != hipErrorNotReady) HIPCHECK(q);
            if (stop->load(std::memory_order_relaxed))
                throw HipError("stopped: another member of the shard group failed");
            if (spin > 64) std::this_thread::yield();
        }
    }
    // this shard's X u into nid_sum (exchanged: n_pad)
    void nidx_xu() {
        mark(PH_NID);
        if (sparse()) {
            launch_sp_nid_xu(stream, spd.rowptr, spd.colidx, spd.rval, n_pad, u, nid, nid_sum);
        } else {
            if (!xu_fused) launch_nid_xu(stream, X, n_pad, u, p_loc, n_pad, nid, nid_xu);
            if (nid_vec())
                launch_part_sum(stream, nid_xu, xu_fused ? xu_fused : ea_parts, n_pad, nid_sum);
        }
    }
    void nidx_init(uint64_t t) {
        if (nid_vec())
            launch_cheb_init(stream, nid_sum, 1, n, n_pad, y, sc, cfg.seed, cfg.stream, t, nid,
                             w, ch_r, ch_d);
        else
            launch_cheb_init(stream, nid_xu, xu_fused ? xu_fused : ea_parts, n, n_pad, y, sc,
                             cfg.seed, cfg.stream, t, nid, w, ch_r, ch_d,
                             mixed_ok() ? ch_b : nullptr, b32_ok() ? ch_xu : nullptr,
                             resid_ok() ? nid_sq : nullptr);
    }
    // the mixed plan's residual pass, restart and correction solve (k2 iterates), after the
    // first solve's products
    void nidx_mixed_tail(int k2) {
        if (nid_resid) return nidx_resid_tail();
        const Beta32Vecs bv = b32_vecs();
        mark(PH_EAPPLY);
        launch_eapply(stream, X, n_pad, n_pad, p_loc, D, w, nid, 0, ea_part, X32, 2, bank());
        mark(PH_NID);
        launch_cheb_restart(stream, ea_part, ea_parts, n_pad, sc, nid, ch_b, w, ch_r, ch_d, &bv);
        for (int j = 1; j < k2; ++j) {
            mark(PH_EAPPLY);
            launch_eapply(stream, X, n_pad, n_pad, p_loc, D, ch_d, nid, j, ea_part, X32, 3);
            mark(PH_NID);
            launch_cheb_step(stream, ea_part, ea_parts, n_pad, sc, nid, j, w, ch_r, ch_d, 2,
                             &bv);
        }
    }
    // The same tail on a residual-certified sweep: the residual pass, the
    // restart and the second decision, then -- before the host waits for that decision -- the
    // correction's first product and step (they return at once unless the device's K2 >= 2, as
    // the speculative first product of solve_schedule does); after it the remaining K2 - 2
    // products, or the redo: the sweep's a-priori plan from x = 0 and the stored b.
    void nidx_resid_tail() {
        const Beta32Vecs bv = b32_vecs();
        const int gb_ = cheb_sq_parts(n_pad, xu_fused ? xu_fused : ea_parts);
        const int gr_ = cheb_sq_parts(n_pad, ea_parts);
        mark(PH_EAPPLY);
        launch_eapply(stream, X, n_pad, n_pad, p_loc, D, w, nid, 0, ea_part, X32, 2, bank());
        mark(PH_NID);
        launch_cheb_restart(stream, ea_part, ea_parts, n_pad, sc, nid, ch_b, w, ch_r, ch_d, &bv,
                            nid_sq + nid_sqn);
        launch_nid_k2(stream, nid_sq, gb_, nid_sq + nid_sqn, gr_, std::min(g_nid_kmax, nid_kmax),
                      sc, nid, &bv, w, n_pad,
                      (unsigned long long *)(eps_dev + kNidRing + 4), ++nid_kseq);
        auto correction = [&](int j) {
            mark(PH_EAPPLY);
            launch_eapply(stream, X, n_pad, n_pad, p_loc, D, ch_d, nid, j, ea_part, X32, 3);
            mark(PH_NID);
            launch_cheb_step(stream, ea_part, ea_parts, n_pad, sc, nid, j, w, ch_r, ch_d, 2,
                             &bv);
        };
        correction(1);
        const unsigned long long tag = wait_tag(nid_kseq, 4, 24);
        const int mode = (int)((tag >> 8) & 0xff), k2 = (int)(tag & 0x7f);
        nid_b32 = b32_ok() && (tag & 128) != 0;
        nid_k2 = k2;
        nid_last = mode;
        nid_resid = false;
        if (((tag >> 16) & 1) == 0) {
            for (int j = 2; j < k2; ++j) correction(j);
            return;
        }
        launch_nid_redo(stream, nid, ch_b, n_pad, w, ch_r, ch_d);
        for (int j = 1; j < mode; ++j) {
            nidx_eapply(j);
            nidx_step(j);
        }
        if (k2 > 0) nidx_mixed_tail(k2);
    }
    // this shard's E d of step j into nid_sum (exchanged: n_pad)
    void nidx_eapply(int j) {
        mark(PH_EAPPLY);
        if (sparse()) {
            launch_sp_eapply(stream, spd.colptr, spd.rowidx, spd.cval, spd.rowptr, spd.colidx,
                             spd.rval, p_loc, n_pad, D, ch_d, nid, j, sp_s, nid_sum);
        } else {
            launch_eapply(stream, X, n_pad, n_pad, p_loc, D, ch_d, nid, j, ea_part,
                          mixed_ok() ? X32 : nullptr, 0, bank());
            if (nid_vec()) launch_part_sum(stream, ea_part, ea_parts, n_pad, nid_sum);
        }
    }
    void nidx_step(int j) {
        mark(PH_NID);
        if (nid_vec())
            launch_cheb_step(stream, nid_sum, 1, n_pad, sc, nid, j, w, ch_r, ch_d);
        else {
            const Beta32Vecs bv = b32_vecs();
            launch_cheb_step(stream, ea_part, ea_parts, n_pad, sc, nid, j, w, ch_r, ch_d, 1, &bv);
        }
    }
    // X beta of the current beta into the partials k_pre sums next
    void xbeta() {
        xb_stale = false;
        if (sparse()) {
            launch_sp_rows(stream, spd.rowptr, spd.colidx, spd.rval, n_pad, beta, nullptr,
                           xb_part, nullptr);
            nparts = 1;
        } else {
            launch_xv(stream, X, n_pad, beta, p_loc, n_pad, xb_part);
            nparts = xv_chunks(p_loc, n_pad);
        }
    }

    // the two halves of the tau / sig2 / alpha draw, around the exchange of red1
    void pre() {
        if (xb_stale) xbeta();
        launch_pre(stream, xb_part, nparts, n_pad, beta, p_loc, sc, red1, nbS);
    }
    void scalars(uint64_t t, int slot, int tau_only) {
        launch_scalars(stream, red1, nbS, y, n, p, sc, hy, cfg.seed, cfg.stream, t,
                       slot_ptr(tr_tau, slot, 1), slot_ptr(tr_sig2, slot, 1),
                       slot_ptr(tr_alpha, slot, 1), tau_only, err);
    }

    // The phases of a sweep between its exchange points, as sweep_schedule (below) orders them.
    void phase_a(uint64_t t) {
        (void)t;
        if (timing) sweep_marks.emplace_back();
        mark(PH_PRE);
        pre();
    }

    // this shard's (or the whole) Gram X D X' with X u into red2 (packed upper triangle, then
    // the n-vector); gate: the near-identity decision word (its kernels skip on mode != 0)
    void wb_gram(const int *gate) {
        if (sparse()) {
            mark(PH_GRAM);
            spd.gram(stream, D, u, red2, red2 + tri_count(n_pad), gate);
            return;
        }
        if (cfg.gram_mode == 1) {
            mark(PH_OZPREP);
            launch_oz_scale(stream, D, p_pad, oz_xmax, n_oz, oz_b, oz_rowmax, oz_rscale,
                            oz_escale, gate);
            // the residue pass over X also forms the X u partials
            launch_oz_residues(stream, X, n_pad, n_pad, n_oz, p_pad, D, oz_rscale, oz_R, u,
                               xu_part, gate);
            mark(PH_GRAM);
            launch_oz_gemm(stream, oz_R, n_oz, p_pad, oz_S, oz_P, 0, kOzLeadDefault, -1, gate);
        } else {
            mark(PH_GRAM);
            launch_gram(stream, X, n_pad, D, n_pad, p_pad, S, slabs, n_pad, slab_stride, gate);
            mark(PH_XU);
            launch_xv(stream, X, n_pad, u, p_pad, n_pad, xu_part, gate);
        }
        mark(PH_REDUCE);
        if (cfg.gram_mode == 1)
            launch_oz_crt(stream, oz_P, oz_S, n_oz, n_pad, oz_escale, xu_part,
                          oz_xu_parts(p_pad, n_oz), red2, gate);
        else
            launch_slab_sum(stream, slabs, S, slab_stride, n_pad, xu_part, xv_chunks(p_pad, n_pad),
                            red2, 1, gate);
    }

    void phase_b(uint64_t t, int slot) {
        mark(PH_SCALARS);
        scalars(t, slot, 0);
        double *trl = slot_ptr(tr_lam, slot, p_loc);
        mark(PH_LAMBDA);
        if (woodbury()) {
            const bool sync = nid_sync();
            const int kl = (!sync && nid_enabled()) ? nid_launch_count() : 0;
            // a sweep that may take the Chebyshev path draws lambda and forms the X u partials
            // in one launch (k_lambda_xu, dense); under the synchronous protocol unless the
            // previous sweep took the factor (then X u would be streamed for nothing: the
            // residue pass forms it; a sweep that turns back to the Chebyshev path streams X u
            // in its own pass)
            xu_fused = 0;
            int folded = 0;
            if (dense() && (sync ? nid_last != 0 : kl > 0)) {
                // under the synchronous protocol the split launch also forms the bound sums
                // (and, unsharded, decides): k_nid_sums / k_nid_reduce are not launched
                NidFold fold;
                if (sync && g_nid_fold) {
                    fold.cn = cn;
                    fold.wg_part = nid_wg;
                    fold.cnt = lam_sync + lambda_xs_sync_words(p_pad);
                    fold.decide = (!sharded() && g_nid_fold == 2) ? 1 : 0;
                    fold.k_launched = std::min(g_nid_kmax, nid_kmax);
                    fold.allow_mixed = allow_mask();
                    fold.nid = nid;
                    fold.red = nid_red;
                    fold.host2 = eps_dev + kNidRing;
                    fold.tag_seq = nid_dseq + 1;
                }
                xu_fused = launch_lambda_xu(stream, beta, p_loc, p_pad, (uint64_t)cfg.j0, sc,
                                            cfg.seed, cfg.stream, t, lam, D, u, trl, err, X,
                                            n_pad, n_pad, nid_xu, lam_sync, ++lam_ep, &fold,
                                            &folded);
                if (folded == 2) ++nid_dseq;
            }
            if (!xu_fused)
                launch_lambda(stream, beta, p_loc, p_pad, (uint64_t)cfg.j0, sc, cfg.seed,
                              cfg.stream, t, LAMBDA_WOODBURY, group, lam, D, u, trl, err);
            ++(xu_fused ? n_lambda_xu : n_lambda_alone);
            nid_only = false;
            nid_b32 = false;
            if (sync) {
                // a shard: the bound sums now, the path after their exchange (solve_schedule)
                nid_kl = 0;
                nidx_partials(folded, xu_fused);
                return;
            }
            nid_kl = nid_begin(kl);
            wb_gram(nid_kl ? &nid->mode : nullptr);
            if (nid_kl && !xu_fused) {
                mark(PH_NID);
                if (sparse())
                    launch_sp_nid_xu(stream, spd.rowptr, spd.colidx, spd.rval, n_pad, u, nid,
                                     nid_xu);
                else
                    launch_nid_xu(stream, X, n_pad, u, p_loc, n_pad, nid, nid_xu);
            }
        } else if (logit()) {
            // omega_i ~ PG(1, x_i' beta), x_i' beta from red1 (k_pre's row sums): drawn by
            // trailing workgroups of the speculative lambda launch.  The logistic engine caps
            // p at 16384 (engine create), inside that launch's range (kLamSpecMax).
            if (!launch_lambda_pg(stream, beta, p_loc, p_pad, 0, sc, cfg.seed, cfg.stream, t,
                                  group, lam, trl, red1 + nbS, n, n_pad, omega, err))
                throw HipError("logistic sweep: p beyond the fused lambda / Polya-Gamma launch");
            if (cfg.gram_mode == 1) {
                // X'Omega X = Y Y', Y = X' diag(sqrt(omega)): the Ozaki-II Gram of the
                // resident transpose (rows = coefficients, K = observations)
                mark(PH_OZPREP);
                launch_oz_scale(stream, omega, n_pad, oz_xmax, n_oz, oz_b, oz_rowmax, oz_rscale,
                                oz_escale);
                launch_oz_residues(stream, Xt, p_pad, p_pad, n_oz, n_pad, omega, oz_rscale, oz_R,
                                   nullptr, nullptr);
                mark(PH_GRAM);
                launch_oz_gemm(stream, oz_R, n_oz, n_pad, oz_S, oz_P);
                mark(PH_REDUCE);
                launch_oz_crt(stream, oz_P, oz_S, n_oz, p_pad, oz_escale, nullptr, 0, Gw);
            } else {
                mark(PH_GRAM);
                launch_gram(stream, Xt, p_pad, omega, p_pad, n_pad, S, slabs, p_pad, slab_stride);
                mark(PH_REDUCE);
                launch_slab_sum(stream, slabs, S, slab_stride, p_pad, nullptr, 0, Gw, 0);
            }
        } else if (tri()) {
            // BridgeWrapper.cpp:166-168: omega, u, then the rtnorm_gibbs beta passes
            mark(PH_BETA);
            launch_tri_update(stream, beta, u, lam, D, p, tVc, tVr, tri_a, tri_d, tri_G, cvec,
                              cfg.ortho, sc, cfg.betaburn, cfg.seed, cfg.stream, t,
                              slot_ptr(tr_beta, slot, p_loc), slot_ptr(tr_u, slot, p_loc), trl,
                              slot_ptr(tr_shape, slot, p_loc), err);
        } else {
            launch_lambda(stream, beta, p_loc, p_pad, (uint64_t)cfg.j0, sc, cfg.seed, cfg.stream, t, LAMBDA_ONLY,
                          group, lam, nullptr, nullptr, trl, err);
        }
    }

    void phase_c(uint64_t t, int slot, int mcmc_phase) {
        double *trb = slot_ptr(tr_beta, slot, p_loc);
        bool xb_fused = false;
        if (woodbury()) {
            // w = M^-1 (y / sig - v): the Gram + Cholesky path, or (nid_kl > 0 and the device
            // decided so) the Chebyshev solve -- the kernels of the other path return at once
            // (a shard that took the Chebyshev path solved it in solve_schedule: nid_only)
            const int *gate = nid_kl ? &nid->mode : nullptr;
            if (!nid_only) {
                mark(PH_FORM);
                launch_form_m(stream, red2, n, n_pad, y, sc, cfg.seed, cfg.stream, t, M, n_pad,
                              n_pad, gate);
                mark(PH_CHOL);
                chol_factor(stream, M, n_pad, n_pad, 1, err, Wd, flags, nullptr, gate);
                mark(PH_SOLVE);
                chol_bsolve(stream, M, n_pad, n_pad, Wd, M + (size_t)n_pad * n_pad, w, 1, flags,
                            err, gate);
            }
            if (nid_kl) nid_solve(t, nid_kl);
        }
        if (sparse()) {
            mark(PH_BETA);
            launch_sp_beta(stream, spd.colptr, spd.rowidx, spd.cval, p_loc, w, u, D, sc, beta, trb);
        } else if (dense()) {
            mark(PH_BETA);
            if (nid_only && nid_b32) {
                // a b32 sweep: beta from the banked dots and one pass over X32; its X beta was
                // written by the solve's last step, the single partial k_pre sums next
                launch_beta_woodbury32(stream, X32, n_pad, n_pad, ch_d, ch_c, gb, u, D, sc, nid,
                                       p_loc, beta, trb);
                nparts = 1;
                xb_fused = true;
            } else if (beta_xb_supported(n_pad)) {
                // beta and the X beta partials of the next sweep in one pass over X
                launch_beta_woodbury_xb(stream, X, n_pad, n_pad, w, u, D, sc, p_loc, beta, trb,
                                        xb_part);
                nparts = beta_xb_parts(p_loc);
                xb_fused = true;
            } else {
                launch_beta_woodbury(stream, X, n_pad, n_pad, w, u, D, sc, p_loc, beta, trb);
            }
        } else if (pxp()) {
            // logistic: A = X'Omega X + diag(lambda / tau^2) (sig2 = 1), c = X'kappa
            mark(PH_FORM);
            const int m = chol_m;  // round_up(p, 64) <= p_pad
            launch_form_a(stream, logit() ? Gw : G, p_pad, lam, sc, cvec, p, m, A, p_pad, m,
                          logit() && cfg.gram_mode == 1);
            mark(PH_CHOL);
            chol_factor(stream, A, p_pad, m, 1, err, Wd, flags);
            mark(PH_SOLVE);
            launch_chol_rhs(stream, A, p_pad, m, p, m, cfg.seed, cfg.stream, t, Y2);
            chol_bsolve(stream, A, p_pad, m, Wd, Y2, W2, 2, flags, err);
            mark(PH_BETA);
            launch_beta_chol(stream, W2, m, sc, p, beta, trb);
        } else if (ortho()) {
            mark(PH_BETA);
            launch_beta_ortho(stream, gdiag, cvec, lam, sc, p_loc, (uint64_t)cfg.j0, cfg.seed,
                              cfg.stream, t, beta, trb);
        }
        if (!xb_fused) {
            mark(PH_XB);
            xbeta();
        }
        if (!hy.know_alpha) {
            mark(PH_ALPHA);
            if (cfg.world > 1) {
                // a column shard: this shard's two sums, exchanged (red3) before phase_d
                launch_alpha_sums(stream, beta, p_loc, sc, cfg.seed, cfg.stream, t, red3);
                return;
            }
            // BridgeWrapper.cpp:272 (burn-in: alpha_a, alpha_b), :294 (MCMC: alpha_b, alpha_b
            // -- reference quirk kept), ortho :499/:519 (alpha_a, alpha_b).
            launch_alpha_mh(stream, beta, p, sc, alpha_prior_a(mcmc_phase), hy.alpha_b, cfg.seed,
                            cfg.stream, t, slot_ptr(tr_alpha, slot, 1));
        }
        mark(PH_END);
    }

    // the reference's MH-prior quirk applies: the stable mixture's general driver (Cholesky or
    // Woodbury draw) passes (alpha_b, alpha_b) in its MCMC loop; the ortho, triangle
    // (BridgeWrapper.cpp:146,173) and logistic drivers pass (alpha_a, alpha_b) in both loops
    bool mh_prior_quirk() const { return method == CHOL || woodbury(); }
    double alpha_prior_a(int mcmc_phase) const {
        return (mh_prior_quirk() && mcmc_phase) ? hy.alpha_b : hy.alpha_a;
    }
    // a sharded chain with alpha unknown exchanges the MH sums between phase_c and phase_d
    bool alpha_exchange() const { return !hy.know_alpha && cfg.world > 1; }

    void phase_d(uint64_t t, int slot, int mcmc_phase) {
        if (!alpha_exchange()) return;
        launch_alpha_decide(stream, red3, p, sc, alpha_prior_a(mcmc_phase), hy.alpha_b, cfg.seed,
                            cfg.stream, t, slot_ptr(tr_alpha, slot, 1));
        mark(PH_END);
    }

    size_t red1_count() const { return (size_t)nbS + n_pad; }
    size_t red2_count() const { return tri_count(n_pad) + n_pad; }

    // RCCL shard-group members (bb_group_run): the group's stop flag, raised when another
    // member failed (its collectives will never be matched, so enqueueing more is pointless),
    // and the sweep index at which this member fails on purpose (bb_debug_fail_member)
    const std::atomic<bool> *stop = nullptr;
    int fail_at = -1;
    int nid_kl = 0;  // Chebyshev iterations launched for the sweep being enqueued
    int xu_fused = 0;  // X u partials formed by this sweep's lambda launch (k_lambda_xu), or 0
    unsigned int *lam_sync = nullptr;  // the split lambda launch's chunk flags and counter
    unsigned int lam_ep = 0;           // its launch epoch (flags are never cleared)
    unsigned long long n_lambda_xu = 0, n_lambda_alone = 0;  // Woodbury lambda launches by kind

    // what a fused chain launch takes from this engine, for its own chain and for the chains
    // of a batch that shares its design (bb_chains: keys (seed, k1 + chain), its own rings)
    ChainDesign chain_design() const {
        return {.X = X, .ldx = n_pad, .n = n, .p = p, .y = y, .G = G, .ldg = p_pad, .cvec = cvec,
                .gdiag = gdiag, .tVc = tVc, .tVr = tVr, .a = tri_a, .d = tri_d, .Gf = tri_G,
                .ortho = tri() ? cfg.ortho : ortho(), .betaburn = cfg.betaburn, .hy = hy};
    }
    // this engine's own chain: the general path's fields (the triangle mixture's shape is D)
    ChainView view() const {
        return {.st = {.beta = beta, .lam = lam, .u = u, .shape = D, .sc = sc, .err = err},
                .tr = {.beta = tr_beta, .lam = tr_lam, .sig2 = tr_sig2, .tau = tr_tau,
                       .alpha = tr_alpha, .u = tr_u, .shape = tr_shape},
                .p = p_loc, .cap = cap, .n = n, .omega = omega};
    }
    // the C ABI's accessors: f(the view) once `refusal` is null and the stream has drained
    template <class F>
    int with_view(const char *refusal, F f) {
        return guarded([&] {
            if (refusal) throw HipError(refusal);
            HIPCHECK(hipStreamSynchronize(stream));
            f(view());
        });
    }
    ChainRun chain_run(uint64_t k1, uint64_t t0, int count, int first_slot, int slot_step,
                       int ring_cap, int mcmc_phase) const {
        return {.k0 = cfg.seed, .k1 = k1, .t0 = t0, .count = count, .first_slot = first_slot,
                .slot_step = slot_step, .cap = ring_cap, .pr_a = alpha_prior_a(mcmc_phase),
                .pr_b = hy.alpha_b};
    }

    // `count` sweeps from t0 into slots first_slot + k slot_step (mod cap)
    void run(uint64_t t0, int count, int first_slot, int slot_step, int mcmc_phase) {
        if (path.kind != CK_NONE) {
            if (timing) {
                sweep_marks.emplace_back();
                mark(PH_BETA);
            }
            path.launch(stream, 0, chain_design(), view(),
                        chain_run(cfg.stream, t0, count, first_slot, slot_step, cap, mcmc_phase));
            if (timing) mark(PH_END);
            xb_stale = true;  // X beta partials refreshed only if a general sweep needs them
            return;
        }
        for (int k = 0; k < count; ++k) {
            if (stop && stop->load(std::memory_order_relaxed)) break;
            if (k == fail_at) throw HipError("injected failure (bb_debug_fail_member)");
            const int slot = first_slot < 0 ? -1 : first_slot + k * slot_step;
            sweep(t0 + (uint64_t)k, slot, mcmc_phase);
        }
    }

    inline void sweep(uint64_t t, int slot, int mcmc_phase);  // sweep_schedule over this engine

    uint32_t read_err() {
        uint32_t f = 0;
        HIPCHECK(hipMemcpyAsync(&f, err, sizeof(f), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        return f;
    }
    void clear_err() { HIPCHECK(hipMemsetAsync(err, 0, sizeof(uint32_t), stream)); }
};

// ---------------------------------------------------------------------------
// The sweep schedule, written once over the engines of `Lanes`, the column shards of one chain
// that one host thread enqueues (OneEngine below; GroupLanes, the on-device shard group):
// each(f) runs a stage on every engine, exchange(buf, count) sums a buffer over the shards,
// first() is the engine whose settings stand for all; spec() is the number of products of the
// Chebyshev solve enqueued before the host reads the decision, decide() reads the decided K
// on every engine, phase_c() runs phase c on every engine.
// ---------------------------------------------------------------------------
// The draw before burn-in: the tau (tau_only), or the sig2 and tau, of launch_scalars at t = 0
// into trace slot 0.
template <class Lanes>
void preburn_schedule(Lanes &L, int tau_only) {
    L.each([](bb_engine *e) { e->pre(); });
    L.exchange(&bb_engine::red1, L.first()->red1_count());
    L.each([&](bb_engine *e) { e->scalars(0, 0, tau_only); });
}

// A Woodbury sweep between phase b and phase c: w by the Chebyshev solve (nid_only), or red2
// for the factor of phase c.
template <class Lanes>
void solve_schedule(Lanes &L, uint64_t t) {
    bb_engine *e0 = L.first();
    const size_t nv = (size_t)e0->n_pad;
    if (!e0->nid_sync()) {
        L.exchange(&bb_engine::red2, e0->red2_count());
        return;
    }
    L.exchange(&bb_engine::nid_red, (size_t)bb_engine::kNidRed);
    L.each([](bb_engine *e) { e->nidx_decide_launch(); });
    // The start of the Chebyshev solve is enqueued before the host waits for the decision --
    // X u, the initial iterate and one product, each returning at once unless the device
    // decided so -- so the device runs them while the host wakes up (no bubble on the common
    // near-identity sweep); the rest follows the decision.  A shard's two exchanges among them
    // run on every rank whatever the decision (the same sequence of collectives everywhere; on
    // a factor sweep they carry unused vectors); an unsharded engine has nothing to exchange.
    const int spec = L.spec();
    if (spec) {
        L.each([](bb_engine *e) { e->nidx_xu(); });
        if (e0->sharded()) L.exchange(&bb_engine::nid_sum, nv);
        L.each([&](bb_engine *e) { e->nidx_init(t); });
        L.each([](bb_engine *e) { e->nidx_eapply(1); });
        if (e0->sharded()) L.exchange(&bb_engine::nid_sum, nv);
        L.each([](bb_engine *e) { e->nidx_step(1); });
    }
    const int K = L.decide();
    if (K > 0) {
        if (!spec) {
            L.each([](bb_engine *e) { e->nidx_xu(); });
            L.exchange(&bb_engine::nid_sum, nv);
            L.each([&](bb_engine *e) { e->nidx_init(t); });
        }
        for (int j = spec ? spec : 1; j < K; ++j) {
            L.each([&](bb_engine *e) { e->nidx_eapply(j); });
            L.exchange(&bb_engine::nid_sum, nv);
            L.each([&](bb_engine *e) { e->nidx_step(j); });
        }
        // the mixed plan is an unsharded engine's alone (mixed_ok), so nothing is exchanged
        if (e0->nid_k2 > 0) L.each([](bb_engine *e) { e->nidx_mixed_tail(e->nid_k2); });
    } else {
        L.each([](bb_engine *e) { e->wb_gram(nullptr); });
        L.exchange(&bb_engine::red2, e0->red2_count());
    }
}

// A sweep is three phases separated by the two exchange points of the column-sharded
// decomposition: red1 = [S_alpha partials | X beta] and, through
// solve_schedule, red2 = [partial Gram | X u]; alpha unknown adds the exchange of the MH sums.
template <class Lanes>
void sweep_schedule(Lanes &L, uint64_t t, int slot, int mcmc_phase) {
    bb_engine *e0 = L.first();
    L.each([&](bb_engine *e) { e->phase_a(t); });
    L.exchange(&bb_engine::red1, e0->red1_count());
    L.each([&](bb_engine *e) { e->phase_b(t, slot); });
    if (e0->woodbury()) solve_schedule(L, t);
    L.phase_c(t, slot, mcmc_phase);
    if (e0->alpha_exchange()) {
        L.exchange(&bb_engine::red3, 2);
        L.each([&](bb_engine *e) { e->phase_d(t, slot, mcmc_phase); });
    }
}

// One engine: a single chain, or a rank exchanging through its communicator (allreduce does
// nothing without one).  The speculative start hides the host's wake-up unless key 8 = 2.
struct OneEngine {
    bb_engine *e;
    bb_engine *first() const { return e; }
    template <class F>
    void each(F f) { f(e); }
    void exchange(double *bb_engine::*buf, size_t count) { e->allreduce(e->*buf, count); }
    int spec() const { return g_nid_sync != 2 ? 2 : 0; }
    int decide() { return e->nidx_decide_read(); }
    void phase_c(uint64_t t, int slot, int mcmc_phase) { e->phase_c(t, slot, mcmc_phase); }
};

inline void bb_engine::sweep(uint64_t t, int slot, int mcmc_phase) {
    OneEngine one{this};
    sweep_schedule(one, t, slot, mcmc_phase);
}

namespace {

// Right singular vectors and singular values of X (n x p, column-major, n >= p) without
// forming X'X, whose condition number is the square of X's: Householder QR X = Q R on the
// host, then one-sided (Hestenes) Jacobi on the columns of R until every pair is orthogonal
// to fp64 precision.  R V = U diag(d) gives X = (Q U) diag(d) V'.  O(n p^2 + sweeps p^3).
void svd_right(const double *Xh, int n, int p, std::vector<double> &V, std::vector<double> &d) {
    std::vector<double> A(Xh, Xh + (size_t)n * p);
    auto col = [&](int j) { return &A[(size_t)j * n]; };
    for (int k = 0; k < p && k < n; ++k) {
        double *ak = col(k);
        double nrm = 0.0;
        for (int i = k; i < n; ++i) nrm += ak[i] * ak[i];
        nrm = sqrt(nrm);
        if (nrm == 0.0) continue;
        const double alpha = ak[k] >= 0 ? -nrm : nrm;
        ak[k] -= alpha;  // v = x - alpha e1 (stored in place)
        double vv = 0.0;
        for (int i = k; i < n; ++i) vv += ak[i] * ak[i];
        for (int j = k + 1; j < p; ++j) {
            double *aj = col(j);
            double sdot = 0.0;
            for (int i = k; i < n; ++i) sdot += ak[i] * aj[i];
            const double f = 2.0 * sdot / vv;
            for (int i = k; i < n; ++i) aj[i] -= f * ak[i];
        }
        ak[k] = alpha;
        for (int i = k + 1; i < n; ++i) ak[i] = 0.0;
    }
    // W = R (p x p), V = I
    std::vector<double> W((size_t)p * p, 0.0);
    for (int j = 0; j < p; ++j)
        for (int i = 0; i <= j && i < n; ++i) W[(size_t)j * p + i] = A[(size_t)j * n + i];
    V.assign((size_t)p * p, 0.0);
    for (int i = 0; i < p; ++i) V[(size_t)i * p + i] = 1.0;
    std::vector<double> nrm2(p);
    for (int sweep = 0; sweep < 80; ++sweep) {
        long rotated = 0;
        // squared column norms, refreshed every sweep and carried through each rotation
        // (||w_i'||^2 = a - t c, ||w_j'||^2 = b + t c)
        for (int j = 0; j < p; ++j) {
            double s2 = 0.0;
            for (int k = 0; k < p; ++k) s2 += W[(size_t)j * p + k] * W[(size_t)j * p + k];
            nrm2[j] = s2;
        }
        for (int i = 0; i < p - 1; ++i) {
            double *wi = &W[(size_t)i * p], *vi = &V[(size_t)i * p];
            for (int j = i + 1; j < p; ++j) {
                double *wj = &W[(size_t)j * p], *vj = &V[(size_t)j * p];
                const double a = nrm2[i], b = nrm2[j];
                double c = 0.0;
                for (int k = 0; k < p; ++k) c += wi[k] * wj[k];
                if (c == 0.0 || fabs(c) <= 1e-15 * sqrt(a * b)) continue;
                ++rotated;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                nrm2[i] = a - t * c;
                nrm2[j] = b + t * c;
                for (int k = 0; k < p; ++k) {
                    const double x = wi[k], y = wj[k];
                    wi[k] = cs * x - sn * y;
                    wj[k] = sn * x + cs * y;
                    const double u = vi[k], w = vj[k];
                    vi[k] = cs * u - sn * w;
                    vj[k] = sn * u + cs * w;
                }
            }
        }
        if (rotated == 0) break;
    }
    d.resize(p);
    for (int j = 0; j < p; ++j) {
        double s2 = 0.0;
        for (int k = 0; k < p; ++k) s2 += W[(size_t)j * p + k] * W[(size_t)j * p + k];
        d[j] = sqrt(s2);
    }
}

// X = U diag(d) V' (BridgeRegression.cpp:47-57, svd 'S' for n > p): tV = V' with singular
// values in decreasing order, each right singular vector signed so its largest-magnitude
// entry is positive; a = d * U'y = V' X'y.
void tri_setup(bb_engine *e, const double *Xh) {
    const int p = e->p, pp = e->p_pad;
    std::vector<double> Gp((size_t)pp * pp), c(pp);
    HIPCHECK(hipStreamSynchronize(e->stream));
    HIPCHECK(hipMemcpy(Gp.data(), e->G, Gp.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(c.data(), e->cvec, (size_t)pp * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> G((size_t)p * p);
    for (int j = 0; j < p; ++j)
        for (int i = 0; i < p; ++i) {  // the device Gram holds the upper triangle
            const int r = i < j ? i : j, q = i < j ? j : i;
            G[(size_t)j * p + i] = Gp[(size_t)q * pp + r];
        }
    std::vector<double> V, sv;
    svd_right(Xh, e->n, p, V, sv);
    std::vector<int> ord(p);
    for (int i = 0; i < p; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return sv[x] > sv[y]; });
    e->h_tV.assign((size_t)p * p, 0.0);
    e->h_a.assign(p, 0.0);
    e->h_d.assign(p, 0.0);
    std::vector<double> tVr((size_t)p * p);
    for (int i = 0; i < p; ++i) {
        const double *v = &V[(size_t)ord[i] * p];
        int jm = 0;
        for (int j = 1; j < p; ++j)
            if (fabs(v[j]) > fabs(v[jm])) jm = j;
        const double sg = v[jm] < 0 ? -1.0 : 1.0;
        double a = 0.0;
        for (int j = 0; j < p; ++j) {
            const double x = sg * v[j];
            e->h_tV[i + (size_t)j * p] = x;
            tVr[(size_t)i * p + j] = x;
            a += x * c[j];
        }
        e->h_a[i] = a;
        e->h_d[i] = sv[ord[i]];
    }
    auto &o = e->owned;
    e->tVc = dalloc<double>((size_t)p * p, o);
    e->tVr = dalloc<double>((size_t)p * p, o);
    e->tri_a = dalloc<double>(p, o);
    e->tri_d = dalloc<double>(p, o);
    HIPCHECK(hipMemcpy(e->tVc, e->h_tV.data(), (size_t)p * p * sizeof(double),
                       hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(e->tVr, tVr.data(), (size_t)p * p * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(e->tri_a, e->h_a.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(e->tri_d, e->h_d.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice));
    e->tri_G = dalloc<double>((size_t)p * p, o);  // full symmetric X'X (ortho variant)
    HIPCHECK(hipMemcpy(e->tri_G, G.data(), (size_t)p * p * sizeof(double), hipMemcpyHostToDevice));
    e->tr_u = dalloc<double>((size_t)p * e->cap, o);
    e->tr_shape = dalloc<double>((size_t)p * e->cap, o);
}

struct SparseIn {
    const int *colptr, *rowidx;
    const double *val;
};

// Certified upper bound Lambda >= lambda_max(X X') for the near-identity bound (bb_nid.hip
// k_nid_reduce): 40 power iterations on X X' (the E-apply pass with D = 1) give the Rayleigh
// quotient rho; U = 1.02 rho is certified by factoring U I - X X' (the Gram with D = 1, the
// device Cholesky): a non-positive pivot (error bit 8) raises U by 25 %, at most six times,
// after which the bound is left out (Lambda = 0: the trace bound alone).  The factor's
// backward error (~n u |A|) is far below the 2 % margin.  Setup only, ~10 ms at C3.
void nid_certify_lambda(bb_engine *e) {
    const int n_pad = e->n_pad, p_pad = e->p_pad;
    hipStream_t s = e->stream;
    double *ones = nullptr;
    NidState *gate = nullptr;
    HIPCHECK(hipMalloc(&ones, (size_t)p_pad * sizeof(double)));
    HIPCHECK(hipMalloc(&gate, sizeof(NidState)));
    std::vector<double> h1(p_pad, 0.0);
    for (int j = 0; j < e->p_loc; ++j) h1[j] = 1.0;
    HIPCHECK(hipMemcpyAsync(ones, h1.data(), h1.size() * sizeof(double), hipMemcpyHostToDevice, s));
    NidState g{};
    g.mode = 64;  // every pass of the power iteration runs
    HIPCHECK(hipMemcpyAsync(gate, &g, sizeof(g), hipMemcpyHostToDevice, s));
    std::vector<double> v(n_pad, 0.0), w(n_pad);
    double nv = 0.0;
    for (int i = 0; i < e->n; ++i) {
        v[i] = std::cos(0.7 * i + 0.3) + 0.5 * std::sin(1.3 * i * i + 0.1);
        nv += v[i] * v[i];
    }
    for (auto &x : v) x /= std::sqrt(nv);
    double rho = 0.0;
    for (int it = 0; it < 40; ++it) {
        HIPCHECK(hipMemcpyAsync(e->ch_d, v.data(), n_pad * sizeof(double), hipMemcpyHostToDevice, s));
        if (e->sparse())
            launch_sp_eapply(s, e->spd.colptr, e->spd.rowidx, e->spd.cval, e->spd.rowptr,
                             e->spd.colidx, e->spd.rval, e->p_loc, n_pad, ones, e->ch_d, gate, 0,
                             e->sp_s, e->ea_part);
        else
            launch_eapply(s, e->X, n_pad, n_pad, e->p_loc, ones, e->ch_d, gate, 0, e->ea_part);
        launch_part_sum(s, e->ea_part, e->sparse() ? 1 : e->ea_parts, n_pad, e->ch_r);
        HIPCHECK(hipMemcpyAsync(w.data(), e->ch_r, n_pad * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        double vw = 0.0, ww = 0.0;
        for (int i = 0; i < n_pad; ++i) {
            vw += v[i] * w[i];
            ww += w[i] * w[i];
        }
        rho = vw;
        if (!(ww > 0.0)) break;
        for (int i = 0; i < n_pad; ++i) v[i] = w[i] / std::sqrt(ww);
    }
    double lam = 0.0;
    if (rho > 0.0 && std::isfinite(rho)) {
        // the Gram X X' into red2 (packed upper triangle)
        if (e->sparse()) {
            e->spd.gram(s, ones, ones, e->red2, e->red2 + tri_count(n_pad));
        } else if (e->cfg.gram_mode == 1) {
            launch_oz_scale(s, ones, p_pad, e->oz_xmax, e->n_oz, e->oz_b, e->oz_rowmax,
                            e->oz_rscale, e->oz_escale);
            launch_oz_residues(s, e->X, n_pad, n_pad, e->n_oz, p_pad, ones, e->oz_rscale, e->oz_R);
            launch_oz_gemm(s, e->oz_R, e->n_oz, p_pad, e->oz_S, e->oz_P);
            launch_oz_crt(s, e->oz_P, e->oz_S, e->n_oz, n_pad, e->oz_escale, nullptr, 0, e->red2);
        } else {
            launch_gram(s, e->X, n_pad, ones, n_pad, p_pad, e->S, e->slabs, n_pad, e->slab_stride);
            launch_slab_sum(s, e->slabs, e->S, e->slab_stride, n_pad, nullptr, 0, e->red2, 1);
        }
        double U = 1.02 * rho;
        for (int attempt = 0; attempt < 7 && lam == 0.0; ++attempt, U *= 1.25) {
            e->clear_err();
            launch_shift_gram(s, e->red2, n_pad, U, e->M, n_pad);
            chol_factor(s, e->M, n_pad, n_pad, 1, e->err, e->Wd, e->flags);
            if ((e->read_err() & (8u | 16u)) == 0) lam = U * (1.0 + 1e-9);
        }
        e->clear_err();
    }
    HIPCHECK(hipMemsetAsync(e->nid, 0, sizeof(NidState), s));
    HIPCHECK(hipMemcpyAsync(&e->nid->lambda_x, &lam, sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(&e->nid->c64, e->nid_cost, sizeof(e->nid_cost), hipMemcpyHostToDevice,
                            s));
    // sum_j |x_j|^2 for the guessed interval of the residual-certified plan,
    // added on the host in column order
    std::vector<double> hcn(e->p_loc);
    HIPCHECK(hipMemcpyAsync(hcn.data(), e->cn, hcn.size() * sizeof(double), hipMemcpyDeviceToHost,
                            s));
    HIPCHECK(hipStreamSynchronize(s));
    double scn = 0.0;
    for (double v : hcn) scn += v;
    HIPCHECK(hipMemcpyAsync(&e->nid->sum_cn, &scn, sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    e->lambda_x = lam;
    (void)hipFree(ones);
    (void)hipFree(gate);
}

void engine_setup(bb_engine *e, const double *Xh, const double *yh, const SparseIn *spin) {
    const bb_config &c = e->cfg;
    e->n = c.n;
    e->p = c.p;
    e->p_loc = c.p_local;
    e->n_pad = round_up(c.n, kGramTile);
    e->p_pad = round_up(c.p_local, 256);
    e->chol_m = round_up(c.p_local, kNB);
    e->cap = c.trace_capacity < 1 ? 1 : c.trace_capacity;
    e->hy = Hyper{c.sig2_shape, c.sig2_scale, c.nu_shape, c.nu_rate, c.alpha_a, c.alpha_b,
                  c.true_tau > 0, c.true_sig2 > 0, c.true_alpha > 0};
    if (spin) {
        if (c.ortho || c.method == CHOL || c.method == ORTHO || c.method == TRI ||
            c.method == LOGIT)
            throw HipError("a CSC design runs the Woodbury (p > n) draw only");
        e->method = SPARSE;
    } else if (c.method == LOGIT) {
        e->method = LOGIT;
        e->hy.know_sig2 = 1;  // the PG mixture has unit scale
        // X'Omega X runs over K = n_pad rows: pad to 512 so the Gram can split K 16 ways
        e->n_pad = round_up(c.n, 512);
        if (c.world > 1) throw HipError("the logistic path runs on one device (world == 1)");
        if (c.ortho) throw HipError("the logistic path has no orthogonal-design variant");
        if (c.p > 16384) throw HipError("logistic path limited to p <= 16384");
    } else if (c.method == TRI) e->method = TRI;
    else if (c.ortho) e->method = ORTHO;
    else if (c.method == CHOL || (c.method == AUTO && c.p <= c.n)) e->method = CHOL;
    else e->method = WOODBURY;
    // column shards: the p > n Woodbury draws (dense, sparse) and the orthogonal design
    // (per-coefficient draws, p > n); alpha known or unknown (the MH sums are exchanged)
    if (c.world > 1 && !e->woodbury() && !(e->ortho() && c.p > c.n))
        throw HipError("column sharding (world > 1) is implemented for the p > n paths only "
                       "(Woodbury, sparse Woodbury, orthogonal design)");
    if (e->tri() && (c.p > c.n || c.p > kTriMaxP))
        throw HipError("triangle sampler needs p <= n and p <= 2048");
    if (e->method == CHOL && c.p > 16384)
        throw HipError("p x p Cholesky path limited to p <= 16384");
    if (e->woodbury() && e->n_pad > 8192)
        throw HipError("Woodbury path limited to n <= 8192 in this build");

    HIPCHECK(hipSetDevice(c.device));
    HIPCHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    auto &o = e->owned;
    const int n_pad = e->n_pad, p_pad = e->p_pad;
    if (spin) {
        e->spd.build(e->stream, c.n, n_pad, c.p_local, spin->colptr, spin->rowidx, spin->val, o);
    } else {
        e->X = dalloc<double>((size_t)n_pad * p_pad, o);
        HIPCHECK(hipMemcpy2D(e->X, (size_t)n_pad * sizeof(double), Xh,
                             (size_t)c.n * sizeof(double), (size_t)c.n * sizeof(double),
                             (size_t)c.p_local, hipMemcpyHostToDevice));
    }
    e->y = dalloc<double>(n_pad, o);
    HIPCHECK(hipMemcpy(e->y, yh, (size_t)c.n * sizeof(double), hipMemcpyHostToDevice));
    e->beta = dalloc<double>(p_pad, o);
    e->lam = dalloc<double>(p_pad, o);
    e->D = dalloc<double>(p_pad, o);
    e->u = dalloc<double>(p_pad, o);
    e->sc = dalloc<DevScalars>(1, o);
    e->err = dalloc<uint32_t>(4, o);
    e->nparts = xv_chunks(p_pad, n_pad);
    e->xb_part = dalloc<double>(
        (size_t)std::max(e->sparse() ? 1 : xv_chunks_max(p_pad), beta_xb_parts(c.p_local)) *
            n_pad,
        o);
    e->nbS = pre_blocks_s(c.p_local);
    e->red1 = dalloc<double>((size_t)e->nbS + n_pad, o);
    e->red3 = dalloc<double>(2, o);
    e->group = stable_group_for(c.p_local);
    e->tr_beta = dalloc<double>((size_t)c.p_local * e->cap, o);
    e->tr_lam = dalloc<double>((size_t)c.p_local * e->cap, o);
    e->tr_sig2 = dalloc<double>(e->cap, o);
    e->tr_tau = dalloc<double>(e->cap, o);
    e->tr_alpha = dalloc<double>(e->cap, o);

    if (e->dense()) {
        if (c.gram_mode == 1) {
            e->n_oz = oz_rows(n_pad);
            const int nkc = p_pad / kOzKC;
            e->oz_b = oz_bits_for(p_pad);
            e->oz_S = oz_splits_for(e->n_oz, nkc);
            e->oz_xmax = dalloc<double>((size_t)nkc * e->n_oz, o);
            e->oz_rowmax = dalloc<double>((size_t)oz_bound_groups(p_pad) * e->n_oz, o);
            e->oz_rscale = dalloc<double>(e->n_oz, o);
            e->oz_escale = dalloc<int>(e->n_oz, o);
            e->oz_R = dalloc<int8_t>(oz_residue_bytes(e->n_oz, p_pad), o);
            e->oz_P = dalloc<int8_t>(oz_partial_bytes(e->n_oz, e->oz_S), o);
            launch_oz_xmax(e->stream, e->X, n_pad, n_pad, e->n_oz, p_pad, e->oz_xmax);
        } else {
            e->S = gram_splits_for(n_pad, p_pad);
            e->slab_stride = (size_t)n_pad * n_pad;
            e->slabs = dalloc<double>(e->slab_stride * e->S, o);
        }
        e->xu_part = dalloc<double>((size_t)xv_chunks_max(p_pad) * n_pad, o);
    }
    if (e->woodbury()) {
        e->red2 = dalloc<double>(tri_count(n_pad) + n_pad, o);
        e->M = dalloc<double>((size_t)n_pad * (n_pad + kNB), o);
        e->w = dalloc<double>(n_pad, o);
        // near-identity solve (bb_nid.hip); the dense E-apply keeps its rows in registers up
        // to n_pad = 4096
        if (e->sparse() || eapply_supported(n_pad)) {
            e->cn = dalloc<double>(p_pad, o);
            if (e->sparse()) {
                std::vector<double> h(c.p_local, 0.0);
                for (int j = 0; j < c.p_local; ++j)
                    for (int q = spin->colptr[j]; q < spin->colptr[j + 1]; ++q)
                        h[j] += spin->val[q] * spin->val[q];
                HIPCHECK(hipMemcpy(e->cn, h.data(), h.size() * sizeof(double),
                                   hipMemcpyHostToDevice));
                e->sp_s = dalloc<double>(p_pad, o);
                e->ea_parts = 1;
                e->ea_part = dalloc<double>(n_pad, o);
                e->nid_xu = dalloc<double>(n_pad, o);
            } else {
                launch_colnorm2(e->stream, e->X, n_pad, n_pad, c.p_local, e->cn);
                e->ea_parts = eapply_parts(c.p_local, n_pad);
                e->ea_part = dalloc<double>((size_t)e->ea_parts * n_pad, o);
                const int xp = std::max(e->ea_parts, lambda_xu_parts(c.p_local, p_pad, n_pad));
                e->nid_xu = dalloc<double>((size_t)xp * n_pad, o);
                // + the folded decision's count (the last word)
                const int sw = lambda_xs_sync_words(p_pad) + 1;
                e->lam_sync = dalloc<unsigned int>(sw, o);
                HIPCHECK(hipMemsetAsync(e->lam_sync, 0, sizeof(unsigned int) * sw, e->stream));
            }
            e->nid = dalloc<NidState>(1, o);
            {
                // the Chebyshev plans' cost model (bb_nid.hip nid_plan_mixed; copied into the
                // NidState by nid_certify_lambda): a pass streams X at ~6.2 TB/s plus ~4 us of
                // launch and partials; a step launch ~6 us
                const double bytes = (double)n_pad * (double)c.p_local;
                e->nid_cost[0] = 8.0 * bytes / 6.2e12 + 4e-6;
                e->nid_cost[1] = 4.0 * bytes / 6.2e12 + 4e-6;
                e->nid_cost[2] = 6e-6;
            }
            e->ch_r = dalloc<double>(n_pad, o);
            e->ch_d = dalloc<double>(n_pad, o);
            e->nid_red = dalloc<double>(bb_engine::kNidRed, o);
            // k_nid_sums' partials, or the split lambda launch's (one per stream workgroup)
            e->nid_wg = dalloc<double>(
                (size_t)std::max(nid_sum_groups(c.p_local), 1024) * (kNidTS + 1), o);
            e->nid_sum = dalloc<double>(n_pad, o);
            // the hint ring, then [eps, mode, k2, tag] of the sweep being decided (coherent:
            // the host polls the tag while the device runs on)
            const int nh = bb_engine::kNidRing + 5;  // + the second decision's tag (s6.8)
            HIPCHECK(hipHostMalloc((void **)&e->eps_host, nh * sizeof(double),
                                   hipHostMallocMapped | hipHostMallocCoherent));
            for (int q = 0; q < nh; ++q) e->eps_host[q] = -1.0;  // no observation yet
            *(unsigned long long *)(e->eps_host + bb_engine::kNidRing + 3) = 0ull;
            *(unsigned long long *)(e->eps_host + bb_engine::kNidRing + 4) = 0ull;
            HIPCHECK(hipHostGetDevicePointer((void **)&e->eps_dev, e->eps_host, 0));
            e->nid_kmax = e->nid_kmax_model();
            // the mixed-precision plan's fp32 copy of X (unsharded dense engines; 4 B per
            // element: 400 MB at C3), unless an entry is outside fp32's normal range
            // Only when the plan can be used (key 10 on, a Chebyshev path at all), and never
            // at the price of the engine: a failed allocation keeps the fp64 plan.
            if (e->dense() && c.world == 1 && g_nid_mixed && e->nid_kmax > 0) {
                void *x32 = nullptr;
                if (hipMalloc(&x32, (size_t)n_pad * p_pad * sizeof(float)) != hipSuccess) {
                    (void)hipGetLastError();  // clear the sticky out-of-memory status
                    x32 = nullptr;
                }
                if (x32) {
                    e->ch_b = dalloc<double>(n_pad, o);
                    int *bad = dalloc<int>(1, o);
                    HIPCHECK(hipMemsetAsync(bad, 0, sizeof(int), e->stream));
                    launch_cast_f32(e->stream, e->X, n_pad, n_pad, c.p_local, (float *)x32, bad);
                    int hb = 0;
                    HIPCHECK(hipMemcpyAsync(&hb, bad, sizeof(int), hipMemcpyDeviceToHost, e->stream));
                    HIPCHECK(hipStreamSynchronize(e->stream));
                    if (hb) {
                        (void)hipFree(x32);  // an entry outside fp32's normal range
                    } else {
                        o.push_back(x32);
                        e->X32 = (float *)x32;
                        // the residual certificate's partials of |b|^2 and |r|^2
                        e->nid_sqn = (n_pad + 7) / 8;
                        e->nid_sq = dalloc<double>(2 * (size_t)e->nid_sqn, o);
                        HIPCHECK(hipMemsetAsync(e->nid_sq, 0, 2 * sizeof(double) * e->nid_sqn,
                                                e->stream));
                        if (beta_xb_supported(n_pad)) {  // the fp32 beta pass's vectors
                            e->gb = dalloc<double>(p_pad, o);
                            e->ch_c = dalloc<double>(n_pad, o);
                            e->ch_xu = dalloc<double>(n_pad, o);
                            HIPCHECK(hipMemsetAsync(e->gb, 0, sizeof(double) * p_pad, e->stream));
                            HIPCHECK(hipMemsetAsync(e->ch_c, 0, sizeof(double) * n_pad, e->stream));
                            HIPCHECK(hipMemsetAsync(e->ch_xu, 0, sizeof(double) * n_pad, e->stream));
                        }
                    }
                }
            }
        }
    }
    // X'X / X'y when the chol or ortho path needs them, or for the least-squares start.
    const bool small = c.p <= c.n && c.world == 1 && !e->sparse() && !e->logit();
    // the Cholesky scratch covers the n x n (Woodbury) and any p x p (chol, LS start) system
    const int m_sys = (e->woodbury() && !small) ? n_pad : (n_pad > p_pad ? n_pad : p_pad);
    e->Wd = dalloc<double>(chol_wd_words(m_sys), o);
    e->flags = dalloc<unsigned int>(chol_flag_words(m_sys, 1), o);
    if (e->logit()) {
        // logistic: X' resident (p_pad x n_pad), K-split slabs of X'Omega X, c = X'kappa
        e->Xt = dalloc<double>((size_t)p_pad * n_pad, o);
        launch_transpose(e->stream, e->X, n_pad, n_pad, p_pad, e->Xt, p_pad);
        if (c.gram_mode == 1) {
            // Ozaki-II X'Omega X (packed upper triangle into Gw): rows = p_pad, K = n_pad
            e->n_oz = oz_rows(p_pad);
            const int nkc = n_pad / kOzKC;
            e->oz_b = oz_bits_for(n_pad);
            e->oz_S = oz_splits_for(e->n_oz, nkc);
            e->oz_xmax = dalloc<double>((size_t)nkc * e->n_oz, o);
            e->oz_rowmax = dalloc<double>((size_t)oz_bound_groups(n_pad) * e->n_oz, o);
            e->oz_rscale = dalloc<double>(e->n_oz, o);
            e->oz_escale = dalloc<int>(e->n_oz, o);
            e->oz_R = dalloc<int8_t>(oz_residue_bytes(e->n_oz, n_pad), o);
            e->oz_P = dalloc<int8_t>(oz_partial_bytes(e->n_oz, e->oz_S), o);
            launch_oz_xmax(e->stream, e->Xt, p_pad, p_pad, e->n_oz, n_pad, e->oz_xmax);
        } else {
            e->S = gram_splits_for(p_pad, n_pad);
            e->slab_stride = (size_t)p_pad * p_pad;
            e->slabs = dalloc<double>(e->slab_stride * e->S, o);
        }
        e->Gw = dalloc<double>(std::max((size_t)p_pad * p_pad, tri_count(p_pad)) + p_pad, o);
        e->omega = dalloc<double>(n_pad, o);
        e->kappa = dalloc<double>(n_pad, o);
        launch_kappa(e->stream, e->y, c.n, n_pad, e->kappa);
        e->cvec = dalloc<double>(p_pad, o);
        launch_coldot(e->stream, e->X, n_pad, n_pad, e->kappa, c.p_local, e->cvec);
        e->A = dalloc<double>((size_t)p_pad * (p_pad + kNB), o);
        e->Y2 = dalloc<double>((size_t)2 * p_pad, o);
        e->W2 = dalloc<double>((size_t)2 * p_pad, o);
    } else if (!e->woodbury() || small) {
        e->cvec = dalloc<double>(p_pad, o);
        launch_coldot(e->stream, e->X, n_pad, n_pad, e->y, c.p_local, e->cvec);
        e->gdiag = dalloc<double>(p_pad, o);
        if (small) {
            // G = X'X: transpose X (n_pad x p_pad) into Xt (p_pad x n_pad), Gram over rows.
            double *Xt = nullptr;
            HIPCHECK(hipMalloc(&Xt, (size_t)p_pad * n_pad * sizeof(double)));
            launch_transpose(e->stream, e->X, n_pad, n_pad, p_pad, Xt, p_pad);
            double *ones = nullptr;
            HIPCHECK(hipMalloc(&ones, (size_t)n_pad * sizeof(double)));
            std::vector<double> h1(n_pad, 1.0);
            HIPCHECK(hipMemcpyAsync(ones, h1.data(), n_pad * sizeof(double),
                                    hipMemcpyHostToDevice, e->stream));
            const int Sg = gram_splits_for(p_pad, n_pad);
            double *sl = nullptr;
            HIPCHECK(hipMalloc(&sl, (size_t)Sg * p_pad * p_pad * sizeof(double)));
            launch_gram(e->stream, Xt, p_pad, ones, p_pad, n_pad, Sg, sl, p_pad,
                        (size_t)p_pad * p_pad);
            double *red = nullptr;
            HIPCHECK(hipMalloc(&red, ((size_t)p_pad * p_pad + p_pad) * sizeof(double)));
            launch_slab_sum(e->stream, sl, Sg, (size_t)p_pad * p_pad, p_pad, nullptr, 0, red, 0);
            e->G = dalloc<double>((size_t)p_pad * p_pad, o);
            HIPCHECK(hipMemcpyAsync(e->G, red, (size_t)p_pad * p_pad * sizeof(double),
                                    hipMemcpyDeviceToDevice, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
            (void)hipFree(Xt);
            (void)hipFree(ones);
            (void)hipFree(sl);
            (void)hipFree(red);
            launch_gdiag(e->stream, e->G, p_pad, c.p_local, e->gdiag);
            e->A = dalloc<double>((size_t)p_pad * (p_pad + kNB), o);
            e->Y2 = dalloc<double>((size_t)2 * p_pad, o);
            e->W2 = dalloc<double>((size_t)2 * p_pad, o);
        } else {
            launch_colnorm2(e->stream, e->X, n_pad, n_pad, c.p_local, e->gdiag);
        }
    }
    if (e->tri()) tri_setup(e, Xh);
    // whole sweeps in one single-workgroup launch where the plan says so (a CSC design never);
    // the engine keeps the path it was created with.  What the kernels read follows from the
    // same configuration above: a plan without its buffers is an error, not the general path.
    if (!spin) e->path.kind = chain_plan(c, false).kind;
    if (e->path.kind != CK_NONE &&
        !(e->tri() ? e->tVc && (!c.ortho || (e->tri_G && e->cvec))
                   : e->cvec && e->gdiag && (e->ortho() || e->G)))
        throw HipError("the fused chain's design buffers are missing");
    if (e->nid) nid_certify_lambda(e);
    HIPCHECK(hipStreamSynchronize(e->stream));
}

void engine_init_state_local(bb_engine *e) {
    const bb_config &c = e->cfg;
    e->nid_seq = 0;  // the near-identity launch hint restarts with the chain
    e->nid_last = -1;
    // least squares start (BridgeWrapper.cpp:242-244, BridgeRegression.cpp:79-91)
    bool ls_ok = false;
    if (e->G != nullptr) {
        e->clear_err();
        const int m = e->chol_m ? e->chol_m : e->p_pad;
        launch_form_a(e->stream, e->G, e->p_pad, nullptr, e->sc, e->cvec, e->p, m, e->A,
                      e->p_pad, m);
        chol_factor(e->stream, e->A, e->p_pad, m, 1, e->err, e->Wd, e->flags);
        HIPCHECK(hipMemcpyAsync(e->Y2, e->A + (size_t)m * e->p_pad, m * sizeof(double),
                                hipMemcpyDeviceToDevice, e->stream));
        chol_bsolve(e->stream, e->A, e->p_pad, m, e->Wd, e->Y2, e->W2, 1, e->flags, e->err);
        uint32_t f = e->read_err();
        ls_ok = (f & 8u) == 0;
        if (ls_ok) {
            HIPCHECK(hipMemcpyAsync(e->beta, e->W2, (size_t)e->p * sizeof(double),
                                    hipMemcpyDeviceToDevice, e->stream));
        }
        e->clear_err();
    }
    if (!ls_ok) {
        HIPCHECK(hipMemsetAsync(e->beta, 0, (size_t)e->p_pad * sizeof(double), e->stream));
        if (g_verbose && c.rank == 0 && !e->logit()) {
            printf("Warning: cannot calculate least squares estimate; X'X is singular.\n");
            printf("Warning: setting least squares estimate to 0.0.\n");
        }
    }
    DevScalars s{};
    s.alpha = c.true_alpha > 0 ? c.true_alpha : 0.5;
    s.sig2 = e->logit() ? 1.0 : (c.true_sig2 > 0 ? c.true_sig2 : 0.0);
    s.tau = c.true_tau > 0 ? c.true_tau : 0.0;
    HIPCHECK(hipMemcpyAsync(e->sc, &s, sizeof(s), hipMemcpyHostToDevice, e->stream));
    if (e->tri()) {  // BridgeWrapper.cpp:123 u[0].fill(0.5); omega starts at 1.0 (:604)
        std::vector<double> h(e->p_pad, 0.5);
        HIPCHECK(hipMemcpyAsync(e->u, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice,
                                e->stream));
        std::vector<double> h1(e->p_pad, 1.0);
        HIPCHECK(hipMemcpyAsync(e->lam, h1.data(), h1.size() * sizeof(double),
                                hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipMemcpyAsync(e->tr_u, h.data(), (size_t)e->p_loc * sizeof(double),
                                hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipMemcpyAsync(e->tr_lam, h1.data(), (size_t)e->p_loc * sizeof(double),
                                hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
    }
    // trace slot 0 holds the starting values (as the reference's slot 0 before burn-in)
    HIPCHECK(hipMemcpyAsync(e->tr_beta, e->beta, (size_t)e->p_loc * sizeof(double),
                            hipMemcpyDeviceToDevice, e->stream));
    e->xbeta();
    launch_record_scalars(e->stream, e->sc, e->tr_tau, e->tr_sig2, e->tr_alpha);
}

// The draw a chain makes before burn-in, under the engine's current key (cfg.seed, cfg.stream)
// and from the state engine_init_state_local left: one rule for a single engine and for every
// chain of a batch (bb_chains::init_state), so the two cannot drift.
void engine_preburn_draw(bb_engine *e) {
    OneEngine one{e};
    if (e->tri() && e->cfg.ortho) {
        // triangle ortho driver draws sig2 then tau before burn-in (BridgeWrapper.cpp:374-375)
        if (!e->hy.know_tau || !e->hy.know_sig2) preburn_schedule(one, 0);
    } else if (!e->ortho() && !e->hy.know_tau) {
        preburn_schedule(one, 1);  // :262
    }
}

void engine_init_state(bb_engine *e) {
    engine_init_state_local(e);
    engine_preburn_draw(e);
    HIPCHECK(hipStreamSynchronize(e->stream));
}

// one contiguous run of trace-ring doubles to the host (one copy, not one per sample)
void ring_copy(double *dst, const double *src, size_t count) {
    HIPCHECK(hipMemcpy(dst, src, count * sizeof(double), hipMemcpyDeviceToHost));
}

// Ring slots [slot0, slot0 + count) of some traces to the host: each is `w` doubles per slot
// from `ring` (slot 0 of the ring) to `dst`, skipped when dst is null.
struct RingTrace {
    double *dst;
    const double *ring;
    size_t w;
};
void ring_fetch(int slot0, int count, int cap, std::initializer_list<RingTrace> traces) {
    ring_runs(slot0, count, cap, [&](int k, int slot, int run) {
        for (const RingTrace &t : traces)
            if (t.dst) ring_copy(t.dst + k * t.w, t.ring + slot * t.w, run * t.w);
    });
}

// (tau, sig2, alpha) of a DevScalars on the device; the write keeps its other fields
void scalars_read(const DevScalars *dev, double *tau, double *sig2, double *alpha) {
    DevScalars s;
    HIPCHECK(hipMemcpy(&s, dev, sizeof(s), hipMemcpyDeviceToHost));
    if (tau) *tau = s.tau;
    if (sig2) *sig2 = s.sig2;
    if (alpha) *alpha = s.alpha;
}
void scalars_write(DevScalars *dev, double tau, double sig2, double alpha) {
    DevScalars s;
    HIPCHECK(hipMemcpy(&s, dev, sizeof(s), hipMemcpyDeviceToHost));
    s.tau = tau;
    s.sig2 = sig2;
    s.alpha = alpha;
    HIPCHECK(hipMemcpy(dev, &s, sizeof(s), hipMemcpyHostToDevice));
}

// The output traces of a .C sampler call: P x M (M) column-major, or P x M x K (M x K) for K
// chains.  `lam` is lambda, or omega for the triangle mixture, whose u and shape are optional.
struct Traces {
    double *beta, *lam, *sig2, *tau, *alpha, *u = nullptr, *shape = nullptr;
    // chain k's P x M (M) slice of K chains' outputs
    Traces chain(size_t k, size_t p, size_t m) const {
        auto at = [&](double *q, size_t w) { return q ? q + k * w * m : nullptr; };
        return {at(beta, p), at(lam, p), at(sig2, 1), at(tau, 1), at(alpha, 1), at(u, p),
                at(shape, p)};
    }
};

// The outputs of a .C summary call, K chains of Q = P + 3 parameters (beta, sig2, tau, alpha):
// mean, var Q x K, acov (L + 1) x Q x K, hmean, hvar 2 x Q x K column-major, flags K.
// The pooled quantile outputs of a `_q` summary entry (TraceQuantiles::get): probs nprobs,
// centre Q, zlo, zhi, below, inbin [Q][nprobs], counts [Q][6].
struct QuantOut {
    const double *probs;
    int nprobs;
    double *centre, *zlo, *zhi, *below, *inbin, *counts;
};

struct SummaryOut {
    double *mean, *var, *acov, *hmean, *hvar;
    int *flags;
    int maxlag;
    const QuantOut *quant = nullptr;  // pooled over the chains: the same for every slice
    // chain k's slice
    SummaryOut chain(size_t k, size_t q) const {
        return {mean + k * q, var + k * q, acov + k * q * (maxlag + 1), hmean + 2 * k * q,
                hvar + 2 * k * q, flags + k, maxlag, quant};
    }
};

// Enqueue throttle of the .C drivers: mark() records the work enqueued so far on a stream and
// waits until at most two marked blocks are ahead of the device.
struct Throttle {
    hipEvent_t evring[3] = {nullptr, nullptr, nullptr};
    long nmarks = 0;
    ~Throttle() {
        for (auto e : evring)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(hipStream_t stream) {
        hipEvent_t &e = evring[nmarks % 3];
        if (!e) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(e, stream));
        if (nmarks >= 2) HIPCHECK(hipEventSynchronize(evring[(nmarks - 2) % 3]));
        ++nmarks;
    }
};

// The C ABI's accessors over one chain's view, an engine's or chain c's of a batch: each makes
// the f(view) that bb_engine::with_view or bb_chains::with_chain runs once the stream has
// drained.  Trace ring slots (a null output is skipped), the current state, the triangle
// mixture's u, the logistic omega.
auto chain_get_trace(int slot0, int count, const Traces &o) {
    return [=](const ChainView &v) {
        const size_t pl = (size_t)v.p;
        ring_fetch(slot0, count, v.cap,
                   {{o.beta, v.tr.beta, pl}, {o.lam, v.tr.lam, pl}, {o.sig2, v.tr.sig2, 1},
                    {o.tau, v.tr.tau, 1}, {o.alpha, v.tr.alpha, 1}, {o.u, v.tr.u, pl},
                    {o.shape, v.tr.shape, pl}});
    };
}
auto chain_get_state(double *beta, double *lambda, double *tau, double *sig2, double *alpha) {
    return [=](const ChainView &v) {
        const size_t pb = (size_t)v.p * sizeof(double);
        if (beta) HIPCHECK(hipMemcpy(beta, v.st.beta, pb, hipMemcpyDeviceToHost));
        if (lambda) HIPCHECK(hipMemcpy(lambda, v.st.lam, pb, hipMemcpyDeviceToHost));
        scalars_read(v.st.sc, tau, sig2, alpha);
    };
}
auto chain_set_state(const double *beta, double tau, double sig2, double alpha) {
    return [=](const ChainView &v) {
        HIPCHECK(hipMemcpy(v.st.beta, beta, (size_t)v.p * sizeof(double), hipMemcpyHostToDevice));
        scalars_write(v.st.sc, tau, sig2, alpha);
    };
}
auto chain_set_tri_state(const double *u) {
    return [=](const ChainView &v) {
        HIPCHECK(hipMemcpy(v.st.u, u, (size_t)v.p * sizeof(double), hipMemcpyHostToDevice));
    };
}
auto chain_get_omega(double *omega) {
    return [=](const ChainView &v) {
        HIPCHECK(hipMemcpy(omega, v.omega, (size_t)v.n * sizeof(double), hipMemcpyDeviceToHost));
    };
}

// Trace slots [slot0, slot0 + count) of EVERY one of the K chains of `v` -> samples [s0, s0 +
// count) of the P x M x K (M x K) outputs: one strided copy per contiguous run of ring and trace.
void chain_copy_out(const ChainView &v, int K, int slot0, int count, int s0, int m,
                    const Traces &o) {
    const int cap = v.cap;
    auto strided = [&](double *dst, const double *src, size_t w, int k, int sl, int run) {
        if (!dst) return;
        if (K == 1 || (run == cap && run == m)) {  // one contiguous block (no ring wrap)
            ring_copy(dst + (size_t)(s0 + k) * w, src + (size_t)sl * w, (size_t)K * run * w);
            return;
        }
        HIPCHECK(hipMemcpy2D(dst + (size_t)(s0 + k) * w, (size_t)m * w * sizeof(double),
                             src + (size_t)sl * w, (size_t)cap * w * sizeof(double),
                             (size_t)run * w * sizeof(double), (size_t)K,
                             hipMemcpyDeviceToHost));
    };
    const size_t p = (size_t)v.p;
    ring_runs(slot0, count, cap, [&](int k, int sl, int run) {
        strided(o.beta, v.tr.beta, p, k, sl, run);
        strided(o.lam, v.tr.lam, p, k, sl, run);
        strided(o.sig2, v.tr.sig2, 1, k, sl, run);
        strided(o.tau, v.tr.tau, 1, k, sl, run);
        strided(o.alpha, v.tr.alpha, 1, k, sl, run);
        strided(o.u, v.tr.u, p, k, sl, run);
        strided(o.shape, v.tr.shape, p, k, sl, run);
    });
}

}  // namespace

// ---------------------------------------------------------------------------
// Chain batch: K chains of one small design, a workgroup each (bb_small.hip k_small_chains;
// the triangle mixture: bb_tri.hip k_tri_chains, with omega in lam; the logistic bridge:
// bb_logit_chain.hip k_logit_chains, with each chain's last Polya-Gamma omega in `omega`).
// One engine (`proto`, never run) holds what the chains share -- X, y, X'X, X'y, the
// triangle mixture's SVD basis and the least-squares start -- and makes each chain's pre-burn
// draw under that chain's key; the state, the error word and the trace rings are per chain
// ([chain][p], [chain][slot][p]): `v` views them all, v.at(c) chain c's.
// ---------------------------------------------------------------------------
struct bb_chains {
    bb_engine *proto = nullptr;
    int K = 0;
    std::vector<void *> owned;
    ChainView v;  // u and shape: the triangle mixture's alone; omega ([chain][n]): the logistic
    DevScalars *sc0 = nullptr;  // the scalars every chain starts from
    Throttle ahead;
    uint64_t base_stream = 0;
    ChainPath path;  // chain_plan's family at creation, with the batch's instance

    bool tri() const { return path.kind == CK_TRI; }
    bool logit() const { return path.kind == CK_LOGIT; }
    ~bb_chains() {
        if (proto && proto->stream) (void)hipStreamSynchronize(proto->stream);
        for (void *q : owned) (void)hipFree(q);
        delete proto;
    }
    hipStream_t stream() const { return proto->stream; }
    ChainView chain(int c) const {
        if (c < 0 || c >= K) throw HipError("chain index out of range");
        return v.at(c);
    }
    // f(chain c's view) once c is in range, `refusal` is null and the stream has drained
    template <class F>
    int with_chain(int c, const char *refusal, F f) {
        return guarded([&] {
            const ChainView vc = chain(c);
            if (refusal) throw HipError(refusal);
            HIPCHECK(hipStreamSynchronize(stream()));
            f(vc);
        });
    }

    void init_state() {
        bb_engine *e = proto;
        hipStream_t s = e->stream;
        const size_t pb = (size_t)v.p * sizeof(double);
        auto d2d = [&](void *dst, const void *src, size_t bytes) {
            HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
        };
        e->cfg.stream = base_stream;
        engine_init_state_local(e);  // least-squares start, starting scalars, X beta
        d2d(sc0, e->sc, sizeof(DevScalars));
        if (!tri()) HIPCHECK(hipMemsetAsync(v.st.lam, 0, (size_t)K * pb, s));
        for (int c = 0; c < K; ++c) {
            const ChainView vc = v.at(c);
            // the pre-burn draw under the chain's own key, from the shared starting scalars
            d2d(e->sc, sc0, sizeof(DevScalars));
            e->clear_err();
            e->cfg.stream = base_stream + (uint64_t)c;
            engine_preburn_draw(e);
            if (tri()) {  // u = 0.5, omega = 1 and their trace slot 0, as engine_init_state_local
                d2d(vc.st.u, e->u, pb);
                d2d(vc.st.lam, e->lam, pb);
                d2d(vc.tr.u, e->tr_u, pb);
                d2d(vc.tr.lam, e->tr_lam, pb);
            }
            d2d(vc.st.beta, e->beta, pb);
            d2d(vc.st.sc, e->sc, sizeof(DevScalars));
            d2d(vc.st.err, e->err, sizeof(uint32_t));
            // trace slot 0: the starting values, as a single engine leaves them
            d2d(vc.tr.beta, e->beta, pb);
            d2d(vc.tr.tau, e->tr_tau, sizeof(double));
            d2d(vc.tr.sig2, e->tr_sig2, sizeof(double));
            d2d(vc.tr.alpha, e->tr_alpha, sizeof(double));
        }
        e->cfg.stream = base_stream;
        e->clear_err();
        HIPCHECK(hipStreamSynchronize(s));
    }

    // The optional device-side summary of all K chains (bb_summary.hip): created by
    // summary_reset, fed ring slots on the batch's stream behind the sweeps that wrote them.
    std::unique_ptr<TraceSummary> summary;
    void summary_reset(int nsamp, int maxlag) {
        if (!summary) summary.reset(new TraceSummary());
        quant.reset();  // a sketch belongs to one summary: quantiles_reset enables it again
        summary->reset(stream(), K, v.p + 3, nsamp, maxlag);
    }
    void summary_add(int slot0, int count, int s0) {
        if (!summary) throw HipError("summary: add before reset");
        summary->add(stream(), v.ring(), slot0, count, s0);
        if (quant) quant->add(stream(), v.ring(), K, slot0, count, s0);
    }
    // The optional pooled quantile sketch (bb_quantile.hip) of the samples the summary takes:
    // enabled after summary_reset and before the first summary_add, fed by summary_add.
    std::unique_ptr<TraceQuantiles> quant;
    void quantiles_reset() {
        if (!summary) throw HipError("quantiles: reset after summary_reset");
        if (summary->next != 0) throw HipError("quantiles: reset before the first summary_add");
        if (!quant) quant.reset(new TraceQuantiles());
        try {
            quant->reset(stream(), K, v.p + 3, summary->M);
        } catch (...) {
            quant.reset();
            throw;
        }
    }
    void quantiles_get(const double *probs, int nprobs, double *centre, double *zlo, double *zhi,
                       double *below, double *inbin, double *counts) {
        if (!quant) throw HipError("quantiles: get before reset");
        quant->get(stream(), probs, nprobs, centre, zlo, zhi, below, inbin, counts);
    }
    // the summaries and every chain's error word (any output may be null)
    void summary_get(double *mean, double *var, double *acov, double *hmean, double *hvar,
                     int *flags) {
        if (!summary) throw HipError("summary: get before reset");
        summary->get(stream(), mean, var, acov, hmean, hvar);
        if (flags) {
            static_assert(sizeof(int) == sizeof(uint32_t), "flags are 32-bit words");
            HIPCHECK(hipMemcpy(flags, v.st.err, (size_t)K * sizeof(uint32_t),
                               hipMemcpyDeviceToHost));
        }
    }
};

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

const char *bb_version(void) { return "bayesbridge_amd 0.1 (gfx950)"; }
const char *bb_last_error(void) { return g_last_error.c_str(); }

int bb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bb_compute_units(int device) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return cus;
}

void bb_set_seed(uint64_t seed) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_seed = seed;
    g_stream = 0;
}
void bb_get_rng_state(uint64_t *seed, uint64_t *stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (seed) *seed = g_seed;
    if (stream) *stream = g_stream;
}
void bb_set_rng_state(uint64_t seed, uint64_t stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_seed = seed;
    g_stream = stream;
}
void bb_use_r_rng(int enable) { g_use_r_rng = enable; }
int bb_set_device(int device) {
    if (device < 0 || device >= bb_device_count()) {
        set_error("invalid device %d", device);
        return -1;
    }
    g_device = device;
    return 0;
}
void bb_set_verbose(int verbose) { g_verbose = verbose; }

void bb_config_default(bb_config *c) {
    memset(c, 0, sizeof(*c));
    c->world = 1;
    c->sig2_shape = 0.0;
    c->sig2_scale = 0.0;
    c->nu_shape = 2.0;
    c->nu_rate = 2.0;
    c->alpha_a = 1.0;
    c->alpha_b = 1.0;
    c->true_alpha = 0.5;
    c->trace_capacity = 1;
    c->seed = 0xB4E5B41D6EULL;
    // Woodbury Gram: Ozaki-II int8 (fp64-accurate, ~2x faster at C3); cfg.gram_mode = 0
    // selects the fp64 MFMA Gram
    c->gram_mode = 1;
}

// the engine of a dense (X_local) or sparse (spin) design
static int engine_create(const bb_config *cfg, const double *X_local, const double *y,
                         const SparseIn *spin, bb_engine **out) {
    *out = nullptr;
    bb_engine *e = new bb_engine();
    const int rc = guarded([&] {
        e->cfg = *cfg;
        if (e->cfg.p_local <= 0) e->cfg.p_local = e->cfg.p;
        if (e->cfg.world < 1) e->cfg.world = 1;
        if (cfg->n <= 0 || cfg->p <= 0) throw HipError("n and p must be positive");
        engine_setup(e, X_local, y, spin);
    });
    if (rc == 0)
        *out = e;
    else
        delete e;
    return rc;
}

int bb_engine_create(const bb_config *cfg, const double *X_local, const double *y,
                     bb_engine **out) {
    return engine_create(cfg, X_local, y, nullptr, out);
}

int bb_engine_create_csc(const bb_config *cfg, const int *colptr, const int *rowidx,
                         const double *val, const double *y, bb_engine **out) {
    const SparseIn sp{colptr, rowidx, val};
    return engine_create(cfg, nullptr, y, &sp, out);
}

long long bb_engine_sparse_pairs(const bb_engine *e) {
    return e->sparse() ? (long long)e->spd.pairs : -1;
}

int bb_engine_sparse_info(const bb_engine *e, long long *pairs, long long *nnz, int *max_row,
                          int *col_mode) {
    if (!e->sparse()) {
        set_error("not a sparse-design engine");
        return -1;
    }
    if (pairs) *pairs = (long long)e->spd.pairs;
    if (nnz) *nnz = (long long)e->spd.nnz;
    if (max_row) *max_row = e->spd.max_row;
    if (col_mode) *col_mode = e->spd.col_mode ? 1 : 0;
    return 0;
}

void bb_engine_destroy(bb_engine *e) { delete e; }

int bb_comm_id_size(void) { return (int)sizeof(ncclUniqueId); }
int bb_comm_unique_id(void *id_bytes) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) {
        set_error("ncclGetUniqueId failed");
        return -1;
    }
    memcpy(id_bytes, &id, sizeof(id));
    return 0;
}
// Every shard must cap the Chebyshev iterations alike, or ranks deciding from the same reduced
// sums would take different paths and post different collectives (a hang, or buffers mixed
// between exchanges).  The cost model's inputs differ between shards (p_loc, p_pad, the sparse
// non-zeros and pairs), so the ranks take the least of their caps: here through the
// new communicator, for groups in group_create.
static void agree_kmax_ranks(bb_engine *e) {
    double *buf = nullptr;
    HIPCHECK(hipMalloc(&buf, sizeof(double)));
    const double mine = e->nid ? (double)e->nid_kmax : 0.0;
    double got = mine;
    try {
        HIPCHECK(hipMemcpyAsync(buf, &mine, sizeof(double), hipMemcpyHostToDevice, e->stream));
        NCCLCHECK(ncclAllReduce(buf, buf, 1, ncclFloat64, ncclMin, e->comm, e->stream));
        HIPCHECK(hipMemcpyAsync(&got, buf, sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
    } catch (...) {
        (void)hipFree(buf);
        throw;
    }
    (void)hipFree(buf);
    if (e->nid) e->nid_kmax = (int)got;
}

int bb_engine_comm_init(bb_engine *e, const void *id_bytes) {
    return guarded(e->cfg.device, [&] {
        ncclUniqueId id;
        memcpy(&id, id_bytes, sizeof(id));
        NCCLCHECK(ncclCommInitRank(&e->comm, e->cfg.world, id, e->cfg.rank));
        agree_kmax_ranks(e);
    });
}

int bb_engine_init_state(bb_engine *e) {
    return guarded(e->cfg.device, [&] { engine_init_state(e); });
}

int bb_engine_run(bb_engine *e, uint64_t t0, int count, int first_slot, int slot_step,
                  int mcmc_phase) {
    return guarded(e->cfg.device, [&] {
        e->run(t0, count, first_slot, slot_step, mcmc_phase);
        HIPCHECK(hipGetLastError());
    });
}

int bb_engine_sync(bb_engine *e) {
    return guarded([&] { HIPCHECK(hipStreamSynchronize(e->stream)); });
}

int bb_engine_get_trace(bb_engine *e, int slot0, int count, double *beta, double *lambda,
                        double *sig2, double *tau, double *alpha) {
    return e->with_view(nullptr, chain_get_trace(slot0, count, {beta, lambda, sig2, tau, alpha}));
}

int bb_engine_get_state(bb_engine *e, double *beta, double *lambda, double *tau, double *sig2,
                        double *alpha) {
    return e->with_view(nullptr, chain_get_state(beta, lambda, tau, sig2, alpha));
}

int bb_engine_set_state(bb_engine *e, const double *beta, double tau, double sig2,
                        double alpha) {
    return e->with_view(nullptr, [&](const ChainView &v) {
        chain_set_state(beta, tau, sig2, alpha)(v);
        e->xbeta();
        HIPCHECK(hipStreamSynchronize(e->stream));
    });
}

int bb_engine_method(const bb_engine *e) { return e->method; }

int bb_engine_get_omega(bb_engine *e, double *omega) {
    return e->with_view(e->logit() ? nullptr : "not a logistic engine", chain_get_omega(omega));
}

int bb_engine_get_tri_trace(bb_engine *e, int slot0, int count, double *u, double *shape) {
    return e->with_view(e->tri() ? nullptr : "not a triangle-method engine",
                        chain_get_trace(slot0, count, {.u = u, .shape = shape}));
}

int bb_engine_set_tri_state(bb_engine *e, const double *u) {
    return e->with_view(e->tri() ? nullptr : "not a triangle-method engine",
                        chain_set_tri_state(u));
}

int bb_engine_get_tri_basis(bb_engine *e, double *tV, double *a, double *d) {
    if (!e->tri()) {
        set_error("not a triangle-method engine");
        return -1;
    }
    if (tV) memcpy(tV, e->h_tV.data(), e->h_tV.size() * sizeof(double));
    if (a) memcpy(a, e->h_a.data(), e->h_a.size() * sizeof(double));
    if (d) memcpy(d, e->h_d.data(), e->h_d.size() * sizeof(double));
    return 0;
}
int bb_engine_gram_mode(const bb_engine *e) { return e->cfg.gram_mode; }

int bb_engine_enable_timing(bb_engine *e, int enable) {
    e->timing = enable != 0;
    e->timing_level = enable == 1 ? 1 : 2;
    return 0;
}

int bb_engine_set_timed_phase(bb_engine *e, int phase) {
    if (phase < 0 || phase >= PH_END) {
        set_error("bb_engine_set_timed_phase: phase %d out of range", phase);
        return -1;
    }
    e->timed_phase = phase;
    return 0;
}

int bb_engine_set_timing_stride(bb_engine *e, int stride) {
    if (stride < 1) {
        set_error("bb_engine_set_timing_stride: stride %d < 1", stride);
        return -1;
    }
    e->timing_stride = stride;
    return 0;
}

int bb_engine_reset_timing(bb_engine *e) {
    (void)hipStreamSynchronize(e->stream);
    e->sweep_marks.clear();
    e->ev_next = 0;
    return 0;
}

int bb_engine_phase_times(bb_engine *e, double *ms, int cap, int *samples) {
    return guarded([&] {
        HIPCHECK(hipStreamSynchronize(e->stream));
        std::vector<double> acc(PH_COUNT, 0.0);
        for (auto &marks : e->sweep_marks)
            for (size_t i = 0; i + 1 < marks.size(); ++i) {
                float v = 0;
                HIPCHECK(hipEventElapsedTime(&v, e->ev_pool[marks[i].second],
                                             e->ev_pool[marks[i + 1].second]));
                acc[marks[i].first] += v;
            }
        const double ns = e->sweep_marks.empty() ? 1.0 : (double)e->sweep_marks.size();
        for (int i = 0; i < cap && i < PH_COUNT; ++i) ms[i] = acc[i] / ns;
        if (samples) *samples = (int)e->sweep_marks.size();
    });
}

const char *bb_phase_name(int i) { return (i >= 0 && i < PH_COUNT) ? kPhaseNames[i] : ""; }
int bb_phase_count(void) { return PH_COUNT; }

int bb_engine_kernel_times(bb_engine *e, double *gram_ms_avg, double *sweep_ms_avg,
                           int *samples) {
    return guarded([&] {
        HIPCHECK(hipStreamSynchronize(e->stream));
        double g = 0, s = 0;
        int ng = 0, ns = 0;
        for (auto &marks : e->sweep_marks) {
            for (size_t i = 0; i + 1 < marks.size(); ++i)
                if (marks[i].first == e->timed_phase) {
                    float v = 0;
                    HIPCHECK(hipEventElapsedTime(&v, e->ev_pool[marks[i].second],
                                                 e->ev_pool[marks[i + 1].second]));
                    g += v;
                    ++ng;
                }
            if (marks.size() >= 2) {
                float v = 0;
                HIPCHECK(hipEventElapsedTime(&v, e->ev_pool[marks.front().second],
                                             e->ev_pool[marks.back().second]));
                s += v;
                ++ns;
            }
        }
        if (gram_ms_avg) *gram_ms_avg = ng ? g / ng : 0.0;
        if (sweep_ms_avg) *sweep_ms_avg = ns ? s / ns : 0.0;
        if (samples) *samples = ns;
    });
}

int bb_engine_timed_brackets(bb_engine *e, int *count) {
    int ng = 0;
    for (auto &marks : e->sweep_marks)
        for (size_t i = 0; i + 1 < marks.size(); ++i)
            if (marks[i].first == e->timed_phase) ++ng;
    *count = ng;
    return 0;
}

int bb_engine_nid_mixed(bb_engine *e, unsigned long long *mixed_sweeps,
                        unsigned long long *products32, double *eta, int *k2, int *holds_x32) {
    return guarded([&] {
        NidState h{};
        if (e->nid) {
            HIPCHECK(hipMemcpyAsync(&h, e->nid, sizeof(h), hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
        }
        if (mixed_sweeps) *mixed_sweeps = h.n_mixed;
        if (products32) *products32 = h.n_products32;
        if (eta) *eta = h.eta;
        if (k2) *k2 = h.k2;
        if (holds_x32) *holds_x32 = e->X32 != nullptr;
    });
}

int bb_engine_nid_beta32(bb_engine *e, unsigned long long *beta32_sweeps, int *b32) {
    return guarded([&] {
        NidState h{};
        if (e->nid) {
            HIPCHECK(hipMemcpyAsync(&h, e->nid, sizeof(h), hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
        }
        if (beta32_sweeps) *beta32_sweeps = h.n_beta32;
        if (b32) *b32 = h.b32;
    });
}

int bb_engine_nid_resid(bb_engine *e, unsigned long long *resid_sweeps,
                        unsigned long long *redo_sweeps, double *ratio) {
    return guarded([&] {
        NidState h{};
        if (e->nid) {
            HIPCHECK(hipMemcpyAsync(&h, e->nid, sizeof(h), hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
        }
        if (resid_sweeps) *resid_sweeps = h.n_resid;
        if (redo_sweeps) *redo_sweeps = h.n_redo;
        if (ratio) *ratio = h.ratio;
    });
}

int bb_engine_nid_bound(bb_engine *e, double *lambda_x, int *kmax) {
    if (lambda_x) *lambda_x = e->lambda_x;
    if (kmax) *kmax = e->nid ? std::min(g_nid_kmax, e->nid_kmax) : -1;
    return 0;
}

int bb_engine_nid_stats(bb_engine *e, unsigned long long *cheb_sweeps,
                        unsigned long long *products, unsigned long long *chol_sweeps,
                        double *eps, int *mode) {
    return guarded([&] {
        NidState h{};
        if (e->nid) {
            HIPCHECK(hipMemcpyAsync(&h, e->nid, sizeof(h), hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
        }
        if (cheb_sweeps) *cheb_sweeps = h.n_cheb;
        if (products) *products = h.n_products;
        if (chol_sweeps) *chol_sweeps = h.n_chol;
        if (eps) *eps = e->nid ? h.eps : -1.0;
        if (mode) *mode = e->nid ? h.mode : -1;
    });
}

int bb_kernel_instance(const char *phase, char *buf, int len) {
    static const char *kFam[KF_COUNT] = {"lambda", "gram", "reduce", "chol", "solve", "beta",
                                         "eapply"};
    if (!phase || !buf || len <= 0) return -1;
    buf[0] = 0;
    int f = -1;
    for (int i = 0; i < KF_COUNT; ++i)
        if (!strcmp(phase, kFam[i])) f = i;
    const void *k = launched_instance(f);
    if (!k) return -1;
    const char *mangled = hipKernelNameRefByPtr(k, nullptr);
    if (!mangled) return -1;
    int st = 0;
    char *dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
    std::string name = (st == 0 && dem) ? dem : mangled;
    free(dem);
    // "void bb::k_eapply<8, false>(double const*, ...)" -> "bb::k_eapply<8, false>" (the form
    // tools/profile_summary.py gives rocprofv3's kernel names)
    if (name.rfind("void ", 0) == 0) name = name.substr(5);
    int depth = 0;
    for (size_t i = 0; i < name.size(); ++i) {
        if (name[i] == '<') ++depth;
        if (name[i] == '>') --depth;
        if (name[i] == '(' && depth == 0) {
            name.resize(i);
            break;
        }
    }
    snprintf(buf, (size_t)len, "%s", name.c_str());
    return 0;
}

int bb_engine_launch_counts(bb_engine *e, unsigned long long *lambda_xu,
                            unsigned long long *lambda_alone) {
    if (lambda_xu) *lambda_xu = e->n_lambda_xu;
    if (lambda_alone) *lambda_alone = e->n_lambda_alone;
    return 0;
}

int bb_engine_error_flags(bb_engine *e, uint32_t *flags) {
    return guarded([&] { *flags = e->read_err(); });
}

// ---------------------------------------------------------------------------
// Chain batch (struct bb_chains above)
// ---------------------------------------------------------------------------
int bb_chain_kernel(const bb_config *cfg, int batch) {
    g_last_error.clear();
    const ChainPlan plan = chain_plan(*cfg, batch != 0);
    if (batch && plan.refusal) set_error("%s", plan.refusal);
    return plan.kind;
}

int bb_chains_create(const bb_config *cfg, int nchains, const double *X, const double *y,
                     bb_chains **out) {
    *out = nullptr;
    if (nchains < 1) {
        set_error("bb_chains_create: nchains must be at least 1 (got %d)", nchains);
        return -1;
    }
    const ChainPlan plan = chain_plan(*cfg, true);
    if (plan.refusal) {
        set_error("bb_chains_create: %s", plan.refusal);
        return -1;
    }
    bb_chains *b = new bb_chains();
    try {
        bb_config c = *cfg;
        b->K = nchains;
        b->base_stream = c.stream;
        c.p_local = c.p;
        c.trace_capacity = 1;  // the shared engine records its own slot 0 only
        if (bb_engine_create(&c, X, y, &b->proto) != 0) throw HipError(g_last_error);
        // the prototype's own plan is the batch's by construction of chain_plan (but for the
        // logistic bridge, whose kernel has no single-chain twin), so this cannot fire
        if (plan.kind != CK_LOGIT && b->proto->path.kind != plan.kind)
            throw HipError("this design does not run as a fused small chain");
        int cus = 0;
        HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device));
        b->path.kind = plan.kind;
        // (alpha sampled, key 26: the 512-thread instance at every K, there is no packed one)
        b->path.packed =
            plan.kind == CK_SMALL && g_chains_packed && nchains >= 2 * cus && !plan.mh;
        // more triangle chains than the 512-thread instance holds at once (one per CU): a
        // narrower instance, several per CU, the same bits
        if (b->tri()) b->path.threads = tri_chains_threads(c.n, c.p, nchains, cus, plan.mh);
        auto &o = b->owned;
        ChainView &v = b->v;
        v.p = c.p;
        v.cap = cfg->trace_capacity < 1 ? 1 : cfg->trace_capacity;
        v.n = c.n;
        const size_t K = (size_t)nchains, p = (size_t)c.p, ring = (size_t)v.cap;
        // [chain][w] doubles, zeroed; `on` false: the family has no such array
        auto rows = [&](size_t w, bool on = true) { return on ? dalloc<double>(K * w, o) : nullptr; };
        v.st = {.beta = rows(p), .lam = rows(p), .u = rows(p, b->tri()),
                .shape = rows(p, b->tri()), .sc = dalloc<DevScalars>(K, o),
                .err = dalloc<uint32_t>(K, o)};
        v.tr = {.beta = rows(ring * p), .lam = rows(ring * p), .sig2 = rows(ring),
                .tau = rows(ring), .alpha = rows(ring), .u = rows(ring * p, b->tri()),
                .shape = rows(ring * p, b->tri())};
        v.omega = rows((size_t)c.n, b->logit());
        b->sc0 = dalloc<DevScalars>(1, o);
    } catch (std::exception &ex) {
        const std::string msg = ex.what();
        delete b;
        set_error("bb_chains_create: %s", msg.c_str());
        return -1;
    }
    *out = b;
    return 0;
}

void bb_chains_destroy(bb_chains *b) { delete b; }
int bb_chains_count(const bb_chains *b) { return b->K; }

int bb_chains_resident_per_cu(const bb_chains *b) {
    if (hipSetDevice(b->proto->cfg.device) != hipSuccess) return -1;
    return b->path.resident_per_cu(b->proto->n, b->v.p, !b->proto->hy.know_alpha);
}

int bb_chains_threads(const bb_chains *b) { return b->path.block_threads(b->v.p); }

int bb_chains_set_threads(bb_chains *b, int threads) {
    if (!b->tri() || hipSetDevice(b->proto->cfg.device) != hipSuccess ||
        tri_chains_resident_per_cu(b->proto->n, b->v.p, threads, !b->proto->hy.know_alpha) < 0) {
        set_error("bb_chains_set_threads: no triangle chain-batch instance of %d threads", threads);
        return -1;
    }
    b->path.threads = threads;
    return 0;
}

int bb_chains_init_state(bb_chains *b) {
    return guarded(b->proto->cfg.device, [&] { b->init_state(); });
}

int bb_chains_run(bb_chains *b, uint64_t t0, int count, int first_slot, int slot_step,
                  int mcmc_phase) {
    // mcmc_phase selects the prior of the alpha MH step (batches created under key 26 or 27)
    return guarded(b->proto->cfg.device, [&] {
        b->path.launch(b->stream(), b->K, b->proto->chain_design(), b->v,
                       b->proto->chain_run(b->base_stream, t0, count, first_slot, slot_step,
                                           b->v.cap, mcmc_phase));
        HIPCHECK(hipGetLastError());
    });
}

int bb_chains_sync(bb_chains *b) {
    return guarded([&] { HIPCHECK(hipStreamSynchronize(b->stream())); });
}

int bb_chains_get_trace(bb_chains *b, int chain, int slot0, int count, double *beta,
                        double *lambda, double *sig2, double *tau, double *alpha) {
    return b->with_chain(
        chain,
        slot0 < 0 || count < 0 ? "bb_chains_get_trace: slot0 and count must be >= 0" : nullptr,
        chain_get_trace(slot0, count, {beta, lambda, sig2, tau, alpha}));
}

int bb_chains_get_state(bb_chains *b, int chain, double *beta, double *lambda, double *tau,
                        double *sig2, double *alpha) {
    return b->with_chain(chain, nullptr, chain_get_state(beta, lambda, tau, sig2, alpha));
}

int bb_chains_set_state(bb_chains *b, int chain, const double *beta, double tau, double sig2,
                        double alpha) {
    return b->with_chain(chain, nullptr, chain_set_state(beta, tau, sig2, alpha));
}

int bb_chains_get_omega(bb_chains *b, int chain, double *omega) {
    return b->with_chain(chain, b->logit() ? nullptr : "not a logistic chain batch",
                         chain_get_omega(omega));
}

int bb_chains_get_tri_trace(bb_chains *b, int chain, int slot0, int count, double *u,
                            double *shape) {
    return b->with_chain(
        chain,
        !b->tri()                 ? "not a triangle-method chain batch"
        : slot0 < 0 || count < 0 ? "bb_chains_get_tri_trace: slot0 and count must be >= 0"
                                  : nullptr,
        chain_get_trace(slot0, count, {.u = u, .shape = shape}));
}

int bb_chains_set_tri_state(bb_chains *b, int chain, const double *u) {
    return b->with_chain(chain, b->tri() ? nullptr : "not a triangle-method chain batch",
                         chain_set_tri_state(u));
}

int bb_chains_get_tri_basis(bb_chains *b, double *tV, double *a, double *d) {
    if (!b->tri()) {
        set_error("not a triangle-method chain batch");
        return -1;
    }
    return bb_engine_get_tri_basis(b->proto, tV, a, d);
}

int bb_chains_summary_reset(bb_chains *b, int nsamp, int maxlag) {
    return guarded(b->proto->cfg.device, [&] { b->summary_reset(nsamp, maxlag); });
}

int bb_chains_summary_add(bb_chains *b, int slot0, int count, int s0) {
    return guarded(b->proto->cfg.device, [&] { b->summary_add(slot0, count, s0); });
}

int bb_chains_summary_get(bb_chains *b, double *mean, double *var, double *acov, double *hmean,
                          double *hvar, int *flags) {
    return guarded(b->proto->cfg.device,
                   [&] { b->summary_get(mean, var, acov, hmean, hvar, flags); });
}

int bb_chains_quantiles_reset(bb_chains *b) {
    return guarded(b->proto->cfg.device, [&] { b->quantiles_reset(); });
}

int bb_chains_quantiles_get(bb_chains *b, const double *probs, int nprobs, double *centre,
                            double *zlo, double *zhi, double *below, double *inbin,
                            double *counts) {
    return guarded(b->proto->cfg.device, [&] {
        b->quantiles_get(probs, nprobs, centre, zlo, zhi, below, inbin, counts);
    });
}

// ~0u when the flags cannot be read; bb_last_error then says why and is empty otherwise, which
// tells a failure from a flag word with every bit set
unsigned bb_chains_error_flags(bb_chains *b, int chain) {
    g_last_error.clear();
    try {
        uint32_t f = 0;
        HIPCHECK(hipMemcpyAsync(&f, b->chain(chain).st.err, sizeof(f), hipMemcpyDeviceToHost,
                                b->stream()));
        HIPCHECK(hipStreamSynchronize(b->stream()));
        return f;
    } catch (std::exception &ex) {
        set_error("bb_chains_error_flags: %s", ex.what());
        return ~0u;
    }
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Shard groups: several column-shard engines driven by ONE host thread, interleaving their
// phases around the two per-sweep exchanges.  Two exchange modes:
//   - on-device sums: every member on one device (tests the sharded decomposition on one
//     GPU -- RCCL cannot place two ranks on one device);
//   - RCCL: members on distinct devices with communicators from ncclCommInitAll, each
//     exchange one ncclGroupStart / ncclAllReduce per member / ncclGroupEnd on the members'
//     streams.  This is the single-process multi-GPU path behind the .C entry points: R
//     calls .C from one process (BridgeWrapper.R:220-228), SURVEY.md 5 "distributed comm
//     backend".
// ---------------------------------------------------------------------------
struct bb_group {
    std::vector<bb_engine *> members;
    bool rccl = false;
    std::vector<ncclComm_t> comms;
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;
    std::vector<hipEvent_t> mev;
    double *tmp = nullptr;
    size_t tmp_count = 0;
    // an RCCL member failed mid-run: the communicators were aborted (the other members'
    // pending all-reduces can never be matched), so nothing may wait on the streams again
    bool poisoned = false;
    ~bb_group() {
        for (auto *m : members) {
            (void)hipSetDevice(m->cfg.device);
            if (!poisoned) (void)hipStreamSynchronize(m->stream);
            if (rccl) m->comm = nullptr;  // lent by this group
            m->stop = nullptr;
            m->group_member = false;
        }
        for (auto c : comms)
            if (c) ncclCommDestroy(c);
        if (!members.empty()) (void)hipSetDevice(members[0]->cfg.device);
        if (stream && !poisoned) (void)hipStreamSynchronize(stream);
        if (tmp) (void)hipFree(tmp);
        if (ev) (void)hipEventDestroy(ev);
        for (auto e : mev) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // sum buf(member) over members, result written back to every member's buf
    void reduce(double *bb_engine::*buf, size_t count) {
        if (rccl) {
            NCCLCHECK(ncclGroupStart());
            for (size_t i = 0; i < members.size(); ++i)
                NCCLCHECK(ncclAllReduce(members[i]->*buf, members[i]->*buf, count, ncclFloat64,
                                        ncclSum, comms[i], members[i]->stream));
            NCCLCHECK(ncclGroupEnd());
            return;
        }
        HIPCHECK(hipSetDevice(members[0]->cfg.device));
        for (size_t i = 0; i < members.size(); ++i) {
            HIPCHECK(hipEventRecord(mev[i], members[i]->stream));
            HIPCHECK(hipStreamWaitEvent(stream, mev[i], 0));
        }
        HIPCHECK(hipMemcpyAsync(tmp, members[0]->*buf, count * sizeof(double),
                                hipMemcpyDeviceToDevice, stream));
        for (size_t i = 1; i < members.size(); ++i)
            launch_sum_into(stream, members[i]->*buf, tmp, count);
        for (size_t i = 0; i < members.size(); ++i)
            HIPCHECK(hipMemcpyAsync(members[i]->*buf, tmp, count * sizeof(double),
                                    hipMemcpyDeviceToDevice, stream));
        HIPCHECK(hipEventRecord(ev, stream));
        for (auto *m : members) HIPCHECK(hipStreamWaitEvent(m->stream, ev, 0));
    }
    void on(bb_engine *m) { HIPCHECK(hipSetDevice(m->cfg.device)); }
};

// The on-device group as the lanes of sweep_schedule: every stage on each member in turn (on
// its device), the group's reduce as the exchange, and no speculative start.
struct GroupLanes {
    bb_group *g;
    bb_engine *first() const { return g->members[0]; }
    template <class F>
    void each(F f) {
        for (auto *m : g->members) {
            g->on(m);
            f(m);
        }
    }
    void exchange(double *bb_engine::*buf, size_t count) { g->reduce(buf, count); }
    int spec() const { return 0; }
    // every member decided from the same reduced sums with the same cap: a member whose
    // device mode differed would skip both solves (stale w)
    int decide() {
        const int K = first()->nidx_decide_read();
        for (auto *m : g->members)
            if (m != first() && m->nidx_decide_read() != K)
                throw HipError("shard group members decided different near-identity paths");
        return K;
    }
    // phase c holds the persistent Cholesky / backward-solve kernels, which need every
    // workgroup of their grid resident at once: two members' launches on the shared device
    // must not overlap (two C3-sized factorisations side by side each hold part of the CUs and
    // wait on tiles owned by workgroups that cannot start), so the members' phase c run one
    // after another
    void phase_c(uint64_t t, int slot, int mcmc_phase) {
        for (size_t i = 0; i < g->members.size(); ++i) {
            bb_engine *m = g->members[i];
            g->on(m);
            if (i > 0) HIPCHECK(hipStreamWaitEvent(m->stream, g->mev[i - 1], 0));
            m->phase_c(t, slot, mcmc_phase);
            if (i + 1 < g->members.size()) HIPCHECK(hipEventRecord(g->mev[i], m->stream));
        }
    }
};

namespace {

bb_group *group_create(bb_engine **engines, int count, bool rccl) {
    bb_group *g = new bb_group();
    try {
        if (count < 1) throw HipError("empty group");
        for (int i = 0; i < count; ++i) {
            if (engines[i]->cfg.world != count || engines[i]->cfg.rank != i)
                throw HipError("group member rank/world mismatch");
            for (int k = 0; k < i; ++k)
                if ((engines[k]->cfg.device == engines[i]->cfg.device) == rccl)
                    throw HipError(rccl ? "an RCCL group needs its members on distinct devices"
                                        : "an on-device group needs its members on one device "
                                          "(use an RCCL group across devices)");
            if (engines[i]->comm) throw HipError("group members must not own a communicator");
            g->members.push_back(engines[i]);
        }
        size_t c = 0;
        for (auto *m : g->members) {
            c = std::max(c, m->red1_count());
            if (m->woodbury()) c = std::max(c, m->red2_count());
        }
        g->tmp_count = c;
        // one iteration cap for every member (see agree_kmax_ranks); members disagreeing on
        // whether the near-identity path exists at all (n_pad decides it) cannot be grouped
        int kmin = 1 << 30;
        for (auto *m : g->members) {
            if ((m->nid != nullptr) != (g->members[0]->nid != nullptr))
                throw HipError("group members disagree on the near-identity solve (n differs?)");
            if (m->nid) kmin = std::min(kmin, m->nid_kmax);
        }
        for (auto *m : g->members)
            if (m->nid) m->nid_kmax = kmin;
        if (rccl) {
            g->rccl = true;
            std::vector<int> devs(count);
            for (int i = 0; i < count; ++i) devs[i] = engines[i]->cfg.device;
            g->comms.assign(count, nullptr);
            NCCLCHECK(ncclCommInitAll(g->comms.data(), count, devs.data()));
            // each member runs whole sweeps on its own host thread (bb_group_run) and
            // exchanges through its own communicator, as one rank of a multi-process job
            for (int i = 0; i < count; ++i) {
                engines[i]->comm = g->comms[i];
                engines[i]->own_comm = false;
            }
        } else {
            HIPCHECK(hipSetDevice(engines[0]->cfg.device));
            HIPCHECK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
            HIPCHECK(hipEventCreateWithFlags(&g->ev, hipEventDisableTiming));
            for (int i = 0; i < count; ++i) {
                hipEvent_t e;
                HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                g->mev.push_back(e);
            }
            HIPCHECK(hipMalloc(&g->tmp, c * sizeof(double)));
            for (int i = 0; i < count; ++i) engines[i]->group_member = true;
        }
    } catch (std::exception &ex) {
        set_error("%s", ex.what());
        delete g;
        return nullptr;
    }
    return g;
}

}  // namespace

extern "C" {

int bb_group_create(bb_engine **engines, int count, bb_group **out) {
    *out = group_create(engines, count, false);
    return *out ? 0 : -1;
}

int bb_group_create_rccl(bb_engine **engines, int count, bb_group **out) {
    *out = group_create(engines, count, true);
    return *out ? 0 : -1;
}

void bb_group_destroy(bb_group *g) { delete g; }

int bb_group_run(bb_group *g, uint64_t t0, int count, int first_slot, int slot_step,
                 int mcmc_phase) {
    if (g->poisoned) {
        set_error("shard group unusable: a member failed in an earlier run and its "
                  "communicators were aborted");
        return -1;
    }
    if (g->rccl) {
        // one enqueue thread per device: member i runs its `count` sweeps exactly as rank i
        // of a one-process-per-GPU job would (phase a, all-reduce, phase b, all-reduce,
        // phase c on its own stream and communicator), so the host cost per sweep does not
        // grow with the device count
        const size_t k = g->members.size();
        std::vector<std::string> errs(k);
        std::vector<std::thread> th;
        std::atomic<bool> stop{false};
        const int fail_member = g_debug_fail_member.exchange(-1), fail_sweep = g_debug_fail_sweep.load();
        th.reserve(k);
        for (size_t i = 0; i < k; ++i)
            th.emplace_back([&, i] {
                bb_engine *m = g->members[i];
                m->stop = &stop;
                m->fail_at = (int)i == fail_member ? fail_sweep : -1;
                try {
                    HIPCHECK(hipSetDevice(m->cfg.device));
                    m->run(t0, count, first_slot, slot_step, mcmc_phase);
                    HIPCHECK(hipGetLastError());
                } catch (std::exception &ex) {
                    errs[i] = ex.what();
                    stop.store(true);  // the others stop enqueueing sweeps
                }
                m->fail_at = -1;
            });
        for (auto &t : th) t.join();
        for (size_t i = 0; i < k; ++i)
            if (!errs[i].empty()) {
                set_error("group member %zu: %s", i, errs[i].c_str());
                // A member stopped part-way through its sweeps, so the all-reduces the others
                // already enqueued can never be matched: abort every communicator (their
                // pending collectives return) and poison the group, so that neither this call
                // nor the destructor waits on those streams.
                for (auto &c : g->comms)
                    if (c) {
                        (void)ncclCommAbort(c);
                        c = nullptr;
                    }
                for (auto *m : g->members) m->comm = nullptr;
                g->poisoned = true;
                return -1;
            }
        return 0;
    }
    return guarded([&] {
        GroupLanes lanes{g};
        for (int k = 0; k < count; ++k)
            sweep_schedule(lanes, t0 + (uint64_t)k, first_slot < 0 ? -1 : first_slot + k * slot_step,
                           mcmc_phase);
        HIPCHECK(hipGetLastError());
    });
}

int bb_group_sync(bb_group *g) {
    if (g->poisoned) {
        set_error("shard group unusable: a member failed and its communicators were aborted");
        return -1;
    }
    return guarded([&] {
        for (auto *m : g->members) {
            g->on(m);
            HIPCHECK(hipStreamSynchronize(m->stream));
        }
    });
}

int bb_group_init_state(bb_group *g) {
    // p > n (Woodbury) start: beta = 0, then the pre-burn tau draw from the summed red1
    return guarded([&] {
        for (auto *m : g->members) {
            if (m->G != nullptr) throw HipError("group init supports the p > n path only");
            g->on(m);
            engine_init_state_local(m);
        }
        GroupLanes lanes{g};
        if (!g->members[0]->ortho() && !g->members[0]->hy.know_tau) preburn_schedule(lanes, 1);
        for (auto *m : g->members) {
            g->on(m);
            HIPCHECK(hipStreamSynchronize(m->stream));
        }
    });
}

}  // extern "C"

namespace {

// ---------------------------------------------------------------------------
// .C drivers: device selection, trace ring with chunked copy-out, interrupt polling.
// ---------------------------------------------------------------------------
// bb_set_device_count: devices a .C chain may shard over (0: every visible device).  The
// default is 1: a sharded chain sums its Gram in a different fp64 order than one device, and
// p > n chains amplify such roundoff, so traces depend on the device count and
// multi-device sharding is opt-in.
int g_max_devices = 1;
size_t g_trace_budget = size_t(1) << 30;   // device bytes of trace ring per engine
std::atomic<int> g_debug_interrupt{-1};     // bb_debug_interrupt_after (test hook)
int g_last_devices = 0, g_last_interrupted = 0, g_last_capacity = 0;

// R's interrupt machinery, resolved at run time (absent outside R).  The reference polls
// R_CheckUserInterrupt every 10 sweeps (BridgeWrapper.cpp:273-275, 295-297), which longjmps
// out of the sampler; here the check runs under R_ToplevelExec, so a pending interrupt is
// caught without unwinding through frames that own device memory or communicators, the
// chain stops, the device is released, and the interrupt is re-raised from the .C frame.
struct RInterrupt {
    int (*toplevel)(void (*)(void *), void *) = nullptr;  // R_ToplevelExec (Rboolean)
    void (*check)(void) = nullptr;                        // R_CheckUserInterrupt
    void (*onintr)(void) = nullptr;                       // Rf_onintr
    bool tried = false;
    bool ok() {
        if (!tried) {
            tried = true;
            toplevel = (int (*)(void (*)(void *), void *))dlsym(RTLD_DEFAULT, "R_ToplevelExec");
            check = (void (*)(void))dlsym(RTLD_DEFAULT, "R_CheckUserInterrupt");
            onintr = (void (*)(void))dlsym(RTLD_DEFAULT, "Rf_onintr");
        }
        return toplevel && check;
    }
} g_rint;

void r_check_cb(void *) { g_rint.check(); }

bool poll_interrupt() {
    int d = g_debug_interrupt.load();
    while (d >= 0) {  // test hook: the d-th poll from now reports an interrupt
        if (g_debug_interrupt.compare_exchange_weak(d, d == 0 ? -1 : d - 1)) {
            if (d == 0) return true;
            break;
        }
    }
    if (g_rint.ok()) return g_rint.toplevel(r_check_cb, nullptr) == 0;
    return false;
}

// From a .C frame with no live C++ objects: hand the caught interrupt back to R.
void reraise_interrupt() {
    if (g_rint.ok() && g_rint.onintr) g_rint.onintr();
}

// bb_config of a .C bridge_reg_stable call (BridgeWrapper.cpp:659-693)
bb_config stable_call_config(const double *sig2_shape, const double *sig2_scale,
                             const double *nu_shape, const double *nu_rate, const double *alpha_a,
                             const double *alpha_b, const double *true_sig2,
                             const double *true_tau, const double *true_alpha, int p, int n,
                             int m, const int *ortho, int nchains = 1) {
    bb_config c;
    bb_config_default(&c);
    c.n = n;
    c.p = p;
    c.p_local = p;
    c.sig2_shape = *sig2_shape;
    c.sig2_scale = *sig2_scale;
    c.nu_shape = *nu_shape;
    c.nu_rate = *nu_rate;
    c.alpha_a = *alpha_a;
    c.alpha_b = *alpha_b;
    c.true_sig2 = *true_sig2;
    c.true_tau = *true_tau;
    c.true_alpha = *true_alpha;
    c.ortho = *ortho != 0;
    c.trace_capacity = m < 1 ? 1 : m;
    c.device = g_device;
    next_call_key(&c.seed, &c.stream, nchains);
    return c;
}

// Trace ring slots for M samples of p_local coefficients (`ntr` p-long traces per slot):
// the whole run if it fits the per-engine budget, else a ring copied out in chunks.  The
// `chains` rings of a chain batch share the budget: each gets a chains-th.
int ring_capacity(int m, int p_local, int ntr, int chains = 1) {
    const size_t per = (size_t)ntr * p_local * sizeof(double) + 3 * sizeof(double);
    size_t cap = g_trace_budget / ((size_t)chains * per);
    if (cap < 16) cap = 16;
    return (int)std::min<size_t>(cap, (size_t)(m < 1 ? 1 : m));
}

// Devices for a column-sharded chain: 1 unless p > n (the Woodbury path, or the orthogonal
// design; alpha known or unknown) and sharding was enabled (bb_set_device_count); at least
// 4096 columns per device.
int chain_devices(const bb_config &c, int nvis = -1) {
    if (nvis < 0) nvis = bb_device_count();
    int k = g_max_devices > 0 ? std::min(g_max_devices, nvis) : nvis;
    if (c.p <= c.n || (c.method != AUTO && c.method != WOODBURY && c.method != ORTHO)) return 1;
    k = std::min(k, std::max(1, c.p / 4096));
    return std::max(1, k);
}

// "Error: <message>" and the line the reference's samplers end on after an error
__attribute__((format(printf, 1, 2))) void print_abort(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("Error: ");
    vprintf(fmt, ap);
    va_end(ap);
    printf("\nAborting Gibbs sampler.\n");
    fflush(stdout);
}

// One chain: a single engine, or the column shards of a multi-device RCCL group.
struct Chain {
    std::vector<bb_engine *> eng;
    std::vector<int> j0s;
    bb_group *grp = nullptr;
    int p = 0, cap = 1;
    Throttle ahead;

    ~Chain() {
        if (grp) bb_group_destroy(grp);
        for (auto *e : eng) bb_engine_destroy(e);
    }
    int init() { return grp ? bb_group_init_state(grp) : bb_engine_init_state(eng[0]); }
    // sweeps per launch (and per interrupt poll) of a .C call: column shards are never fused
    int block() const { return eng[0]->path.block(); }
    int run(uint64_t t0, int count, int slot, int step, int mcmc) {
        return grp ? bb_group_run(grp, t0, count, slot, step, mcmc)
                   : bb_engine_run(eng[0], t0, count, slot, step, mcmc);
    }
    int sync() { return grp ? bb_group_sync(grp) : bb_engine_sync(eng[0]); }
    uint32_t flags() {
        uint32_t all = 0;
        for (auto *e : eng) {
            uint32_t f = 0;
            (void)hipSetDevice(e->cfg.device);
            if (bb_engine_error_flags(e, &f) == 0) all |= f;
        }
        return all;
    }
    // the numerical failures of a complete run, as the drivers print them
    void report_flags() {
        const uint32_t f = flags();
        if (f & ~4u) print_abort("numerical failure in the device sampler (flags %u)", f);
    }
    // Marks the work enqueued so far (member 0's stream: members advance in lockstep through
    // the exchanges) and waits until at most two marked blocks are ahead of the device.
    void throttle() {
        HIPCHECK(hipSetDevice(eng[0]->cfg.device));
        ahead.mark(eng[0]->stream);
    }
    // trace slots [slot0, slot0 + count) -> samples [s0, s0 + count) of the P x M outputs
    int copy_out(int slot0, int count, int s0, const Traces &o) {
        if (count <= 0) return 0;
        const size_t P = (size_t)p;
        if (eng.size() == 1)  // the batch's copy with one chain
            return guarded([&] {
                HIPCHECK(hipStreamSynchronize(eng[0]->stream));
                chain_copy_out(eng[0]->view(), 1, slot0, count, s0, 0, o);
            });
        for (size_t r = 0; r < eng.size(); ++r) {
            bb_engine *e = eng[r];
            const size_t pl = (size_t)e->p_loc;
            std::vector<double> b(pl * count), l(pl * count);
            (void)hipSetDevice(e->cfg.device);
            if (bb_engine_get_trace(e, slot0, count, b.data(), l.data(),
                                    r == 0 && o.sig2 ? o.sig2 + s0 : nullptr,
                                    r == 0 ? o.tau + s0 : nullptr, r == 0 ? o.alpha + s0 : nullptr))
                return -1;
            for (int k = 0; k < count; ++k) {
                memcpy(o.beta + (s0 + k) * P + j0s[r], &b[k * pl], pl * sizeof(double));
                memcpy(o.lam + (s0 + k) * P + j0s[r], &l[k * pl], pl * sizeof(double));
            }
        }
        return 0;
    }
};

// Builds the chain: `create(cfg, j0, j1, &engine)` makes the engine of columns [j0, j1).
template <class Create>
int chain_build(Chain &ch, bb_config c, int ntr, Create create) {
    const int ndev = chain_devices(c);
    const int nvis = std::max(1, bb_device_count());
    ch.p = c.p;
    if (ndev <= 1) {
        c.trace_capacity = ring_capacity(c.trace_capacity, c.p, ntr);
        ch.cap = c.trace_capacity;
        bb_engine *e = nullptr;
        if (create(&c, 0, c.p, &e) != 0) return -1;
        ch.eng.push_back(e);
        ch.j0s.push_back(0);
        return 0;
    }
    const int per = (c.p + ndev - 1) / ndev;
    const int cap = ring_capacity(c.trace_capacity, per, ntr);
    ch.cap = cap;
    for (int r = 0; r < ndev; ++r) {
        bb_config cr = c;
        const int j0 = r * per, j1 = std::min(c.p, j0 + per);
        cr.p_local = j1 - j0;
        cr.j0 = j0;
        cr.rank = r;
        cr.world = ndev;
        cr.device = (g_device + r) % nvis;
        cr.trace_capacity = cap;
        bb_engine *e = nullptr;
        if (create(&cr, j0, j1, &e) != 0) return -1;
        ch.eng.push_back(e);
        ch.j0s.push_back(j0);
    }
    ch.grp = group_create(ch.eng.data(), ndev, true);
    return ch.grp ? 0 : -1;
}

enum Outcome { OUT_OK = 0, OUT_ERROR = 1, OUT_INTERRUPTED = 2 };

// The schedule of every .C sampler call: burn-in then the MCMC samples, in blocks of kBlock
// sweeps between interrupt polls (at most two blocks queued ahead of the device), the trace
// ring copied out whenever it is full.  Sample s >= 1 runs at t = t_base + s; burn-in is
// `nburn` sweeps in slot 0 from t = 1.  `ch` is what is driven -- a Chain, or a chain batch
// (ChainsRun) -- with init / run / sync / throttle returning 0 or throwing, and `cap` ring
// slots; copy_out(slot0, count, s0) moves ring slots to samples [s0, s0 + count) of the
// caller's outputs, report_flags() prints the numerical failures after a complete run.
template <class C, class CopyOut, class Report>
Outcome drive_schedule(C &ch, int kBlock, int nburn, uint64_t t_base, int m, int b,
                       double *runtime, CopyOut copy_out, Report report_flags) {
    *runtime = 0.0;
    if (ch.init() != 0) return OUT_ERROR;
    bool interrupted = false;
    try {
        auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < nburn && !interrupted; k += kBlock) {
            if (ch.run(1 + (uint64_t)k, std::min(kBlock, nburn - k), 0, 0, 0) != 0)
                return OUT_ERROR;
            ch.throttle();
            interrupted = poll_interrupt();
        }
        if (ch.sync() != 0) return OUT_ERROR;
        auto t1 = std::chrono::steady_clock::now();
        if (g_verbose && !interrupted) {
            const double bt = std::chrono::duration<double>(t1 - t0).count();
            printf("Burn-in complete: %g sec. for %i iterations.\n", bt, b);
            if (b > 0) printf("Expect approx. %g sec. for %i samples.\n", bt * m / b, m);
        }
        int copied = 0, next = 1;  // samples copied out / next sample to compute
        while (copied < m && !interrupted) {
            const int hi = std::min(m, copied + ch.cap);
            for (int s = next; s < hi && !interrupted; s += kBlock) {
                const int cnt = std::min(kBlock, hi - s);
                if (ch.run(t_base + (uint64_t)s, cnt, s % ch.cap, 1, 1) != 0) return OUT_ERROR;
                ch.throttle();
                interrupted = poll_interrupt();
                next = s + cnt;
            }
            if (ch.sync() != 0) return OUT_ERROR;
            if (copy_out(copied % ch.cap, next - copied, copied) != 0) return OUT_ERROR;
            copied = next;
        }
        if (interrupted && copied == 0 && ch.sync() == 0) (void)copy_out(0, 1, 0);
        *runtime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        if (interrupted) {
            printf("Interrupted: %i of %i samples returned.\n", std::max(copied, 1), m);
            return OUT_INTERRUPTED;
        }
        report_flags();
    } catch (std::exception &ex) {
        set_error("%s", ex.what());
        return OUT_ERROR;
    }
    return OUT_OK;
}

void print_banner(const char *title, const bb_config &c, int b, int m) {
    if (!g_verbose) return;  // BridgeWrapper.cpp:235-240 (stable), :112-117 (triangles)
    printf("%s", title);
    if (c.true_alpha > 0) printf(" known alpha=%g", c.true_alpha);
    if (c.true_sig2 > 0 && c.method != LOGIT) printf(", sig2=%g", c.true_sig2);
    if (c.true_tau > 0) printf(", tau=%g", c.true_tau);
    if (c.ortho) printf("\nAssuming orthogonal design matrix!");
    printf("\nBurn-in: %i, Num. Samples: %i\n", b, m);
}

// What tells the samplers' .C calls apart: the banner's title, the p-long traces per ring slot
// and the schedule -- `nburn` burn-in sweeps in slot 0, MCMC sample i at t = t_base + i.
struct CallKind {
    const char *title;
    int ntr, nburn;
    uint64_t t_base;
};
// the stable family (BridgeWrapper.cpp:207-313 / :434-537): B + 1 burn-in sweeps
CallKind stable_kind(int b, const char *title = "Bridge Regression (mix. of normals):") {
    return {title, 2, b + 1, (uint64_t)b + 1};
}
// the triangle mixture (BridgeWrapper.cpp:80-204 / :320-432): `burn` sweeps; a slot is 4
// P-vectors (beta, u, omega, shape)
CallKind tri_kind(int b) {
    return {"Bridge Regression (mix. of triangles):", 4, b, (uint64_t)b};
}

// The frame of every .C sampler call: the banner, `run` (whatever it builds is gone when it
// returns), bb_last_error and the reference's closing line after an error, else the completion
// line -- "of K chains" for a batch (K > 0) -- and the interrupt flag of bb_last_call_info.
template <class Run>
Outcome call_frame(const CallKind &kd, const bb_config &c, int b, int K, double *runtime,
                   Run run) {
    const int m = c.trace_capacity;
    print_banner(kd.title, c, b, m);
    g_last_interrupted = 0;
    *runtime = 0.0;
    const Outcome o = run();
    if (o == OUT_ERROR) print_abort("%s", g_last_error.c_str());
    if (g_verbose && o == OUT_OK) {
        printf("Sampling complete: %g sec. for %i iterations", *runtime, m);
        K > 0 ? printf(" of %i chains.\n", K) : printf(".\n");
    }
    g_last_interrupted = o == OUT_INTERRUPTED;
    return o;
}

// One chain of a .C sampler call over the engines `create` makes.  Errors print and return
// partial traces.
template <class Create>
Outcome sampler_call(const CallKind &kd, const bb_config &c, int b, Create create,
                     const Traces &out, double *runtime) {
    return call_frame(kd, c, b, 0, runtime, [&] {
        Chain ch;
        if (chain_build(ch, c, kd.ntr, create) != 0) return OUT_ERROR;
        g_last_devices = (int)ch.eng.size();
        g_last_capacity = ch.cap;
        return drive_schedule(
            ch, ch.block(), kd.nburn, kd.t_base, c.trace_capacity, b, runtime,
            [&](int slot0, int count, int s0) { return ch.copy_out(slot0, count, s0, out); },
            [&] { ch.report_flags(); });
    });
}

// the engines of a dense column-major X with n rows (a shard takes its columns)
auto dense_create(const double *yp, const double *Xp, int n) {
    return [=](const bb_config *cc, int j0, int, bb_engine **e) {
        return bb_engine_create(cc, Xp + (size_t)j0 * n, yp, e);
    };
}
// ... over such an X
Outcome dense_call(const CallKind &kd, const bb_config &c, const double *yp, const double *Xp,
                   int b, const Traces &out, double *runtime) {
    return sampler_call(kd, c, b, dense_create(yp, Xp, c.n), out, runtime);
}

// A chain batch as drive_schedule drives it: every run advances all K chains.
struct ChainsRun {
    bb_chains *b;
    int cap;
    int init() { return bb_chains_init_state(b); }
    int run(uint64_t t0, int count, int slot, int step, int mcmc) {
        return bb_chains_run(b, t0, count, slot, step, mcmc);
    }
    int sync() { return bb_chains_sync(b); }
    void throttle() { b->ahead.mark(b->stream()); }
};

// K chains of a small design as one batch on drive_schedule, in ChainPath::block()'s blocks.
// The trace budget bounds the batch: each chain's ring gets a K-th.
// With `sum` the ring fills are not copied out but reduced on the device behind the sweeps
// (bb_chains::summary_add), and the summaries come back after a complete run.
Outcome chains_batch(const CallKind &kd, const bb_config &c0, int K, const double *yp,
                     const double *Xp, int b, const Traces &out, double *runtime,
                     const SummaryOut *sum = nullptr) {
    const int m = c0.trace_capacity;
    bb_config c = c0;
    c.trace_capacity = ring_capacity(m, c.p, kd.ntr, K);
    bb_chains *raw = nullptr;
    if (bb_chains_create(&c, K, Xp, yp, &raw) != 0) return OUT_ERROR;
    std::unique_ptr<bb_chains> ch(raw);
    g_last_devices = 1;
    g_last_capacity = ch->v.cap;
    ChainsRun run{raw, ch->v.cap};
    if (sum && bb_chains_summary_reset(raw, m, sum->maxlag) != 0) return OUT_ERROR;
    if (sum && sum->quant && bb_chains_quantiles_reset(raw) != 0) return OUT_ERROR;
    const Outcome o = drive_schedule(
        run, ch->path.block(), kd.nburn, kd.t_base, m, b, runtime,
        [&](int slot0, int count, int s0) {
            if (sum)
                ch->summary_add(slot0, count, s0);
            else
                chain_copy_out(ch->v, K, slot0, count, s0, m, out);
            return 0;
        },
        [&] {
            std::vector<uint32_t> f(K, 0u);
            HIPCHECK(hipMemcpy(f.data(), ch->v.st.err, (size_t)K * sizeof(uint32_t),
                               hipMemcpyDeviceToHost));
            for (int k = 0; k < K; ++k)
                if (f[k] & ~4u)
                    print_abort("numerical failure in the device sampler (flags %u) in chain %i",
                                f[k], k);
        });
    if (sum && o == OUT_OK &&
        bb_chains_summary_get(raw, sum->mean, sum->var, sum->acov, sum->hmean, sum->hvar,
                              sum->flags) != 0)
        return OUT_ERROR;
    if (const QuantOut *q = sum ? sum->quant : nullptr; q && o == OUT_OK &&
        bb_chains_quantiles_get(raw, q->probs, q->nprobs, q->centre, q->zlo, q->zhi, q->below,
                                q->inbin, q->counts) != 0)
        return OUT_ERROR;
    return o;
}

// bridge_reg_stable_chains / bridge_regression_chains: the batch where the fused small chain
// applies, else the K chains one after another through the single-chain driver on streams
// k1 + k.
Outcome chains_call(const CallKind &kd, const bb_config &c, int K, const double *yp,
                    const double *Xp, int b, const Traces &out, double *runtime) {
    const int m = c.trace_capacity;
    *runtime = 0.0;
    if (chain_plan(c, true).kind != CK_NONE)
        return call_frame(kd, c, b, K, runtime,
                          [&] { return chains_batch(kd, c, K, yp, Xp, b, out, runtime); });
    for (int k = 0; k < K; ++k) {
        bb_config ck = c;
        ck.stream = c.stream + (uint64_t)k;
        double rt = 0.0;
        const Outcome o = dense_call(kd, ck, yp, Xp, b, out.chain(k, c.p, m), &rt);
        *runtime += rt;
        if (o == OUT_INTERRUPTED) return o;
    }
    return OUT_OK;
}

// One chain of a summary call on a single engine: its ring ([slot][p], tr_sig2 / tr_tau /
// tr_alpha) is reduced by the chain batch's kernel with one chain.  An interrupted or failed
// run leaves the outputs as they were.
// With `tq` the chain's samples also go to the call's pooled quantile sketch, which the first
// chain sizes for all `nchains` (its first kept draw is the centre).
Outcome summary_chain_call(const CallKind &kd, const bb_config &c, int b, const double *yp,
                           const double *Xp, const SummaryOut &out, double *runtime,
                           TraceQuantiles *tq = nullptr, int nchains = 1) {
    const int m = c.trace_capacity;
    return call_frame(kd, c, b, 0, runtime, [&] {
        Chain ch;
        if (chain_build(ch, c, kd.ntr, dense_create(yp, Xp, c.n)) != 0 || ch.eng.size() != 1) {
            if (ch.eng.size() > 1) set_error("summaries need every column on one device");
            return OUT_ERROR;
        }
        g_last_devices = 1;
        g_last_capacity = ch.cap;
        bb_engine *e = ch.eng[0];
        TraceSummary ts;
        const SummaryRing ring = e->view().ring();
        if (guarded(e->cfg.device, [&] {
                ts.reset(e->stream, 1, c.p + 3, m, out.maxlag);
                if (tq && !tq->ready()) tq->reset(e->stream, nchains, c.p + 3, m);
            }) != 0)
            return OUT_ERROR;
        const Outcome o = drive_schedule(
            ch, ch.block(), kd.nburn, kd.t_base, m, b, runtime,
            [&](int slot0, int count, int s0) {
                HIPCHECK(hipSetDevice(e->cfg.device));
                ts.add(e->stream, ring, slot0, count, s0);
                if (tq) tq->add(e->stream, ring, 1, slot0, count, s0);
                return 0;
            },
            [&] { ch.report_flags(); });
        if (o == OUT_OK &&
            guarded(e->cfg.device, [&] {
                ts.get(e->stream, out.mean, out.var, out.acov, out.hmean, out.hvar);
                *out.flags = (int)ch.flags();
            }) != 0)
            return OUT_ERROR;
        return o;
    });
}

// bridge_reg_stable_chains_summary / bridge_regression_chains_summary: chains_call with the
// ring fills reduced on the device and only the summaries returned.  A chain that would be
// sharded by columns over several devices is refused: every column has to be on one device.
Outcome chains_summary_call(const char *entry, const CallKind &kd, const bb_config &c, int K,
                            const double *yp, const double *Xp, int b, const SummaryOut &out,
                            double *runtime) {
    *runtime = 0.0;
    if (chain_plan(c, true).kind != CK_NONE)
        return call_frame(kd, c, b, K, runtime, [&] {
            return chains_batch(kd, c, K, yp, Xp, b, Traces{}, runtime, &out);
        });
    if (const int ndev = chain_devices(c); ndev > 1) {
        set_error("%s: this design would be sharded by columns over %d devices; summaries need "
                  "every column on one device (bb_set_device_count(1))", entry, ndev);
        print_abort("%s", g_last_error.c_str());
        return OUT_ERROR;
    }
    // one sketch for the whole call: every chain's stream is drained (the summary's get)
    // before the next chain starts, so the adds of the K engines never overlap
    TraceQuantiles tq;
    for (int k = 0; k < K; ++k) {
        bb_config ck = c;
        ck.stream = c.stream + (uint64_t)k;
        double rt = 0.0;
        const Outcome o = summary_chain_call(kd, ck, b, yp, Xp, out.chain(k, c.p + 3), &rt,
                                             out.quant ? &tq : nullptr, K);
        *runtime += rt;
        if (o != OUT_OK) return o;
    }
    if (const QuantOut *q = out.quant) {
        if (guarded(tq.device, [&] {
                tq.get(0, q->probs, q->nprobs, q->centre, q->zlo, q->zhi, q->below, q->inbin,
                       q->counts);
            }) != 0) {
            print_abort("%s", g_last_error.c_str());
            return OUT_ERROR;
        }
    }
    return OUT_OK;
}

Outcome stable_csc(const bb_config &c, const double *yp, const int *Xcolptr, const int *Xrowidx,
                   const double *Xval, int b, const Traces &out, double *runtime) {
    const int p = c.p, n = c.n;
    if (p > n && !c.ortho) {
        return sampler_call(
            stable_kind(b), c, b,
            [&](const bb_config *cc, int j0, int j1, bb_engine **e) {
                // the shard's columns: colptr rebased to its first entry
                std::vector<int> cp(j1 - j0 + 1);
                for (int j = j0; j <= j1; ++j) cp[j - j0] = Xcolptr[j] - Xcolptr[j0];
                return bb_engine_create_csc(cc, cp.data(), Xrowidx + Xcolptr[j0],
                                            Xval + Xcolptr[j0], yp, e);
            },
            out, runtime);
    }
    // p <= n or the orthogonal design: the dense paths of bridge_reg_stable (least-squares
    // start, p x p Cholesky or ortho draw) on the densified X, after the same validation as
    // the sparse engine's
    try {
        csc_validate(n, p, Xcolptr, Xrowidx);
    } catch (std::exception &ex) {
        print_abort("%s", ex.what());
        *runtime = 0.0;
        return OUT_ERROR;
    }
    std::vector<double> Xd((size_t)n * p, 0.0);
    for (int j = 0; j < p; ++j)
        for (int q = Xcolptr[j]; q < Xcolptr[j + 1]; ++q) Xd[(size_t)j * n + Xrowidx[q]] = Xval[q];
    return dense_call(stable_kind(b), c, yp, Xd.data(), b, out, runtime);
}

// the logistic family: the stable driver's schedule under its own banner
CallKind logit_kind(int b) {
    return stable_kind(b, "Bridge Regression (logistic, Polya-Gamma mix. of normals):");
}

Outcome logit_call(bb_config c, const double *yp, const double *Xp, int b, Traces out,
                   double *runtime) {
    c.method = LOGIT;
    for (int i = 0; i < c.n; ++i)
        if (!(yp[i] == 0.0 || yp[i] == 1.0)) {
            print_abort("logistic bridge needs y in {0, 1} (y[%d] = %g)", i, yp[i]);
            *runtime = 0.0;
            return OUT_ERROR;
        }
    std::vector<double> sig2(c.trace_capacity);
    out.sig2 = sig2.data();
    return dense_call(logit_kind(b), c, yp, Xp, b, out, runtime);
}

// a logistic entry's y, checked before a key is taken or an output is touched
bool logit_y_ok(const char *entry, const double *yp, int n) {
    for (int i = 0; i < n; ++i)
        if (!(yp[i] == 0.0 || yp[i] == 1.0)) {
            set_error("%s: logistic bridge needs y in {0, 1} (y[%d] = %g)", entry, i, yp[i]);
            printf("Error: %s\n", g_last_error.c_str());
            fflush(stdout);
            return false;
        }
    return true;
}

// bb_config of a .C bridge_reg_logit_chains call: bridge_reg_logit's (sig2 == 1, no prior on
// it) with the logistic method and K keys taken
bb_config logit_chains_config(const double *nu_shape, const double *nu_rate,
                              const double *alpha_a, const double *alpha_b,
                              const double *true_tau, const double *true_alpha, int p, int n,
                              int m, int nchains) {
    const double zero = 0.0, one = 1.0;
    const int no = 0;
    bb_config c = stable_call_config(&zero, &zero, nu_shape, nu_rate, alpha_a, alpha_b, &one,
                                     true_tau, true_alpha, p, n, m, &no, nchains);
    c.method = LOGIT;
    return c;
}

// a chains entry's nchains, checked before a key is taken or an output is touched
bool nchains_ok(const char *entry, int nchains) {
    if (nchains >= 1) return true;
    set_error("%s: nchains must be at least 1 (got %d)", entry, nchains);
    printf("Error: %s\n", g_last_error.c_str());
    fflush(stdout);
    return false;
}

// a summary entry's (nsamp, maxlag), checked like nchains
bool summary_args_ok(const char *entry, int nsamp, int maxlag) {
    const char *why = TraceSummary::refusal(nsamp, maxlag);
    if (!why) return true;
    set_error("%s: %s (got maxlag %d, %d samples)", entry, why, maxlag, nsamp);
    printf("Error: %s\n", g_last_error.c_str());
    fflush(stdout);
    return false;
}

// a _q summary entry's probabilities and pooled sample count, checked like nchains (q null:
// the entry without quantiles)
bool quant_args_ok(const char *entry, const QuantOut *q, int nchains, int nsamp) {
    if (!q) return true;
    const char *why = TraceQuantiles::probs_refusal(q->probs, q->nprobs);
    if (!why) why = TraceQuantiles::refusal(nchains, nsamp);
    if (!why) return true;
    set_error("%s: %s (got %d probabilities, %d chains of %d samples)", entry, why, q->nprobs,
              nchains, nsamp);
    printf("Error: %s\n", g_last_error.c_str());
    fflush(stdout);
    return false;
}

// bb_config of a .C bridge_regression call: stable_call_config with the triangle method
bb_config tri_call_config(const double *sig2_shape, const double *sig2_scale,
                          const double *nu_shape, const double *nu_rate, const double *alpha_a,
                          const double *alpha_b, const double *true_sig2, const double *true_tau,
                          const double *true_alpha, int p, int n, int m, const int *ortho,
                          const int *betaburn, int nchains = 1) {
    const int no = 0;
    bb_config c = stable_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a, alpha_b,
                                     true_sig2, true_tau, true_alpha, p, n, m, &no, nchains);
    c.method = TRI;
    c.ortho = *ortho != 0;                       // bridge_regression_ortho, :320-432
    c.betaburn = *betaburn > 0 ? *betaburn : 0;  // BridgeRegression.cpp:407
    return c;
}

}  // namespace

extern "C" {

void bb_set_device_count(int count) { g_max_devices = count < 0 ? 0 : count; }

// .C-callable forms of the controls (R's .C passes every argument as a pointer,
// BridgeWrapper.h:164-245; the by-value forms above are for C / ctypes hosts)
void bb_set_device_count_C(const int *count) { bb_set_device_count(*count); }
void bb_get_device_count_C(int *count) { *count = g_max_devices; }
void bb_plan_devices_C(const int *n, const int *p, const int *ortho, const int *nvisible,
                       int *devices) {
    bb_config c;
    bb_config_default(&c);
    c.n = *n;
    c.p = *p;
    c.ortho = *ortho != 0;
    *devices = chain_devices(c, *nvisible >= 0 ? *nvisible : -1);
}
void bb_set_device_C(const int *device, int *status) {
    const int rc = bb_set_device(*device);
    if (status) *status = rc;
}
void bb_set_verbose_C(const int *verbose) { bb_set_verbose(*verbose); }
void bb_use_r_rng_C(const int *enable) { bb_use_r_rng(*enable); }
// R passes numbers as doubles; converting a negative, NaN or out-of-range double to an
// integer type is undefined behaviour, so such a value is refused (the state is kept, the
// reason goes to bb_last_error and stderr) instead of being cast
static bool r_count_ok(const char *what, double v) {
    if (std::isfinite(v) && v >= 0.0 && v <= 9007199254740992.0 && v == std::floor(v)) return true;
    set_error("%s: %g is not an integer in [0, 2^53]; ignored", what, v);
    fprintf(stderr, "BayesBridge: %s: %g is not an integer in [0, 2^53]; ignored\n", what, v);
    return false;
}
void bb_set_seed_C(const double *seed) {
    if (r_count_ok("bb_set_seed_C seed", *seed)) bb_set_seed((uint64_t)*seed);
}
void bb_set_rng_state_C(const double *seed, const double *stream) {
    if (r_count_ok("bb_set_rng_state_C seed", *seed) &&
        r_count_ok("bb_set_rng_state_C stream", *stream))
        bb_set_rng_state((uint64_t)*seed, (uint64_t)*stream);
}
void bb_get_rng_state_C(double *seed, double *stream) {
    uint64_t s = 0, t = 0;
    bb_get_rng_state(&s, &t);
    *seed = (double)s;
    *stream = (double)t;
}
void bb_set_trace_budget_C(const double *bytes) {
    if (r_count_ok("bb_set_trace_budget_C bytes", *bytes)) bb_set_trace_budget((long long)*bytes);
}
void bb_last_call_info_C(int *devices, int *trace_capacity, int *interrupted) {
    (void)bb_last_call_info(devices, trace_capacity, interrupted);
}
void bb_debug_fail_member(int member, int sweep) {
    g_debug_fail_sweep = sweep;
    g_debug_fail_member = member;
}

int bb_set_chol_version(int version) {
    if (version == 0) return g_chol_version;  // query
    if (version < 1 || version > 4) return -1;
    g_chol_version = version;
    return 0;
}
int bb_set_tuning(int key, int value) {
    // one row per key: its variable and the largest value it takes (1: a switch, any non-zero
    // value turns it on).  A negative value only queries; every call returns the old value.
    static const struct {
        int key, *var, max;
    } kKeys[] = {{1, &g_oz_res_nt, 2},  {2, &g_bxb_nt, 1},     {3, &g_sp_nt, 3},
                 {6, &g_nid_kmax, 64},  {7, &g_lam_xu, 3},     {8, &g_nid_sync, 2},
                 {9, &g_shard_proto, 1}, {10, &g_nid_mixed, 1}, {11, &g_nid_poll, 1},
                 {12, &g_rs_xcd, 1},    {13, &g_lam_wave, 1},  {15, &g_lam_lend, 1},
                 {17, &g_nid_fold, 2},  {20, &g_bsolve_ll, 1}, {21, &g_chains_packed, 1},
                 {24, &g_nid_b32, 2},   {25, &g_chains_wide, 1}, {26, &g_fused_alpha, 1},
                 {27, &g_fused_tri_alpha, 1}, {29, &g_nid_resid, 8}};
    for (const auto &k : kKeys)
        if (k.key == key) {
            const int old = *k.var;
            if (value >= 0) *k.var = std::min(value, k.max);
            return old;
        }
    if (key == 4) {  // a mask of four bits
        const int old = g_lam_occ;
        if (value >= 0) g_lam_occ = value & 15;
        return old;
    }
    if (key == 5) {  // a lane count the kernel has an instance of (anything else queries)
        const int old = g_lam_lanes;
        if (value == 0 || value == 4 || value == 8 || value == 16 || value == 32 || value == 64)
            g_lam_lanes = value;
        return old;
    }
    if (key == 16) {  // forced Chebyshev iterate count (benchmarking only; bb_nid.hip)
        const int old = g_nid_force_k;
        if (value >= 0) nid_set_force_k(std::min(value, 64));
        return old;
    }
    return -1;
}
void bb_set_trace_budget(long long bytes) {
    g_trace_budget = bytes > 0 ? (size_t)bytes : (size_t(1) << 30);
}
void bb_debug_interrupt_after(int polls) { g_debug_interrupt = polls; }
int bb_last_call_info(int *devices, int *trace_capacity, int *interrupted) {
    if (devices) *devices = g_last_devices;
    if (trace_capacity) *trace_capacity = g_last_capacity;
    if (interrupted) *interrupted = g_last_interrupted;
    return 0;
}

void bridge_reg_stable(double *betap, double *lambdap, double *sig2p, double *taup,
                       double *alphap, const double *yp, const double *Xp,
                       const double *sig2_shape, const double *sig2_scale,
                       const double *nu_shape, const double *nu_rate, const double *alpha_a,
                       const double *alpha_b, const double *true_sig2, const double *true_tau,
                       const double *true_alpha, const int *P, const int *N, const int *M,
                       const int *burn, double *runtime, const int *ortho) {
    const bb_config c = stable_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a,
                                           alpha_b, true_sig2, true_tau, true_alpha, *P, *N, *M,
                                           ortho);
    if (dense_call(stable_kind(*burn), c, yp, Xp, *burn, {betap, lambdap, sig2p, taup, alphap},
                   runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

void bridge_reg_stable_chains(double *betap, double *lambdap, double *sig2p, double *taup,
                              double *alphap, const double *yp, const double *Xp,
                              const double *sig2_shape, const double *sig2_scale,
                              const double *nu_shape, const double *nu_rate,
                              const double *alpha_a, const double *alpha_b,
                              const double *true_sig2, const double *true_tau,
                              const double *true_alpha, const int *P, const int *N,
                              const int *M, const int *burn, double *runtime,
                              const int *ortho, const int *nchains) {
    if (!nchains_ok("bridge_reg_stable_chains", *nchains)) return;
    const bb_config c = stable_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a,
                                           alpha_b, true_sig2, true_tau, true_alpha, *P, *N, *M,
                                           ortho, *nchains);
    if (chains_call(stable_kind(*burn), c, *nchains, yp, Xp, *burn,
                    {betap, lambdap, sig2p, taup, alphap}, runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

// the body of bridge_reg_stable_chains_summary and, with q, of its _q form
static void stable_chains_summary(const char *entry, const QuantOut *q, double *meanp,
                                  double *varp, double *acovp, double *hmeanp, double *hvarp,
                                  int *flagsp, const int *maxlag, const double *yp,
                                  const double *Xp, const double *sig2_shape,
                                  const double *sig2_scale, const double *nu_shape,
                                  const double *nu_rate, const double *alpha_a,
                                  const double *alpha_b, const double *true_sig2,
                                  const double *true_tau, const double *true_alpha, const int *P,
                                  const int *N, const int *M, const int *burn, double *runtime,
                                  const int *ortho, const int *nchains) {
    if (!nchains_ok(entry, *nchains) || !summary_args_ok(entry, *M, *maxlag) ||
        !quant_args_ok(entry, q, *nchains, *M))
        return;
    const bb_config c = stable_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a,
                                           alpha_b, true_sig2, true_tau, true_alpha, *P, *N, *M,
                                           ortho, *nchains);
    if (chains_summary_call(entry, stable_kind(*burn), c, *nchains, yp, Xp, *burn,
                            {meanp, varp, acovp, hmeanp, hvarp, flagsp, *maxlag, q},
                            runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

void bridge_reg_stable_chains_summary(double *meanp, double *varp, double *acovp, double *hmeanp,
                                      double *hvarp, int *flagsp, const int *maxlag,
                                      const double *yp, const double *Xp,
                                      const double *sig2_shape, const double *sig2_scale,
                                      const double *nu_shape, const double *nu_rate,
                                      const double *alpha_a, const double *alpha_b,
                                      const double *true_sig2, const double *true_tau,
                                      const double *true_alpha, const int *P, const int *N,
                                      const int *M, const int *burn, double *runtime,
                                      const int *ortho, const int *nchains) {
    stable_chains_summary("bridge_reg_stable_chains_summary", nullptr, meanp, varp, acovp, hmeanp,
                          hvarp, flagsp, maxlag, yp, Xp, sig2_shape, sig2_scale, nu_shape,
                          nu_rate, alpha_a, alpha_b, true_sig2, true_tau, true_alpha, P, N, M,
                          burn, runtime, ortho, nchains);
}

void bridge_reg_stable_chains_summary_q(
    double *meanp, double *varp, double *acovp, double *hmeanp, double *hvarp, int *flagsp,
    const int *maxlag, const double *yp, const double *Xp, const double *sig2_shape,
    const double *sig2_scale, const double *nu_shape, const double *nu_rate,
    const double *alpha_a, const double *alpha_b, const double *true_sig2,
    const double *true_tau, const double *true_alpha, const int *P, const int *N, const int *M,
    const int *burn, double *runtime, const int *ortho, const int *nchains, const double *probs,
    const int *nprobs, double *centrep, double *zlop, double *zhip, double *belowp,
    double *inbinp, double *countsp) {
    const QuantOut q{probs, *nprobs, centrep, zlop, zhip, belowp, inbinp, countsp};
    stable_chains_summary("bridge_reg_stable_chains_summary_q", &q, meanp, varp, acovp, hmeanp,
                          hvarp, flagsp, maxlag, yp, Xp, sig2_shape, sig2_scale, nu_shape,
                          nu_rate, alpha_a, alpha_b, true_sig2, true_tau, true_alpha, P, N, M,
                          burn, runtime, ortho, nchains);
}

void bridge_reg_stable_csc(double *betap, double *lambdap, double *sig2p, double *taup,
                           double *alphap, const double *yp, const int *Xcolptr,
                           const int *Xrowidx, const double *Xval, const double *sig2_shape,
                           const double *sig2_scale, const double *nu_shape,
                           const double *nu_rate, const double *alpha_a, const double *alpha_b,
                           const double *true_sig2, const double *true_tau,
                           const double *true_alpha, const int *P, const int *N, const int *M,
                           const int *burn, double *runtime, const int *ortho) {
    const bb_config c = stable_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a,
                                           alpha_b, true_sig2, true_tau, true_alpha, *P, *N, *M,
                                           ortho);
    if (stable_csc(c, yp, Xcolptr, Xrowidx, Xval, *burn, {betap, lambdap, sig2p, taup, alphap},
                   runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

void bridge_reg_logit(double *betap, double *lambdap, double *taup, double *alphap,
                      const double *yp, const double *Xp, const double *nu_shape,
                      const double *nu_rate, const double *alpha_a, const double *alpha_b,
                      const double *true_tau, const double *true_alpha, const int *P,
                      const int *N, const int *M, const int *burn, double *runtime) {
    const double zero = 0.0, one = 1.0;
    const int no = 0;
    const bb_config c = stable_call_config(&zero, &zero, nu_shape, nu_rate, alpha_a, alpha_b,
                                           &one, true_tau, true_alpha, *P, *N, *M, &no);
    if (logit_call(c, yp, Xp, *burn, {betap, lambdap, nullptr, taup, alphap}, runtime) ==
        OUT_INTERRUPTED)
        reraise_interrupt();
}

void bridge_reg_logit_chains(double *betap, double *lambdap, double *taup, double *alphap,
                             const double *yp, const double *Xp, const double *nu_shape,
                             const double *nu_rate, const double *alpha_a,
                             const double *alpha_b, const double *true_tau,
                             const double *true_alpha, const int *P, const int *N, const int *M,
                             const int *burn, double *runtime, const int *nchains) {
    const char *entry = "bridge_reg_logit_chains";
    if (!nchains_ok(entry, *nchains) || !logit_y_ok(entry, yp, *N)) return;
    const bb_config c = logit_chains_config(nu_shape, nu_rate, alpha_a, alpha_b, true_tau,
                                            true_alpha, *P, *N, *M, *nchains);
    // the sig2 trace (the constant 1) has no output: it lands in a buffer of the call's own
    std::vector<double> sig2((size_t)c.trace_capacity * (size_t)*nchains);
    if (chains_call(logit_kind(*burn), c, *nchains, yp, Xp, *burn,
                    {betap, lambdap, sig2.data(), taup, alphap}, runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

// the body of bridge_reg_logit_chains_summary and, with q, of its _q form
static void logit_chains_summary(const char *entry, const QuantOut *q, double *meanp, double *varp,
                                 double *acovp, double *hmeanp, double *hvarp, int *flagsp,
                                 const int *maxlag, const double *yp, const double *Xp,
                                 const double *nu_shape, const double *nu_rate,
                                 const double *alpha_a, const double *alpha_b,
                                 const double *true_tau, const double *true_alpha, const int *P,
                                 const int *N, const int *M, const int *burn, double *runtime,
                                 const int *nchains) {
    if (!nchains_ok(entry, *nchains) || !summary_args_ok(entry, *M, *maxlag) ||
        !quant_args_ok(entry, q, *nchains, *M) || !logit_y_ok(entry, yp, *N))
        return;
    const bb_config c = logit_chains_config(nu_shape, nu_rate, alpha_a, alpha_b, true_tau,
                                            true_alpha, *P, *N, *M, *nchains);
    if (chains_summary_call(entry, logit_kind(*burn), c, *nchains, yp, Xp, *burn,
                            {meanp, varp, acovp, hmeanp, hvarp, flagsp, *maxlag, q},
                            runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

void bridge_reg_logit_chains_summary(double *meanp, double *varp, double *acovp, double *hmeanp,
                                     double *hvarp, int *flagsp, const int *maxlag,
                                     const double *yp, const double *Xp, const double *nu_shape,
                                     const double *nu_rate, const double *alpha_a,
                                     const double *alpha_b, const double *true_tau,
                                     const double *true_alpha, const int *P, const int *N,
                                     const int *M, const int *burn, double *runtime,
                                     const int *nchains) {
    logit_chains_summary("bridge_reg_logit_chains_summary", nullptr, meanp, varp, acovp, hmeanp,
                         hvarp, flagsp, maxlag, yp, Xp, nu_shape, nu_rate, alpha_a, alpha_b,
                         true_tau, true_alpha, P, N, M, burn, runtime, nchains);
}

void bridge_reg_logit_chains_summary_q(
    double *meanp, double *varp, double *acovp, double *hmeanp, double *hvarp, int *flagsp,
    const int *maxlag, const double *yp, const double *Xp, const double *nu_shape,
    const double *nu_rate, const double *alpha_a, const double *alpha_b, const double *true_tau,
    const double *true_alpha, const int *P, const int *N, const int *M, const int *burn,
    double *runtime, const int *nchains, const double *probs, const int *nprobs, double *centrep,
    double *zlop, double *zhip, double *belowp, double *inbinp, double *countsp) {
    const QuantOut q{probs, *nprobs, centrep, zlop, zhip, belowp, inbinp, countsp};
    logit_chains_summary("bridge_reg_logit_chains_summary_q", &q, meanp, varp, acovp, hmeanp,
                         hvarp, flagsp, maxlag, yp, Xp, nu_shape, nu_rate, alpha_a, alpha_b,
                         true_tau, true_alpha, P, N, M, burn, runtime, nchains);
}

void bridge_regression(double *betap, double *up, double *omegap, double *shapep,
                       double *sig2p, double *taup, double *alphap, const double *yp,
                       const double *Xp, const double *sig2_shape, const double *sig2_scale,
                       const double *nu_shape, const double *nu_rate, const double *alpha_a,
                       const double *alpha_b, const double *true_sig2, const double *true_tau,
                       const double *true_alpha, const int *P, const int *N, const int *M,
                       const int *burn, double *runtime, const int *ortho,
                       const int *betaburn, const int *use_hmc) {
    (void)use_hmc;  // BridgeRegression.cpp:418 forces use_hmc = false
    const bb_config c = tri_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a,
                                        alpha_b, true_sig2, true_tau, true_alpha, *P, *N, *M,
                                        ortho, betaburn);
    if (dense_call(tri_kind(*burn), c, yp, Xp, *burn,
                   {betap, omegap, sig2p, taup, alphap, up, shapep}, runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

void bridge_regression_chains(double *betap, double *up, double *omegap, double *shapep,
                              double *sig2p, double *taup, double *alphap, const double *yp,
                              const double *Xp, const double *sig2_shape,
                              const double *sig2_scale, const double *nu_shape,
                              const double *nu_rate, const double *alpha_a,
                              const double *alpha_b, const double *true_sig2,
                              const double *true_tau, const double *true_alpha, const int *P,
                              const int *N, const int *M, const int *burn, double *runtime,
                              const int *ortho, const int *betaburn, const int *use_hmc,
                              const int *nchains) {
    (void)use_hmc;
    if (!nchains_ok("bridge_regression_chains", *nchains)) return;
    const bb_config c = tri_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a,
                                        alpha_b, true_sig2, true_tau, true_alpha, *P, *N, *M,
                                        ortho, betaburn, *nchains);
    if (chains_call(tri_kind(*burn), c, *nchains, yp, Xp, *burn,
                    {betap, omegap, sig2p, taup, alphap, up, shapep}, runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

// the body of bridge_regression_chains_summary and, with q, of its _q form
static void tri_chains_summary(const char *entry, const QuantOut *q, double *meanp, double *varp,
                               double *acovp, double *hmeanp, double *hvarp, int *flagsp,
                               const int *maxlag, const double *yp, const double *Xp,
                               const double *sig2_shape, const double *sig2_scale,
                               const double *nu_shape, const double *nu_rate,
                               const double *alpha_a, const double *alpha_b,
                               const double *true_sig2, const double *true_tau,
                               const double *true_alpha, const int *P, const int *N, const int *M,
                               const int *burn, double *runtime, const int *ortho,
                               const int *betaburn, const int *nchains) {
    if (!nchains_ok(entry, *nchains) || !summary_args_ok(entry, *M, *maxlag) ||
        !quant_args_ok(entry, q, *nchains, *M))
        return;
    const bb_config c = tri_call_config(sig2_shape, sig2_scale, nu_shape, nu_rate, alpha_a,
                                        alpha_b, true_sig2, true_tau, true_alpha, *P, *N, *M,
                                        ortho, betaburn, *nchains);
    if (chains_summary_call(entry, tri_kind(*burn), c, *nchains, yp, Xp, *burn,
                            {meanp, varp, acovp, hmeanp, hvarp, flagsp, *maxlag, q},
                            runtime) == OUT_INTERRUPTED)
        reraise_interrupt();
}

void bridge_regression_chains_summary(double *meanp, double *varp, double *acovp, double *hmeanp,
                                      double *hvarp, int *flagsp, const int *maxlag,
                                      const double *yp, const double *Xp,
                                      const double *sig2_shape, const double *sig2_scale,
                                      const double *nu_shape, const double *nu_rate,
                                      const double *alpha_a, const double *alpha_b,
                                      const double *true_sig2, const double *true_tau,
                                      const double *true_alpha, const int *P, const int *N,
                                      const int *M, const int *burn, double *runtime,
                                      const int *ortho, const int *betaburn, const int *use_hmc,
                                      const int *nchains) {
    (void)use_hmc;
    tri_chains_summary("bridge_regression_chains_summary", nullptr, meanp, varp, acovp, hmeanp,
                       hvarp, flagsp, maxlag, yp, Xp, sig2_shape, sig2_scale, nu_shape, nu_rate,
                       alpha_a, alpha_b, true_sig2, true_tau, true_alpha, P, N, M, burn, runtime,
                       ortho, betaburn, nchains);
}

void bridge_regression_chains_summary_q(
    double *meanp, double *varp, double *acovp, double *hmeanp, double *hvarp, int *flagsp,
    const int *maxlag, const double *yp, const double *Xp, const double *sig2_shape,
    const double *sig2_scale, const double *nu_shape, const double *nu_rate,
    const double *alpha_a, const double *alpha_b, const double *true_sig2,
    const double *true_tau, const double *true_alpha, const int *P, const int *N, const int *M,
    const int *burn, double *runtime, const int *ortho, const int *betaburn, const int *use_hmc,
    const int *nchains, const double *probs, const int *nprobs, double *centrep, double *zlop,
    double *zhip, double *belowp, double *inbinp, double *countsp) {
    (void)use_hmc;
    const QuantOut q{probs, *nprobs, centrep, zlop, zhip, belowp, inbinp, countsp};
    tri_chains_summary("bridge_regression_chains_summary_q", &q, meanp, varp, acovp, hmeanp,
                       hvarp, flagsp, maxlag, yp, Xp, sig2_shape, sig2_scale, nu_shape, nu_rate,
                       alpha_a, alpha_b, true_sig2, true_tau, true_alpha, P, N, M, burn, runtime,
                       ortho, betaburn, nchains);
}

}  // extern "C"
