// bb_host.h -- what the host translation units (bb_engine.cpp, bb_prims.cpp) share: the
// last-error string, HIP / RCCL error checks, the guard every C ABI function runs under, device
// allocation and a call's scoped scratch, the .C call key and the sparse design.  Internal to
// the library: everything here has hidden visibility, so nothing becomes a dynamic export.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "bb_kernels.h"
#include "bb_quantile.h"
#include "bb_sparse.h"

#pragma GCC visibility push(hidden)
namespace bb {

// defined in bb_engine.cpp
extern thread_local std::string g_last_error;
extern int g_device;
extern int g_verbose;
// Key for one .C call: from R's RNG if present, else (seed, stream++).  A call that runs
// `count` chains takes the streams k1 .. k1 + count - 1 (one seed drawn under R's RNG).
void next_call_key(uint64_t *k0, uint64_t *k1, int count = 1);

inline void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIPCHECK(x)                                                                       \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            char b_[512];                                                                 \
            snprintf(b_, sizeof(b_), "HIP error %s at %s:%d: %s", hipGetErrorName(e_),    \
                     __FILE__, __LINE__, #x);                                             \
            throw HipError(b_);                                                           \
        }                                                                                 \
    } while (0)

#define NCCLCHECK(x)                                                                      \
    do {                                                                                  \
        ncclResult_t r_ = (x);                                                            \
        if (r_ != ncclSuccess) {                                                          \
            char b_[512];                                                                 \
            snprintf(b_, sizeof(b_), "RCCL error %s at %s:%d", ncclGetErrorString(r_),    \
                     __FILE__, __LINE__);                                                 \
            throw HipError(b_);                                                           \
        }                                                                                 \
    } while (0)

// The guard of the C ABI: runs f and turns an exception into bb_last_error() and -1.  f
// returns nothing (the call then returns 0) or the call's own code (-2 "rejection cap" and
// friends, having set the error text itself).
template <class F>
int guarded(F &&f) {
    try {
        if constexpr (std::is_void_v<decltype(f())>) {
            f();
            return 0;
        } else {
            return f();
        }
    } catch (std::exception &ex) {
        set_error("%s", ex.what());
        return -1;
    }
}
// ... with `device` made current first
template <class F>
int guarded(int device, F &&f) {
    return guarded([&] {
        HIPCHECK(hipSetDevice(device));
        return f();
    });
}

inline int round_up(int x, int m) { return ((x + m - 1) / m) * m; }

template <typename T>
T *dalloc(size_t count, std::vector<void *> &owned) {
    void *p = nullptr;
    if (count == 0) count = 1;
    HIPCHECK(hipMalloc(&p, count * sizeof(T)));
    HIPCHECK(hipMemset(p, 0, count * sizeof(T)));
    // the engine's streams are non-blocking: the zero fill must land before their first use
    HIPCHECK(hipDeviceSynchronize());
    owned.push_back(p);
    return (T *)p;
}

// The device allocations and events of one kernel-level call, released on every way out.
struct Scratch {
    std::vector<void *> owned;
    std::vector<hipEvent_t> events;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (void *q : owned) (void)hipFree(q);
    }
    template <typename T>
    T *alloc(size_t count) {
        return dalloc<T>(count, owned);
    }
    hipEvent_t event() {
        hipEvent_t e;
        HIPCHECK(hipEventCreate(&e));
        events.push_back(e);
        return e;
    }
};

// f(k, slot, run) for each contiguous run of the slots [slot0, slot0 + count) in a ring of
// `cap`: slots slot .. slot + run - 1 hold the samples k .. k + run - 1 of the request
template <class F>
void ring_runs(int slot0, int count, int cap, F f) {
    for (int k = 0; k < count;) {
        const int slot = (slot0 + k) % cap;
        const int run = std::min(count - k, cap - slot);
        f(k, slot, run);
        k += run;
    }
}

// Posterior summaries of K chains' trace rings, accumulated on the device (bb_summary.hip;
// the records and their layout: bb_kernels.h): reset(), then the M samples in order through
// add() as the rings fill, then get().  Everything is enqueued on the caller's stream, behind
// the sweeps that wrote the slots; the current device is the caller's.
struct TraceSummary {
    int K = 0, Q = 0, M = 0, L = 0;
    int next = 0;  // samples added so far
    double *acc = nullptr, *out = nullptr;
    size_t acc_count = 0, out_count = 0;
    TraceSummary() = default;
    TraceSummary(const TraceSummary &) = delete;
    TraceSummary &operator=(const TraceSummary &) = delete;
    ~TraceSummary() {
        (void)hipFree(acc);
        (void)hipFree(out);
    }
    // doubles of the outputs per (chain, parameter): mean, var, acov[0..L], hmean[2], hvar[2]
    static size_t out_per_record(int L) { return (size_t)(L + 1) + 6; }
    // why (nsamp, maxlag) cannot be summarised, or nullptr
    static const char *refusal(int nsamp, int maxlag) {
        if (maxlag < 0) return "maxlag must be at least 0";
        if (maxlag > kSummaryMaxLag) return "maxlag must be at most 63 (a lag per lane of a wave)";
        if (nsamp < 1) return "the number of samples must be at least 1";
        return nullptr;
    }
    // sized for K chains of Q parameters, M samples and lags 0..L, and zeroed
    void reset(hipStream_t s, int K_, int Q_, int M_, int L_) {
        if (const char *why = refusal(M_, L_)) throw HipError(std::string("summary: ") + why);
        if (K_ < 1 || Q_ < 1) throw HipError("summary: no chains or no parameters");
        const size_t na = (size_t)K_ * Q_ * kSummaryStride;
        const size_t no = (size_t)K_ * Q_ * out_per_record(L_);
        auto fit = [&](double *&q, size_t &have, size_t need) {
            if (have == need) return;
            HIPCHECK(hipStreamSynchronize(s));
            (void)hipFree(q);
            q = nullptr;
            have = 0;
            HIPCHECK(hipMalloc((void **)&q, need * sizeof(double)));
            have = need;
        };
        fit(acc, acc_count, na);
        fit(out, out_count, no);
        K = K_, Q = Q_, M = M_, L = L_, next = 0;
        HIPCHECK(hipMemsetAsync(acc, 0, na * sizeof(double), s));
    }
    // ring slots [slot0, slot0 + count) (wrapping at ring.cap) are the samples [s0, s0 + count)
    void add(hipStream_t s, const SummaryRing &ring, int slot0, int count, int s0) {
        if (!acc) throw HipError("summary: add before reset");
        if (ring.params() != Q) throw HipError("summary: the rings hold another parameter count");
        if (slot0 < 0 || count < 0) throw HipError("summary: slot0 and count must be >= 0");
        if (s0 != next || count > M - next) {
            char b[160];
            snprintf(b, sizeof(b), "summary: samples are added in order (next %d of %d; got %d "
                     "from %d)", next, M, count, s0);
            throw HipError(b);
        }
        ring_runs(slot0, count, ring.cap, [&](int k, int slot, int run) {
            launch_trace_summary(s, ring, K, slot, run, s0 + k, M, L, acc);
        });
        HIPCHECK(hipGetLastError());
        next += count;
    }
    // The outputs to the host once all M samples are in, chain-major: mean, var [K][Q], acov
    // [K][Q][L + 1], hmean, hvar [K][Q][2].  Waits for the stream.
    void get(hipStream_t s, double *mean, double *var, double *acov, double *hmean,
             double *hvar) {
        if (!acc || next != M) {
            char b[128];
            snprintf(b, sizeof(b), "summary: %d of %d samples added", acc ? next : 0, M);
            throw HipError(b);
        }
        const size_t kq = (size_t)K * Q;
        double *dm = out, *dv = dm + kq, *da = dv + kq, *dhm = da + kq * (L + 1),
               *dhv = dhm + 2 * kq;
        launch_summary_finalise(s, acc, K, Q, M, L, dm, dv, da, dhm, dhv);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(s));
        auto fetch = [&](double *dst, const double *src, size_t n) {
            if (dst) HIPCHECK(hipMemcpy(dst, src, n * sizeof(double), hipMemcpyDeviceToHost));
        };
        fetch(mean, dm, kq);
        fetch(var, dv, kq);
        fetch(acov, da, kq * (L + 1));
        fetch(hmean, dhm, 2 * kq);
        fetch(hvar, dhv, 2 * kq);
    }
};

// The pooled order-statistic sketch of K chains' trace rings (bb_quantile.hip; the bins:
// bb_quantile.h): reset(), then every chain's M samples through add() as the rings fill -- all
// chains of a batch at once, or one chain after another through single-chain rings -- then
// get() for any probabilities.  One histogram and three counters per parameter, pooled over
// the chains; the centre is the first sample of the first add().  Enqueued on the caller's
// stream like TraceSummary; integer counts, so the order of the adds changes nothing.
struct TraceQuantiles {
    int K = 0, Q = 0, M = 0;
    int device = 0;                // the device current at reset(): where the sketch lives
    unsigned long long added = 0;  // samples added so far, over all chains
    bool centred = false;
    unsigned int *hist = nullptr;  // [Q][kQuantBins], then the counters [Q][kQuantCounters]
    double *centre = nullptr;      // [Q]
    size_t hist_count = 0, centre_count = 0;
    TraceQuantiles() = default;
    TraceQuantiles(const TraceQuantiles &) = delete;
    TraceQuantiles &operator=(const TraceQuantiles &) = delete;
    ~TraceQuantiles() {
        (void)hipFree(hist);
        (void)hipFree(centre);
    }
    unsigned int *counters() const { return hist + (size_t)Q * kQuantBins; }
    // why K chains of nsamp samples cannot be pooled, or nullptr (the counts are 32-bit)
    static const char *refusal(int nchains, int nsamp) {
        if (nchains < 1 || nsamp < 1) return "no chains or no samples";
        if ((unsigned long long)nchains * (unsigned long long)nsamp >= (1ull << 32))
            return "nchains x nsamp must be below 2^32 (the sketch counts in 32 bits)";
        return nullptr;
    }
    // why these probabilities cannot be selected, or nullptr
    static const char *probs_refusal(const double *probs, int nprobs) {
        if (nprobs < 1) return "at least one probability is needed";
        if (nprobs > kQuantMaxProbs) return "at most 64 probabilities per call";
        for (int j = 0; j < nprobs; ++j)
            if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return "every probability must be in [0, 1]";
        return nullptr;
    }
    bool ready() const { return hist != nullptr && K > 0; }
    // sized for K chains of Q parameters and M samples each, and zeroed
    void reset(hipStream_t s, int K_, int Q_, int M_) {
        if (const char *why = refusal(K_, M_)) throw HipError(std::string("quantiles: ") + why);
        if (Q_ < 1) throw HipError("quantiles: no parameters");
        const size_t nh = (size_t)Q_ * (kQuantBins + kQuantCounters);
        if (hist_count != nh || centre_count != (size_t)Q_) {
            HIPCHECK(hipStreamSynchronize(s));
            (void)hipFree(hist);
            (void)hipFree(centre);
            hist = nullptr, centre = nullptr, hist_count = centre_count = 0;
            HIPCHECK(hipMalloc((void **)&hist, nh * sizeof(unsigned int)));
            hist_count = nh;
            HIPCHECK(hipMalloc((void **)&centre, (size_t)Q_ * sizeof(double)));
            centre_count = (size_t)Q_;
        }
        K = K_, Q = Q_, M = M_, added = 0, centred = false;
        HIPCHECK(hipGetDevice(&device));
        HIPCHECK(hipMemsetAsync(hist, 0, nh * sizeof(unsigned int), s));
        HIPCHECK(hipMemsetAsync(centre, 0, (size_t)Q_ * sizeof(double), s));
    }
    // ring slots [slot0, slot0 + count) (wrapping at ring.cap) of each of the ring's `chains`
    // chains; the very first add starts at a chain's sample 0 and fixes the centre
    void add(hipStream_t s, const SummaryRing &ring, int chains, int slot0, int count, int s0) {
        if (!ready()) throw HipError("quantiles: add before reset");
        if (ring.params() != Q) throw HipError("quantiles: the rings hold another parameter count");
        if (slot0 < 0 || count < 0 || chains < 1)
            throw HipError("quantiles: slot0 and count must be >= 0");
        const unsigned long long total = (unsigned long long)K * M;
        if ((unsigned long long)chains * count > total - added)
            throw HipError("quantiles: more samples than the sketch was sized for");
        if (count == 0) return;
        if (!centred) {
            if (s0 != 0) throw HipError("quantiles: the first samples added must start at 0");
            launch_quantile_centre(s, ring, slot0 % ring.cap, centre);
            centred = true;
        }
        ring_runs(slot0, count, ring.cap, [&](int, int slot, int run) {
            launch_trace_hist(s, ring, chains, slot, run, centre, hist, counters());
        });
        HIPCHECK(hipGetLastError());
        added += (unsigned long long)chains * count;
    }
    // The selection once every sample is in: centre [Q], zlo, zhi, below, inbin [Q][nprobs],
    // counts [Q][6] (any may be null).  Waits for the stream.
    void get(hipStream_t s, const double *probs, int nprobs, double *centre_out, double *zlo,
             double *zhi, double *below, double *inbin, double *counts) {
        const unsigned long long total = (unsigned long long)K * M;
        if (!ready() || added != total) {
            char b[128];
            snprintf(b, sizeof(b), "quantiles: %llu of %llu samples added", ready() ? added : 0ull,
                     ready() ? total : 0ull);
            throw HipError(b);
        }
        if (const char *why = probs_refusal(probs, nprobs))
            throw HipError(std::string("quantiles: ") + why);
        Scratch dev;
        const size_t qn = (size_t)Q * nprobs;
        double *dp = dev.alloc<double>(nprobs), *out = dev.alloc<double>(4 * qn + 6 * (size_t)Q);
        HIPCHECK(hipMemcpyAsync(dp, probs, (size_t)nprobs * sizeof(double), hipMemcpyHostToDevice,
                                s));
        launch_quantile_select(s, hist, counters(), Q, total, dp, nprobs, out, out + qn,
                               out + 2 * qn, out + 3 * qn, out + 4 * qn);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(s));
        auto fetch = [&](double *dst, const double *src, size_t n) {
            if (dst) HIPCHECK(hipMemcpy(dst, src, n * sizeof(double), hipMemcpyDeviceToHost));
        };
        fetch(centre_out, centre, (size_t)Q);
        fetch(zlo, out, qn);
        fetch(zhi, out + qn, qn);
        fetch(below, out + 2 * qn, qn);
        fetch(inbin, out + 3 * qn, qn);
        fetch(counts, out + 4 * qn, 6 * (size_t)Q);
    }
};

// ---------------------------------------------------------------------------
// Sparse design (CSC input): CSC + CSR copies on the device and the Gram pair list
// (bb_sparse.h).  Built once at setup; X is constant over a chain.
// ---------------------------------------------------------------------------
// The canonical dgCMatrix form every CSC entry point requires (colptr[0] = 0,
// non-decreasing, rows in [0, n), strictly increasing within a column); throws otherwise.
// Both .C CSC paths (sparse engine and densified dense path) run it, so a malformed matrix
// is refused the same way whichever path its shape selects.
inline void csc_validate(int n, int p, const int *cp, const int *ri) {
    if (cp[0] != 0) throw HipError("CSC: colptr[0] must be 0");
    for (int j = 0; j < p; ++j) {
        if (cp[j + 1] < cp[j]) throw HipError("CSC: colptr must be non-decreasing");
        for (int q = cp[j]; q < cp[j + 1]; ++q) {
            if (ri[q] < 0 || ri[q] >= n) throw HipError("CSC: row index out of range");
            if (q > cp[j] && ri[q] <= ri[q - 1])
                throw HipError("CSC: row indices must be strictly increasing within a "
                               "column (canonical dgCMatrix form)");
        }
    }
}

struct SparseDesign {
    int n = 0, n_pad = 0, p = 0;
    long nnz = 0;
    size_t pairs = 0;
    int *colptr = nullptr, *rowidx = nullptr, *rowptr = nullptr, *colidx = nullptr,
        *cpos = nullptr, *pj = nullptr;
    double *cval = nullptr, *rval = nullptr, *prod = nullptr;
    unsigned *estart = nullptr;
    unsigned short *pidx = nullptr;
    int max_row = 0;        // largest row nnz
    bool col_mode = false;  // by-column Gram kernel (max_row <= kSpColMaxRow)

    // Validates the CSC (colptr[0] = 0, non-decreasing, rows in [0, n), strictly increasing
    // within a column -- R's dgCMatrix is in this canonical form), transposes it on the host
    // into a CSR with each entry's CSC position, uploads both and builds the pair list.
    void build(hipStream_t s, int n_, int n_pad_, int p_, const int *cp, const int *ri,
               const double *cv, std::vector<void *> &owned) {
        n = n_;
        n_pad = n_pad_;
        p = p_;
        csc_validate(n, p, cp, ri);
        nnz = cp[p];
        std::vector<int> rp(n_pad + 1, 0), ci(nnz > 0 ? nnz : 1), pos(nnz > 0 ? nnz : 1);
        std::vector<double> rv(nnz > 0 ? nnz : 1);
        for (long q = 0; q < nnz; ++q) ++rp[ri[q] + 1];
        max_row = 0;
        for (int r = 0; r < n_pad; ++r) max_row = std::max(max_row, rp[r + 1]);
        col_mode = max_row <= kSpColMaxRow;
        for (int r = 0; r < n_pad; ++r) rp[r + 1] += rp[r];
        std::vector<int> next(rp.begin(), rp.end() - 1);
        for (int j = 0; j < p; ++j)
            for (int q = cp[j]; q < cp[j + 1]; ++q) {
                const int k = next[ri[q]]++;
                ci[k] = j;
                rv[k] = cv[q];
                pos[k] = q;
            }
        colptr = dalloc<int>(p + 1, owned);
        rowidx = dalloc<int>(nnz, owned);
        cval = dalloc<double>(nnz, owned);
        rowptr = dalloc<int>(n_pad + 1, owned);
        colidx = dalloc<int>(nnz, owned);
        rval = dalloc<double>(nnz, owned);
        cpos = dalloc<int>(nnz, owned);
        HIPCHECK(hipMemcpy(colptr, cp, (size_t)(p + 1) * sizeof(int), hipMemcpyHostToDevice));
        if (nnz > 0) {
            HIPCHECK(hipMemcpy(rowidx, ri, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(cval, cv, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(colidx, ci.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(rval, rv.data(), (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(cpos, pos.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
        }
        HIPCHECK(hipMemcpy(rowptr, rp.data(), (size_t)(n_pad + 1) * sizeof(int),
                           hipMemcpyHostToDevice));
        // pair counts per output column, host scan, then the pair list itself
        unsigned long long *dcnt = nullptr, *dbase = nullptr;
        HIPCHECK(hipMalloc(&dcnt, (size_t)n_pad * sizeof(unsigned long long)));
        launch_sp_count(s, rowptr, colidx, cpos, colptr, n_pad, dcnt);
        std::vector<unsigned long long> cnt(n_pad), base(n_pad);
        HIPCHECK(hipMemcpyAsync(cnt.data(), dcnt, cnt.size() * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        (void)hipFree(dcnt);
        unsigned long long tot = 0;
        for (int c = 0; c < n_pad; ++c) {
            base[c] = tot;
            tot += cnt[c];
        }
        if (tot > 0xFFFFFF00ull)
            throw HipError("sparse Gram: more than 2^32 - 1 column pairs (X too dense for the "
                           "pair-list Gram; use the dense entry point)");
        pairs = (size_t)tot;
        size_t fr = 0, total_mem = 0;
        HIPCHECK(hipMemGetInfo(&fr, &total_mem));
        const size_t need = pairs * (sizeof(double) + (col_mode ? 2 : sizeof(int))) +
                            (tri_count(n_pad) + 1) * sizeof(unsigned);
        if (need + (size_t(1) << 28) > fr) {
            char b[256];
            snprintf(b, sizeof(b), "sparse Gram: pair list needs %.2f GB, %.2f GB free", need / 1e9,
                     fr / 1e9);
            throw HipError(b);
        }
        estart = dalloc<unsigned>(tri_count(n_pad) + 1, owned);
        prod = dalloc<double>(pairs, owned);
        if (col_mode)
            pidx = dalloc<unsigned short>(pairs, owned);
        else
            pj = dalloc<int>(pairs, owned);
        HIPCHECK(hipMalloc(&dbase, (size_t)n_pad * sizeof(unsigned long long)));
        HIPCHECK(hipMemcpyAsync(dbase, base.data(), base.size() * sizeof(unsigned long long),
                                hipMemcpyHostToDevice, s));
        launch_sp_build(s, rowptr, colidx, cpos, rval, colptr, rowidx, cval, n_pad, dbase, estart,
                        prod, pj, pidx);
        const unsigned last = (unsigned)tot;
        HIPCHECK(hipMemcpyAsync(estart + tri_count(n_pad), &last, sizeof(unsigned),
                                hipMemcpyHostToDevice, s));
        HIPCHECK(hipStreamSynchronize(s));
        (void)hipFree(dbase);
    }

    // tri (packed upper triangle of X diag(D) X', n_pad wide) and xu = X u
    void gram(hipStream_t s, const double *D, const double *u, double *tri, double *xu,
              const int *gate = nullptr) const {
        if (col_mode) {
            launch_sp_gram_col(s, rowptr, colidx, rval, estart, prod, pidx, D, u, n_pad, max_row,
                               tri, xu, gate);
        } else {
            launch_sp_gram(s, estart, prod, pj, D, n_pad, tri, gate);
            launch_sp_rows(s, rowptr, colidx, rval, n_pad, u, D, xu, tri, gate);
        }
    }
};

}  // namespace bb
#pragma GCC visibility pop
