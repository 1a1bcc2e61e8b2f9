// bb_quantile.hip -- a pooled order-statistic sketch of trace rings, built on the device
// (gfx950): credible intervals and sign probabilities without the traces.
//
// bb_summary.hip's accumulators are running moment sums: no order statistic comes out of them.
// Here every sample of parameter q, of every chain, is counted into one histogram per
// parameter whose bins are a fixed function of the bits of z = x - c_q (bb_quantile.h), c_q the
// first kept draw of chain 0.  The counts are integers, so the histogram is bitwise independent
// of the ring capacity, of the split into launches, of ring wrap, of the grid and of the order
// in which the adds arrive.  k_quantile_select scans a histogram for the bins that hold the
// requested order statistics: each comes back as a bracket [zlo, zhi] at most 2^-8 |z| wide,
// with the counts below and inside the bin.
//
// k_trace_hist has k_trace_summary's shape: workgroup (chain, 8 adjacent parameters), a wave
// per parameter, the ring chunk [slot][p] staged through LDS 64 slots at a time.  The posterior
// mass of a parameter sits in a few thousand bins and all K chains add to them, so a wave
// combines what it can before anything leaves the workgroup:
//   - the zero bin, the overflow bins, the NaN count and the sign counts are wave ballots kept
//     in registers (a constant column -- a known alpha, the logistic sig2 -- puts every sample
//     of every chain in the zero bin);
//   - ordinary bins go to the wave's LDS window, the top kHistWin bins of each sign below the
//     next power of two above the largest |z| of the first staged chunk that has one, flushed
//     at the end with one global add per non-zero bin, adjacent lanes on adjacent bins;
//   - an ordinary sample outside the window is added to global memory directly.
// Where a sample is added changes no count.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "bb_quantile.h"

namespace bb {

namespace {

constexpr int kHistTile = 8;                  // adjacent parameters (waves) of a workgroup
constexpr int kHistChunk = 64;                // ring slots staged per pass: one per lane
constexpr int kHistThreads = 64 * kHistTile;  // a thread per staged value
constexpr int kHistWin = 896;                 // bins per sign of a wave's window: 3.5 octaves
static_assert(sizeof(double) * kHistChunk * (kHistTile + 1) +
                      sizeof(unsigned int) * kHistTile * 2 * kHistWin <= 65536,
              "the staged chunk and the windows share 64 KB of LDS");

constexpr int kSelThreads = 256;
constexpr int kSelSeg = (kQuantBins + kSelThreads - 1) / kSelThreads;  // bins per thread

__device__ __forceinline__ int wave_max_all(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ unsigned int wave_count(bool pred) {
    return (unsigned int)__popcll(__ballot(pred));
}

}  // namespace

__global__ __launch_bounds__(64) void k_quantile_centre(
    const double *__restrict__ rb, const double *__restrict__ rs2, const double *__restrict__ rtau,
    const double *__restrict__ ralpha, int P, int Q, int slot, double *__restrict__ centre) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= Q) return;
    centre[q] = q < P ? rb[(size_t)slot * P + q]
                      : (q == P ? rs2 : q == P + 1 ? rtau : ralpha)[slot];
}

// Workgroup b: chain b / tiles, parameters [q0, q0 + kHistTile) with q0 = (b % tiles) kHistTile,
// wave w the parameter q0 + w (k_trace_summary's staging).
__global__ __launch_bounds__(kHistThreads) void k_trace_hist(
    const double *__restrict__ rb, const double *__restrict__ rs2, const double *__restrict__ rtau,
    const double *__restrict__ ralpha, int P, int Q, int cap, int tiles, int slot, int count,
    const double *__restrict__ centre, unsigned int *__restrict__ hist,
    unsigned int *__restrict__ cnt) {
    __shared__ double tile[kHistChunk][kHistTile + 1];
    __shared__ unsigned int win[kHistTile][2 * kHistWin];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * kHistTile, q = q0 + w;
    const bool live = q < Q;  // wave-uniform
    const size_t ring0 = (size_t)c * cap + slot;
    unsigned int *mywin = win[w];
    for (int i = lane; i < 2 * kHistWin; i += 64) mywin[i] = 0u;
    const double cq = live ? centre[q] : 0.0;
    unsigned int *h = hist + (size_t)(live ? q : 0) * kQuantBins;
    // wave-uniform counts, and the window [rtop - kHistWin, rtop) of each sign (< 0: not set)
    unsigned int n_nan = 0, n_neg = 0, n_pos = 0, n_zero = 0, n_ovn = 0, n_ovp = 0;
    int rtop = -1;
    for (int base = 0; base < count; base += kHistChunk) {
        const int n = min(kHistChunk, count - base);
        __syncthreads();  // the previous chunk is consumed
        {
            const int i = tid / kHistTile, j = tid % kHistTile, qq = q0 + j;
            if (i < n && qq < Q) {
                const size_t sl = ring0 + base + i;
                tile[i][j] = qq < P ? rb[sl * P + qq]
                                    : (qq == P ? rs2 : qq == P + 1 ? rtau : ralpha)[sl];
            }
        }
        __syncthreads();
        if (!live) continue;
        const bool on = lane < n;
        const double xv = on ? tile[lane][w] : 0.0;
        const double z = xv - cq;
        const int bin = on ? quantile_bin(z) : -2;
        n_nan += wave_count(bin == -1);
        n_pos += wave_count(on && xv > 0.0);
        n_neg += wave_count(on && xv < 0.0);
        n_zero += wave_count(bin == kQuantZeroBin);
        n_ovn += wave_count(bin == 0);
        n_ovp += wave_count(bin == kQuantBins - 1);
        const bool ord = bin > 0 && bin < kQuantBins - 1 && bin != kQuantZeroBin;
        const bool pos = bin > kQuantZeroBin;
        const int r = pos ? bin - kQuantZeroBin - 1 : kQuantSignBins - bin;  // of an ordinary bin
        if (rtop < 0) {
            const int rmax = wave_max_all(ord ? r : -1);
            if (rmax >= 0) rtop = max(kHistWin, ((rmax >> 8) + 1) << 8);
        }
        if (ord) {
            const int o = r - (rtop - kHistWin);
            if (o >= 0 && o < kHistWin)
                atomicAdd(&mywin[(pos ? kHistWin : 0) + o], 1u);
            else
                atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();  // the window's adds are in
    if (!live) return;
    if (rtop >= 0) {
        for (int i = lane; i < 2 * kHistWin; i += 64) {
            const unsigned int v = mywin[i];
            if (v == 0u) continue;
            const bool pos = i >= kHistWin;
            const int r = rtop - kHistWin + (pos ? i - kHistWin : i);  // in [0, kQuantSignBins)
            atomicAdd(&h[pos ? kQuantZeroBin + 1 + r : kQuantSignBins - r], v);
        }
    }
    if (lane == 0) {
        unsigned int *k = cnt + (size_t)q * kQuantCounters;
        if (n_nan) atomicAdd(&k[QCNT_NAN], n_nan);
        if (n_neg) atomicAdd(&k[QCNT_NEG], n_neg);
        if (n_pos) atomicAdd(&k[QCNT_POS], n_pos);
        if (n_zero) atomicAdd(&h[kQuantZeroBin], n_zero);
        if (n_ovn) atomicAdd(&h[0], n_ovn);
        if (n_ovp) atomicAdd(&h[kQuantBins - 1], n_ovp);
    }
}

// One workgroup per parameter: thread t sums the bins [t kSelSeg, (t + 1) kSelSeg), the
// segment sums are scanned, and for each probability the thread whose segment holds the rank
// walks it.
__global__ __launch_bounds__(kSelThreads) void k_quantile_select(
    const unsigned int *__restrict__ hist, const unsigned int *__restrict__ cnt,
    unsigned long long total, const double *__restrict__ probs, int nprobs,
    double *__restrict__ zlo, double *__restrict__ zhi, double *__restrict__ below,
    double *__restrict__ inbin, double *__restrict__ counts) {
    __shared__ unsigned long long seg[kSelThreads + 1];
    const int q = blockIdx.x, t = threadIdx.x;
    const unsigned int *h = hist + (size_t)q * kQuantBins;
    const int b0 = t * kSelSeg, b1 = min(kQuantBins, b0 + kSelSeg);
    unsigned long long mine = 0;
    for (int b = b0; b < b1; ++b) mine += h[b];
    seg[t + 1] = mine;
    __syncthreads();
    if (t == 0) {
        seg[0] = 0;
        for (int i = 1; i <= kSelThreads; ++i) seg[i] += seg[i - 1];
    }
    __syncthreads();
    const unsigned long long before = seg[t];
    const unsigned long long nan = cnt[(size_t)q * kQuantCounters + QCNT_NAN];
    const unsigned long long N = total - nan;
    if (t == 0) {
        double *o = counts + (size_t)q * 6;
        o[0] = (double)N;
        o[1] = (double)nan;
        o[2] = (double)cnt[(size_t)q * kQuantCounters + QCNT_NEG];
        o[3] = (double)cnt[(size_t)q * kQuantCounters + QCNT_POS];
        o[4] = (double)h[kQuantZeroBin];
        o[5] = (double)h[0] + (double)h[kQuantBins - 1];
    }
    for (int j = 0; j < nprobs; ++j) {
        const size_t at = (size_t)q * nprobs + j;
        if (N == 0) {
            if (t == 0) {
                const double nn = __builtin_nan("");
                zlo[at] = nn, zhi[at] = nn, below[at] = nn, inbin[at] = nn;
            }
            continue;
        }
        const double want = ceil(probs[j] * (double)N);
        unsigned long long k = want < 1.0 ? 1ull : (unsigned long long)want;
        if (k > N) k = N;
        if (!(before < k && k <= before + mine)) continue;  // one thread holds the rank
        unsigned long long lo = before;
        for (int b = b0; b < b1; ++b) {
            const unsigned int v = h[b];
            if (k <= lo + v) {
                double e0, e1;
                quantile_bin_edges(b, &e0, &e1);
                zlo[at] = e0, zhi[at] = e1, below[at] = (double)lo, inbin[at] = (double)v;
                break;
            }
            lo += v;
        }
    }
}

void launch_quantile_centre(hipStream_t s, const SummaryRing &r, int slot, double *centre) {
    const int Q = r.params();
    if (slot < 0 || slot >= r.cap)
        throw std::invalid_argument("launch_quantile_centre: slot out of range");
    k_quantile_centre<<<(Q + 63) / 64, 64, 0, s>>>(r.beta, r.sig2, r.tau, r.alpha, r.p, Q, slot,
                                                    centre);
}

void launch_trace_hist(hipStream_t s, const SummaryRing &r, int K, int slot, int count,
                       const double *centre, unsigned int *hist, unsigned int *cnt) {
    if (count <= 0 || K <= 0) return;
    const int Q = r.params(), tiles = (Q + kHistTile - 1) / kHistTile;
    if (slot < 0 || slot + count > r.cap || (size_t)K * tiles > 0x7fffffffu)
        throw std::invalid_argument("launch_trace_hist: arguments out of range");
    k_trace_hist<<<K * tiles, kHistThreads, 0, s>>>(r.beta, r.sig2, r.tau, r.alpha, r.p, Q, r.cap,
                                                    tiles, slot, count, centre, hist, cnt);
}

void launch_quantile_select(hipStream_t s, const unsigned int *hist, const unsigned int *cnt,
                            int Q, unsigned long long total, const double *probs, int nprobs,
                            double *zlo, double *zhi, double *below, double *inbin,
                            double *counts) {
    if (Q < 1 || nprobs < 0 || nprobs > kQuantMaxProbs)
        throw std::invalid_argument("launch_quantile_select: arguments out of range");
    k_quantile_select<<<Q, kSelThreads, 0, s>>>(hist, cnt, total, probs, nprobs, zlo, zhi, below,
                                                inbin, counts);
}

}  // namespace bb
