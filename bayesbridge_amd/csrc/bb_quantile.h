// bb_quantile.h -- the bin scheme of the pooled order-statistic sketch (bb_quantile.hip,
// DESIGN.md s6.4), shared by the kernels and the host (bb_quantile_bin), and the launches.
//
// Every sample x of parameter q is binned as z = x - c_q, c_q the first kept draw of chain 0.
// With a the bits of |z|, e = a >> 52 and m = (a >> 44) & 0xff:
//   959 <= e < 1087 (2^-64 <= |z| < 2^64)   ordinary bin r = (e - 959) 256 + m, per sign
//   |z| < 2^-64 (+-0 and subnormals too)     the zero bin
//   |z| >= 2^64 (+-inf too)                  the overflow bin of its sign
//   NaN                                      no bin (counted)
// ordered from the negative overflow bin up: index 0 the negative overflow bin, 32768 - r the
// negative bin r, 32769 the zero bin, 32770 + r the positive bin r, 65538 the positive overflow
// bin.  Positive bin r is [lo, hi) with lo's bits ((r >> 8) + 959) << 52 | (r & 255) << 44 and
// hi's those plus 1 << 44, negative bins mirror it, the zero bin is [-2^-64, 2^-64] and the
// overflow bins run to +-inf: a bin is at most 2^-8 |z| wide.  The key is a fixed function of
// the value's bits and the counts are integers, so a histogram does not depend on the ring
// capacity, the split into launches, ring wrap or the grid.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bb_kernels.h"

namespace bb {

constexpr int kQuantExp0 = 959, kQuantExp1 = 1087;            // ordinary bins: e in [Exp0, Exp1)
constexpr int kQuantSignBins = (kQuantExp1 - kQuantExp0) * 256;  // 32768 per sign
constexpr int kQuantZeroBin = kQuantSignBins + 1;                // 32769
constexpr int kQuantBins = 2 * kQuantSignBins + 3;               // 65539
constexpr int kQuantMaxProbs = 64;
// per-parameter counters beside the histogram
enum { QCNT_NAN = 0, QCNT_NEG, QCNT_POS, kQuantCounters = 4 };

// the bin of z, -1 for NaN
__host__ __device__ inline int quantile_bin(double z) {
    unsigned long long b;
    __builtin_memcpy(&b, &z, sizeof(b));
    const unsigned long long a = b & 0x7fffffffffffffffull;
    const bool neg = (b >> 63) != 0;
    if (a > 0x7ff0000000000000ull) return -1;
    const int e = (int)(a >> 52), m = (int)((a >> 44) & 0xff);
    if (e < kQuantExp0) return kQuantZeroBin;
    if (e >= kQuantExp1) return neg ? 0 : kQuantBins - 1;
    const int r = (e - kQuantExp0) * 256 + m;
    return neg ? kQuantSignBins - r : kQuantZeroBin + 1 + r;
}

// the edges of a bin: every z of the bin has lo <= z <= hi
__host__ __device__ inline void quantile_bin_edges(int bin, double *lo, double *hi) {
    auto from_bits = [](unsigned long long u) {
        double d;
        __builtin_memcpy(&d, &u, sizeof(d));
        return d;
    };
    const double two64 = from_bits((unsigned long long)kQuantExp1 << 52);
    const double tiny = from_bits((unsigned long long)kQuantExp0 << 52);  // 2^-64
    const double inf = from_bits(0x7ff0000000000000ull);
    if (bin <= 0) {
        *lo = -inf, *hi = -two64;
    } else if (bin >= kQuantBins - 1) {
        *lo = two64, *hi = inf;
    } else if (bin == kQuantZeroBin) {
        *lo = -tiny, *hi = tiny;
    } else {
        const bool neg = bin < kQuantZeroBin;
        const unsigned long long r = neg ? kQuantSignBins - bin : bin - kQuantZeroBin - 1;
        const unsigned long long u = ((r >> 8) + kQuantExp0) << 52 | (r & 255) << 44;
        const double a = from_bits(u), b = from_bits(u + (1ull << 44));
        if (neg)
            *lo = -b, *hi = -a;
        else
            *lo = a, *hi = b;
    }
}

// centre[q] = sample at ring slot `slot` of chain 0 (the first kept draw)
void launch_quantile_centre(hipStream_t s, const SummaryRing &r, int slot, double *centre);
// Adds ring slots [slot, slot + count) (no wrap) of each of K chains to hist ([Q][kQuantBins])
// and cnt ([Q][kQuantCounters]), binned about centre ([Q]).
void launch_trace_hist(hipStream_t s, const SummaryRing &r, int K, int slot, int count,
                       const double *centre, unsigned int *hist, unsigned int *cnt);
// For parameter q and probability probs[j] (nprobs <= kQuantMaxProbs), with N = total - NaNs
// and k = min(N, max(1, ceil(probs[j] N))): the edges zlo, zhi of the bin holding the k-th
// smallest z, the count below it and the count in it ([Q][nprobs]; NaN when N = 0), and counts
// ([Q][6]: N, NaN, negative, positive, zero-bin, overflow).
void launch_quantile_select(hipStream_t s, const unsigned int *hist, const unsigned int *cnt,
                            int Q, unsigned long long total, const double *probs, int nprobs,
                            double *zlo, double *zhi, double *below, double *inbin,
                            double *counts);

}  // namespace bb
