// bb_summary.hip -- posterior summaries of trace rings, reduced on the device (gfx950).
//
// A chain batch fills its trace rings far faster than the host can take them,
// and the published protocol needs only per-coefficient mean, sd, effective sample size and
// R-hat.  k_trace_summary reduces each ring fill into fixed-size running sums (the records of
// bb_kernels.h: SummaryRing, kSummaryStride), k_summary_finalise turns them into
//   mean, var (divisor M - 1), acov[0..L] (divisor M, centred at the chain mean, as R's
//   acf(type = "covariance")), and the mean and variance of the first and last floor(M / 2)
//   samples (the split of diagnostics.rhat),
// which is what coda::effectiveSize, the pooled moments and split R-hat are computed from.
//
// One wave per (chain, parameter); lane k is lag k.  With z_t = x_t - x_0 (sums of squares
// stay safe when |mean| >> sd) the wave holds the window z_{t-k} in one register that moves up
// a lane per sample (DPP wave_shr:1, lane 0 takes z_t), and lane k adds z_t z_{t-k} to S_k once
// t >= k and z_t to H_k before.  At the end, with m = T / M and tail_k the sum of the last k
// values,
//   acov_k = [S_k - m ((T - H_k) + (T - tail_k)) + (M - k) m^2] / M.
// Every accumulator is one running sum in sample order, so the result is bitwise independent
// of the ring capacity, of the split into launches, of ring wrap and of the grid; a non-finite
// sample stays in its own wave.  The build is -ffp-contract=off: the products and the sums
// round separately.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "bb_kernels.h"
#include "bb_wave.h"

namespace bb {

namespace {

constexpr int kSumTile = 8;                 // adjacent parameters (waves) of a workgroup
constexpr int kSumChunk = kSummaryLanes;    // ring slots staged per pass: one per lane
constexpr int kSumThreads = 64 * kSumTile;  // = kSumChunk * kSumTile: a thread per staged value

// lane k takes lane k - 1's v, lane 0 takes `in` (wave_shr:1 leaves lane 0 its old value)
__device__ __forceinline__ double wave_shift_in(double v, double in) {
    const long long b = __double_as_longlong(v), n = __double_as_longlong(in);
    const int lo = __builtin_amdgcn_update_dpp((int)n, (int)b, 0x138, 0xf, 0xf, false);
    const int hi =
        __builtin_amdgcn_update_dpp((int)(n >> 32), (int)(b >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

}  // namespace

// Workgroup b: chain b / tiles, parameters [q0, q0 + kSumTile) with q0 = (b % tiles) kSumTile,
// wave w the parameter q0 + w.  The ring chunk [slot][p] is staged through LDS kSumChunk slots
// at a time, adjacent threads reading adjacent parameters of a slot; the scalars come from
// their own rings.
__global__ __launch_bounds__(kSumThreads) void k_trace_summary(
    const double *__restrict__ rb, const double *__restrict__ rs2, const double *__restrict__ rtau,
    const double *__restrict__ ralpha, int P, int Q, int cap, int tiles, int slot, int count,
    int s0, int M, int L, double *__restrict__ acc) {
    __shared__ double tile[kSumChunk][kSumTile + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * kSumTile, q = q0 + w;
    const bool live = q < Q;  // wave-uniform
    const size_t ring0 = (size_t)c * cap + slot;
    double *a = acc + ((size_t)c * Q + (live ? q : 0)) * kSummaryStride;
    double S = 0.0, H = 0.0, W = 0.0, T = 0.0, x0 = 0.0, hs0 = 0.0, hs1 = 0.0, hq0 = 0.0,
           hq1 = 0.0;
    if (live) {
        if (lane <= L) {
            S = a[lane];
            H = a[kSummaryLanes + lane];
            W = a[2 * kSummaryLanes + lane];
        }
        T = a[SUM_T];
        x0 = a[SUM_X0];
        hs0 = a[SUM_HS0];
        hs1 = a[SUM_HS1];
        hq0 = a[SUM_HQ0];
        hq1 = a[SUM_HQ1];
    }
    const int n2 = M / 2;  // the halves: samples [0, n2) and [M - n2, M)
    for (int base = 0; base < count; base += kSumChunk) {
        const int n = min(kSumChunk, count - base);
        __syncthreads();  // the previous chunk is consumed
        {
            const int i = tid / kSumTile, j = tid % kSumTile, qq = q0 + j;
            if (i < n && qq < Q) {
                const size_t sl = ring0 + base + i;
                tile[i][j] = qq < P ? rb[sl * P + qq]
                                    : (qq == P ? rs2 : qq == P + 1 ? rtau : ralpha)[sl];
            }
        }
        __syncthreads();
        if (!live) continue;
        const int t0 = s0 + base;
        const double xv = lane < n ? tile[lane][w] : 0.0;
        if (t0 == 0) x0 = readlane_f64(xv, 0);
        const double zv = xv - x0;
        if (t0 >= kSummaryMaxLag) {  // every lag has its partner: no head sums any more
            for (int i = 0; i < n; ++i) {
                const double z = readlane_f64(zv, i);
                const int t = t0 + i;
                W = wave_shift_in(W, z);
                const double zw = z * W;
                S += zw;
                T += z;
                if (t < n2) {
                    const double zz = z * z;
                    hs0 += z;
                    hq0 += zz;
                } else if (t >= M - n2) {
                    const double zz = z * z;
                    hs1 += z;
                    hq1 += zz;
                }
            }
        } else {
            for (int i = 0; i < n; ++i) {
                const double z = readlane_f64(zv, i);
                const int t = t0 + i;
                W = wave_shift_in(W, z);
                const double zw = z * W;
                if (lane <= t)
                    S += zw;
                else
                    H += z;
                T += z;
                if (t < n2) {
                    const double zz = z * z;
                    hs0 += z;
                    hq0 += zz;
                } else if (t >= M - n2) {
                    const double zz = z * z;
                    hs1 += z;
                    hq1 += zz;
                }
            }
        }
    }
    if (!live) return;
    if (lane <= L) {
        a[lane] = S;
        a[kSummaryLanes + lane] = H;
        a[2 * kSummaryLanes + lane] = W;
    }
    if (lane == 0) {
        a[SUM_T] = T;
        a[SUM_X0] = x0;
        a[SUM_HS0] = hs0;
        a[SUM_HS1] = hs1;
        a[SUM_HQ0] = hq0;
        a[SUM_HQ1] = hq1;
    }
}

// One wave per (chain, parameter) record, lane k the lag k: the outputs from the sums.  Lags
// >= M are 0; a half of fewer than one sample has no moments (NaN).
__global__ __launch_bounds__(256) void k_summary_finalise(
    const double *__restrict__ acc, long records, int M, int L, double *__restrict__ mean,
    double *__restrict__ var, double *__restrict__ acov, double *__restrict__ hmean,
    double *__restrict__ hvar) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= records) return;  // wave-uniform
    const double *a = acc + (size_t)r * kSummaryStride;
    double S = 0.0, H = 0.0, W = 0.0;
    if (lane <= L) {
        S = a[lane];
        H = a[kSummaryLanes + lane];
        W = a[2 * kSummaryLanes + lane];
    }
    const double T = a[SUM_T], x0 = a[SUM_X0];
    const double dM = (double)M;
    const double m = T / dM;
    double tail = 0.0;  // the sum of the last `lane` values, newest first
    for (int j = 0; j < kSummaryMaxLag; ++j) {
        const double wj = readlane_f64(W, j);
        if (lane > j) tail += wj;
    }
    double v = 0.0;
    if (lane < M) {
        const double mm = m * m;
        const double cross = m * ((T - H) + (T - tail));
        const double sq = (double)(M - lane) * mm;
        v = ((S - cross) + sq) / dM;
    }
    if (lane <= L) acov[(size_t)r * (L + 1) + lane] = v;
    if (lane == 0) {
        mean[r] = x0 + m;
        var[r] = (v * dM) / (dM - 1.0);
    }
    if (lane < 2) {
        const int n2 = M / 2;
        const double hs = a[SUM_HS0 + lane], hq = a[SUM_HQ0 + lane], dn = (double)n2;
        double hm = __builtin_nan(""), hv = __builtin_nan("");
        if (n2 >= 1) {
            hm = x0 + hs / dn;
            const double sq = hs * hs;
            hv = (hq - sq / dn) / (dn - 1.0);
        }
        hmean[(size_t)r * 2 + lane] = hm;
        hvar[(size_t)r * 2 + lane] = hv;
    }
}

void launch_trace_summary(hipStream_t s, const SummaryRing &r, int K, int slot, int count, int s0,
                          int M, int L, double *acc) {
    if (count <= 0 || K <= 0) return;
    const int Q = r.params(), tiles = (Q + kSumTile - 1) / kSumTile;
    if (L < 0 || L > kSummaryMaxLag || slot < 0 || slot + count > r.cap || s0 < 0 ||
        s0 + count > M || (size_t)K * tiles > 0x7fffffffu)
        throw std::invalid_argument("launch_trace_summary: arguments out of range");
    k_trace_summary<<<K * tiles, kSumThreads, 0, s>>>(r.beta, r.sig2, r.tau, r.alpha, r.p, Q,
                                                      r.cap, tiles, slot, count, s0, M, L, acc);
}

void launch_summary_finalise(hipStream_t s, const double *acc, int K, int Q, int M, int L,
                             double *mean, double *var, double *acov, double *hmean,
                             double *hvar) {
    const long records = (long)K * Q;
    if (records <= 0) return;
    if (L < 0 || L > kSummaryMaxLag || M < 1 || (records + 3) / 4 > 0x7fffffffL)
        throw std::invalid_argument("launch_summary_finalise: arguments out of range");
    k_summary_finalise<<<(unsigned)((records + 3) / 4), 256, 0, s>>>(acc, records, M, L, mean,
                                                                      var, acov, hmean, hvar);
}

}  // namespace bb
