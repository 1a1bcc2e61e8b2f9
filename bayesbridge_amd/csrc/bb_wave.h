// bb_wave.h -- the wave64 primitives every translation unit shares (gfx950): the 64-bit lane
// read and the xor-tree sums.  Each exists once, so a sum's tree -- which fixes its bits -- is
// named once.
#pragma once
#include <hip/hip_runtime.h>

namespace bb {

// v of lane `lane` (uniform over the wave), in every lane: two v_readlane_b32
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// xor tree inside aligned groups of W lanes; every lane of the group gets the sum
template <int W>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum over the wave in every lane (offsets 32, 16, ..., 1)
__device__ __forceinline__ double wave_sum_all(double v) { return group_sum<64>(v); }

}  // namespace bb
