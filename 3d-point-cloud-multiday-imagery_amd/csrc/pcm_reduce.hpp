// pcm_reduce.hpp — the wave reduce-scatter of the exact statistics passes (pcm_stats.hip, pcm_align.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace pcm_stats {

typedef unsigned long long u64;

constexpr int pow2_ceil(int w) {
    int p = 1;
    while (p < w) p <<= 1;
    return p;
}
constexpr int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// Sum v[0..WP) over the 64 lanes.  H = log2(WP) halving steps: at xor mask m a
// lane with bit m set keeps the upper half of its words and sends the lower one
// (the partner does the opposite), so after them a lane holds the one word
// lane >> (6 - H), summed over the lanes that share its low 6 - H bits; the
// remaining masks are plain butterfly adds.  Returns the wave total of word
// lane >> (6 - H) in every lane.
template <int WP>
__device__ __forceinline__ u64 reduce_scatter(u64 (&v)[WP], int lane) {
    constexpr int H = ilog2(WP);
#pragma unroll
    for (int s = 0; s < H; ++s) {
        const int half = WP >> (s + 1), mask = 32 >> s;
        const bool up = (lane & mask) != 0;
#pragma unroll
        for (int j = 0; j < half; ++j) {
            // both words are read first: selecting between the two array elements themselves makes the
            // compiler index the array by a register (a compare chain per word)
            const u64 a = v[j], b = v[j + half];
            const u64 keep = up ? b : a;
            const u64 send = up ? a : b;
            v[j] = keep + __shfl_xor(send, mask);
        }
    }
    u64 t = v[0];
#pragma unroll
    for (int mask = 32 >> H; mask >= 1; mask >>= 1) t += __shfl_xor(t, mask);
    return t;
}

}  // namespace pcm_stats
