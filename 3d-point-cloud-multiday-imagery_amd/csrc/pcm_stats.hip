// pcm_stats.hip — exact per-(group, cluster) moments of a labelled cloud (DESIGN.md §4,
// "Cluster statistics").
//
// One pass over (X, labels[, groups]) in the caller's row order.  Every row adds
// W = PCM_STATS_WORDS(D) integer words to the row (g, label) of `out`:
//
//   word 0            1                                   (count)
//   words 1..D        xq_a = trunc(ldexp(x_a, q_a))       (fixed_i of the engine)
//   then per a <= b   lo = p & 0xffffffff, hi = p >> 32   (p = xq_a * xq_b, int64)
//
// All adds are integer adds, so the words do not depend on the order of the
// rows, on the grid, or on how the rows are split over calls and ranks.
//
// Accumulation paths (which one a row takes never changes a bit of the result):
//   * wave path: the rows are not sorted, but real clouds are coherent -- the
//     64 rows of a wave round share one or two keys (g * k + label).  Up to
//     LEADERS times per round the wave takes the key of its first pending lane,
//     (the carried key before any other) and ballots the lanes holding it; each
//     of them adds its W words to its own registers.  Every wave takes a
//     contiguous run of rounds and carries these per-lane sums of ONE key across
//     them; only when the key changes are they summed over the wave with a
//     reduce-scatter (each xor step halves the words a lane carries; lane l ends
//     with the total of word l >> SH) and flushed: one no-return atomic
//     wave-instruction over the W contiguous words of the row;
//   * straggler path: keys held by fewer than MIN_GROUP lanes, and whatever is
//     left after LEADERS keys, add their W words with per-lane atomics (a randomly
//     ordered cloud takes this path: slow, equally exact).
// Skipped rows (label outside [0, k), group >= n_groups, a non-finite
// coordinate) add nothing but 1 to the trailing word.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "pcm_common.hpp"
#include "pcm_kmeans.h"
#include "pcm_reduce.hpp"   // u64, pow2_ceil, ilog2, reduce_scatter

namespace pcm_stats {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int LEADERS = 4;      // key switches (flushes of the carried row) per round
constexpr int MIN_GROUP = 4;    // fewer lanes on a new key: per-lane atomics are cheaper than a flush
constexpr int MIN_ROUNDS = 4;   // rounds per wave before the grid shrinks

struct QExp {
    int q[4];
};

template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<__half>(__half v) { return __half2float(v); }

// trunc(x * 2^q): the engine's fixed_i (pcm_kernels.hpp)
__device__ __forceinline__ int fixed_i(float x, int q) { return (int)__builtin_ldexpf(x, q); }

template <typename T, int D, bool GROUPS>
__global__ __launch_bounds__(TPB) void k_cluster_stats(const T *__restrict__ X, long long n,
                                                       const int32_t *__restrict__ labels,
                                                       const uint8_t *__restrict__ groups, int n_groups, int k, QExp qe,
                                                       u64 *__restrict__ out, long long rounds, long long rpw) {
    constexpr int W = PCM_STATS_WORDS(D), WP = pow2_ceil(W), SH = 6 - ilog2(WP);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const long long r0 = wave * rpw, r1 = r0 + rpw < rounds ? r0 + rpw : rounds;
    const int myword = lane >> SH;
    const bool owner = (lane & ((1 << SH) - 1)) == 0 && myword < W;
    int ckey = -1;          // key of the carried row (wave-uniform), -1: none
    u64 acc[W];             // this lane's share of the carried row: summed over the wave only at the flush
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0;
    unsigned skipped = 0;   // wave-uniform
    auto flush = [&]() {
        if (ckey < 0) return;
        u64 v[WP];
#pragma unroll
        for (int w = 0; w < WP; ++w) v[w] = w < W ? acc[w < W ? w : 0] : 0ull;
        const u64 tot = reduce_scatter<WP>(v, lane);
        if (owner) atomicAdd(out + (long long)ckey * W + myword, tot);
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = 0;
    };
    // the loads of round r + 1 are issued before round r is reduced (one round per wave in flight
    // would leave the pass latency-bound); they are unconditional -- the row index is clamped to
    // n - 1 and what a lane past the end loads is never used -- so that no branch makes them wait
    T nx[D];
    int nlab = 0, ng = 0;
    auto fetch = [&](long long r) {
        long long i = r * 64 + lane;
        i = i < n ? i : n - 1;
        nlab = labels[i];
        if (GROUPS) ng = (int)groups[i];
#pragma unroll
        for (int a = 0; a < D; ++a) nx[a] = X[i * D + a];
    };
    if (r0 >= r1) return;
    fetch(r0);
    for (long long r = r0; r < r1; ++r) {
        const long long i = r * 64 + lane;
        const int lab = nlab, g = ng;
        T xr[D];
#pragma unroll
        for (int a = 0; a < D; ++a) xr[a] = nx[a];
        fetch(r + 1);
        bool valid = false;
        int key = -1;
        u64 val[W];
#pragma unroll
        for (int w = 0; w < W; ++w) val[w] = 0;
        if (i < n) {
            float x[D];
            bool fin = true;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                x[a] = to_f<T>(xr[a]);
                fin = fin && isfinite(x[a]);
            }
            valid = fin && lab >= 0 && lab < k && g < n_groups;
            if (valid) {
                key = g * k + lab;
                long long xq[D];
                val[0] = 1;
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    xq[a] = (long long)fixed_i(x[a], qe.q[a]);
                    val[1 + a] = (u64)xq[a];
                }
#pragma unroll
                for (int a = 0; a < D; ++a)
#pragma unroll
                    for (int b = a; b < D; ++b) {
                        const int w = 1 + D + 2 * (a * D - a * (a - 1) / 2 + (b - a));   // upper triangle, row-major
                        const long long p = xq[a] * xq[b];
                        val[w] = (u64)p & 0xffffffffull;
                        val[w + 1] = (u64)(p >> 32);
                    }
            }
        }
        skipped += (unsigned)__popcll(__ballot(i < n && !valid));
        u64 todo = __ballot(valid), strag = 0;
        for (int t = 0, switched = 0; t < 2 * LEADERS && switched < LEADERS && todo; ++t) {
            // the carried key first (its lanes cost W adds and no flush), then the key of the first pending lane
            u64 m = ckey >= 0 ? __ballot(valid && key == ckey) & todo : 0ull;
            int lk = ckey;
            if (!m) {
                const int leader = __ffsll((long long)todo) - 1;
                lk = __builtin_amdgcn_readfirstlane(__shfl(key, leader));
                m = __ballot(valid && key == lk) & todo;
            }
            todo &= ~m;
            if (lk != ckey) {
                if (__popcll(m) < MIN_GROUP) {   // e.g. a stray label inside a run: not worth giving up the carried row
                    strag |= m;
                    continue;
                }
                flush();
                ckey = lk;
                ++switched;
            }
            if ((m >> lane) & 1ull) {
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] += val[w];
            }
        }
        strag |= todo;
        if ((strag >> lane) & 1ull) {
            u64 *row = out + (long long)key * W;
#pragma unroll
            for (int w = 0; w < W; ++w) atomicAdd(row + w, val[w]);
        }
    }
    flush();
    if (lane == 0 && skipped) atomicAdd(out + (long long)n_groups * k * W, (u64)skipped);
}

}  // namespace pcm_stats

using namespace pcm_stats;

extern "C" {

int pcm_cluster_stats(const void *X, int dtype, int64_t n, int d, const int32_t *labels, const uint8_t *groups,
                      int n_groups, int k, const int32_t *q, uint64_t *out, void *stream) {
    if (d < 1 || d > 4) return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: d must be 1..4");
    if (dtype != PCM_F32 && dtype != PCM_F16) return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: dtype must be PCM_F32 or PCM_F16");
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: n must be below 2^31 (exactness of the limb sums)");
    if (k < 1) return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: k must be >= 1");
    if (n_groups < 1 || n_groups > PCM_STATS_MAXG)
        return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: n_groups must be 1.." + std::to_string(PCM_STATS_MAXG));
    if ((int64_t)n_groups * k > (int64_t)0x7fffffff) return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: n_groups * k must be below 2^31");
    if (n > 0 && (!out || !labels || !X || !q)) return pcm_fail(PCM_E_ARG, "pcm_cluster_stats: X, labels, q or out is null");
    if (n == 0) return 0;   // nothing to add: no device call
    hipStream_t s = (hipStream_t)stream;
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
        ncu = 256;
    // every wave takes a contiguous run of rounds (64 rows each), so that a row it carries in
    // registers is flushed once per run of equal keys, not once per round
    const long long rounds = (n + 63) / 64;
    long long nblk = std::min<long long>((long long)ncu * 16, (rounds + WAVES * MIN_ROUNDS - 1) / (WAVES * MIN_ROUNDS));
    if (const char *e = std::getenv("PCM_STATS_BLOCKS")) {   // measurement: the words must not depend on the grid
        const long long v = std::atoll(e);
        if (v >= 1) nblk = std::min<long long>(v, 1 << 20);
    }
    nblk = std::max<long long>(1, std::min(nblk, (rounds + WAVES - 1) / WAVES));
    const long long rpw = (rounds + nblk * WAVES - 1) / (nblk * WAVES);
    QExp qe = {{0, 0, 0, 0}};
    for (int a = 0; a < d; ++a) qe.q[a] = q[a];
    auto launch = [&](auto TT, auto DD) {
        using T = decltype(TT);
        constexpr int D = decltype(DD)::value;
        if (groups)
            k_cluster_stats<T, D, true><<<(unsigned)nblk, TPB, 0, s>>>((const T *)X, n, labels, groups, n_groups, k, qe,
                                                                       (u64 *)out, rounds, rpw);
        else
            k_cluster_stats<T, D, false><<<(unsigned)nblk, TPB, 0, s>>>((const T *)X, n, labels, groups, n_groups, k, qe,
                                                                        (u64 *)out, rounds, rpw);
    };
    auto by_d = [&](auto TT) {
        switch (d) {
        case 1: launch(TT, std::integral_constant<int, 1>{}); break;
        case 2: launch(TT, std::integral_constant<int, 2>{}); break;
        case 3: launch(TT, std::integral_constant<int, 3>{}); break;
        default: launch(TT, std::integral_constant<int, 4>{}); break;
        }
    };
    if (dtype == PCM_F16) by_d(__half{});
    else by_d(float{});
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("k_cluster_stats: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
