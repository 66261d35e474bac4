// pcm_grid.hip — exact height-map raster of a (labelled, multi-day) cloud (DESIGN.md §4,
// "Height grid").
//
// One pass over (X[, labels][, groups]) in the caller's row order; X rows are (z, y, x).
// A row's pixel is (fy, fx) = floor(ldexp((y, x) - (oy, ox), -s)) in float32 (one rounded
// subtraction, an exact scaling, a floor), its height zq = trunc(ldexp(z, q)) (fixed_i of
// the engine).  It updates four 64-bit words of its (group, pixel), each in its own H x W
// plane (include/pcm_kmeans.h has the layout):
//
//   word 0   count                                              integer add
//   word 1   sum zq (int64)                                     integer add
//   word 2   ((zq + 2^25) << 32) | (0xffffffff - label)         unsigned max   (top)
//   word 3   ((2^25 - zq) << 32) | (0xffffffff - label)         unsigned max   (bottom)
//
// Adds and maxima of integers commute: the words do not depend on the order of the rows,
// on the grid, or on how the rows are split over calls and ranks.
//
// Accumulation: per 64-row round the lanes whose key (g*H + fy)*W + fx equals their left
// neighbour's form a run; count, sum, top and bottom are combined over each run with a
// segmented scan over the wave and the last lane of the run issues the four no-return
// atomics.  When no two adjacent lanes share a key (a raster cloud at s = 0) the scan is
// skipped wave-uniformly and every lane issues its own: 64 consecutive 8-byte words per
// atomic wave-instruction.  Equal keys that are not adjacent issue one set of atomics per
// run; which lanes were combined never changes a bit of the result.
// Skipped rows (a non-finite coordinate, label outside [0, k), group >= n_groups,
// |zq| >= 2^25) add 1 to the second trailing word, valid rows outside the raster 1 to the
// first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "pcm_common.hpp"
#include "pcm_kmeans.h"

namespace pcm_grid {

typedef unsigned long long u64;

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MIN_ROUNDS = 4;   // rounds per wave before the grid shrinks
constexpr int ZBIAS = 1 << 25;  // |zq| < 2^25: the engine's QBITS

template <bool LABELS, bool GROUPS>
__global__ __launch_bounds__(TPB) void k_height_grid(const float *__restrict__ X, long long n,
                                                     const int32_t *__restrict__ labels,
                                                     const uint8_t *__restrict__ groups, int n_groups, int k, int H, int W,
                                                     float oy, float ox, int s, int q, u64 *__restrict__ out,
                                                     long long rounds, long long rpw) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const long long r0 = wave * rpw, r1 = r0 + rpw < rounds ? r0 + rpw : rounds;
    const long long HW = (long long)H * W;
    const float fH = (float)H, fW = (float)W;   // exact: H, W <= 2^24
    unsigned outside = 0, skipped = 0;          // wave-uniform
    // the loads of round r + 1 are issued before round r is reduced; they are unconditional -- the
    // row index is clamped to n - 1 and what a lane past the end loads is never used
    float nz = 0.f, ny = 0.f, nx = 0.f;
    int nlab = 0, ng = 0;
    auto fetch = [&](long long r) {
        long long i = r * 64 + lane;
        i = i < n ? i : n - 1;
        if (LABELS) nlab = labels[i];
        if (GROUPS) ng = (int)groups[i];
        nz = X[i * 3];
        ny = X[i * 3 + 1];
        nx = X[i * 3 + 2];
    };
    if (r0 >= r1) return;
    fetch(r0);
    for (long long r = r0; r < r1; ++r) {
        const long long i = r * 64 + lane;
        const int lab = nlab, g = ng;
        const float z = nz, y = ny, x = nx;
        fetch(r + 1);
        const bool live = i < n;
        bool valid = false, inside = false;
        int key = -1, zq = 0;
        if (live) {
            const float zt = truncf(__builtin_ldexpf(z, q));
            // a NaN or infinite zt fails the comparison
            valid = isfinite(z) && isfinite(y) && isfinite(x) && lab >= 0 && lab < k && g < n_groups &&
                    fabsf(zt) < (float)ZBIAS;
            if (valid) {
                const float fy = floorf(__builtin_ldexpf(y - oy, -s));
                const float fx = floorf(__builtin_ldexpf(x - ox, -s));
                inside = fy >= 0.f && fy < fH && fx >= 0.f && fx < fW;   // compared before the conversion
                if (inside) {
                    key = (g * H + (int)fy) * W + (int)fx;               // below 2^31: G*H*W is
                    zq = (int)zt;
                }
            }
        }
        skipped += (unsigned)__popcll(__ballot(live && !valid));
        outside += (unsigned)__popcll(__ballot(valid && !inside));
        if (!__ballot(key >= 0)) continue;
        int cnt = 1, sum = zq;                                           // 64 rows: |sum| < 2^31
        const u64 lo = (u64)(0xffffffffu - (unsigned)lab);
        u64 top = ((u64)(unsigned)(zq + ZBIAS) << 32) | lo;
        u64 bot = ((u64)(unsigned)(ZBIAS - zq) << 32) | lo;
        // heads of the runs of adjacent lanes with equal key (a lane without a pixel is a run of its own)
        const int prev = __shfl_up(key, 1);
        const bool head = lane == 0 || key != prev || key < 0;
        const u64 hm = __ballot(head);
        if (hm != ~0ull) {
            // inclusive segmented scan: a lane takes what lies d lanes to its left while that is still its run
            const int myhead = 63 - __clzll((long long)(hm & (~0ull >> (63 - lane))));
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int c2 = __shfl_up(cnt, d), s2 = __shfl_up(sum, d);
                const u64 t2 = __shfl_up(top, d), b2 = __shfl_up(bot, d);
                if (lane - d >= myhead) {
                    cnt += c2;
                    sum += s2;
                    top = t2 > top ? t2 : top;
                    bot = b2 > bot ? b2 : bot;
                }
            }
        }
        const bool tail = (((hm >> 1) | (1ull << 63)) >> lane) & 1ull;
        if (tail && key >= 0) {
            u64 *p = out + ((long long)key + (long long)g * 3 * HW);     // plane (g*4 + 0), this pixel
            atomicAdd(p, (u64)cnt);
            atomicAdd(p + HW, (u64)(long long)sum);
            atomicMax(p + 2 * HW, top);
            atomicMax(p + 3 * HW, bot);
        }
    }
    if (lane == 0) {
        u64 *trail = out + 4ll * n_groups * HW;
        if (outside) atomicAdd(trail, (u64)outside);
        if (skipped) atomicAdd(trail + 1, (u64)skipped);
    }
}

}  // namespace pcm_grid

using namespace pcm_grid;

extern "C" {

int pcm_height_grid(const float *X, int64_t n, const int32_t *labels, int k, const uint8_t *groups, int n_groups, int H,
                    int W, float oy, float ox, int cell_log2, int q, uint64_t *out, void *stream) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_height_grid: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_height_grid: n must be below 2^31 (exactness of the sums)");
    if (H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return pcm_fail(PCM_E_ARG, "pcm_height_grid: H and W must be 1..2^24");
    if (n_groups < 1 || n_groups > PCM_GRID_MAXG)
        return pcm_fail(PCM_E_ARG, "pcm_height_grid: n_groups must be 1.." + std::to_string(PCM_GRID_MAXG));
    // H*W <= 2^48 and n_groups <= 2^8: the product fits in int64
    if ((int64_t)n_groups * H * W > (int64_t)0x7fffffff) return pcm_fail(PCM_E_ARG, "pcm_height_grid: n_groups * H * W must be below 2^31");
    if (k < 1) return pcm_fail(PCM_E_ARG, "pcm_height_grid: k must be >= 1");
    if (cell_log2 < -8 || cell_log2 > 16) return pcm_fail(PCM_E_ARG, "pcm_height_grid: cell_log2 must be -8..16");
    if (n > 0 && (!X || !out)) return pcm_fail(PCM_E_ARG, "pcm_height_grid: X or out is null");
    if (n == 0) return 0;   // nothing to add: no device call
    hipStream_t st = (hipStream_t)stream;
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
        ncu = 256;
    const long long rounds = (n + 63) / 64;
    long long nblk = std::min<long long>((long long)ncu * 16, (rounds + WAVES * MIN_ROUNDS - 1) / (WAVES * MIN_ROUNDS));
    if (const char *e = std::getenv("PCM_GRID_BLOCKS")) {   // measurement: the words must not depend on the grid
        const long long v = std::atoll(e);
        if (v >= 1) nblk = std::min<long long>(v, 1 << 20);
    }
    nblk = std::max<long long>(1, std::min(nblk, (rounds + WAVES - 1) / WAVES));
    const long long rpw = (rounds + nblk * WAVES - 1) / (nblk * WAVES);
#define PCM_GRID_LAUNCH(L, G)                                                                                             \
    k_height_grid<L, G><<<(unsigned)nblk, TPB, 0, st>>>(X, n, labels, groups, n_groups, k, H, W, oy, ox, cell_log2, q,    \
                                                        (u64 *)out, rounds, rpw)
    if (labels && groups) PCM_GRID_LAUNCH(true, true);
    else if (labels) PCM_GRID_LAUNCH(true, false);
    else if (groups) PCM_GRID_LAUNCH(false, true);
    else PCM_GRID_LAUNCH(false, false);
#undef PCM_GRID_LAUNCH
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("k_height_grid: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
