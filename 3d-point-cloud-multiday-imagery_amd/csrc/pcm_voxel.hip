// pcm_voxel.hip — exact voxel occupancy, fixed-point centroid sums and day masks of a cloud
// ("Voxels").
//
// Rows are (z, y, x) float32.  The lattice is anchored at `origin`; on axis a the cell of a finite
// row is, in float32 with every operation rounded and no contraction,
//     c_a = floorf((x_a - o_a) * inv_a),   inv_a = float32(1.0 / float64(v_a))  (formed on the host).
// The map is monotone in x_a (a rounded subtraction of a constant, a rounded product with a
// positive constant and floorf are all non-decreasing), so the cells of the bounding box's two
// corners bound every row's cell: k_voxel_plan checks them alone.  A row with a NaN or Inf
// coordinate belongs to no voxel.
//
// Steps: k_voxel_bbox / k_voxel_plan / k_voxel_keys write one 63-bit key per row (relative
// (cz, cy, cx), 21 bits each, x fastest; the skip key 2^63 - 1 sorts last); the caller sorts;
// k_voxel_heads counts, per wave of 64 sorted rows, the segment heads (key differs from the
// previous sorted row's), k_voxel_scan_tiles / k_voxel_scan_top turn the counts into each wave's
// first voxel index (two levels: within a tile of 1024 waves, and the tiles) and their total M;
// k_voxel_reduce gathers X[perm] per wave, scans count, fixed-point sums, group mask and lowest row
// over the segments inside the wave and writes a segment that lies wholly inside the wave with
// plain stores.  Only a wave's first segment (when it began in an earlier wave) and
// its last (when it goes on in the next) go to the initialised outputs with integer atomics: at
// most two sets per wave.  Integer adds, ors and minima commute: the same bits for any row order,
// sort and launch shape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

#include "pcm_common.hpp"
#include "pcm_kmeans.h"

namespace pcm_voxel {

typedef unsigned long long u64;
typedef long long i64;

constexpr int TPB = PCM_VOXEL_TPB;
constexpr int WAVES = TPB / 64;
constexpr int SCAN_TPB = 1024;
constexpr int AXIS_BITS = 21;
constexpr i64 AXIS_MAX = ((i64)1 << AXIS_BITS) - 1;
constexpr i64 SKIP_KEY = 0x7fffffffffffffffll;   // sorts behind every cell
constexpr float CELL_ABS_MAX = 1099511627776.f;  // 2^40: |cell| stays exact in int64 arithmetic

static_assert(TPB % 64 == 0, "whole waves");

// info words (device int64[PCM_VOXEL_INFO_WORDS]); 9..14 are the box as order-preserving uint32
enum { I_ERR = 0, I_CLO = 1, I_SPAN = 4, I_SKIPPED = 7, I_M = 8, I_UMIN = 9, I_UMAX = 12, I_BADPERM = 15 };

struct Lattice {
    float o[3], inv[3];
};

__device__ __forceinline__ unsigned enc(float f) {
    const unsigned b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned u) {
    return __uint_as_float((u >> 31) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ float cellf(float x, float o, float inv) { return floorf((x - o) * inv); }

__global__ void k_voxel_init(i64 *info) {
    const int t = threadIdx.x;
    if (t < PCM_VOXEL_INFO_WORDS) info[t] = (t >= I_UMIN && t < I_UMIN + 3) ? (i64)0xffffffffu : 0;
}

// bounding box of the finite rows and the number of the others
__global__ __launch_bounds__(TPB) void k_voxel_bbox(const float *__restrict__ X, i64 n, i64 *info) {
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    unsigned skipped = 0;
    for (i64 i = (i64)blockIdx.x * TPB + threadIdx.x; i < n; i += (i64)gridDim.x * TPB) {
        const float z = X[i * 3], y = X[i * 3 + 1], x = X[i * 3 + 2];
        if (isfinite(z) && isfinite(y) && isfinite(x)) {
            const unsigned e[3] = {enc(z), enc(y), enc(x)};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = e[a] < lo[a] ? e[a] : lo[a];
                hi[a] = e[a] > hi[a] ? e[a] : hi[a];
            }
        } else {
            ++skipped;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned l2 = __shfl_xor(lo[a], d), h2 = __shfl_xor(hi[a], d);
            lo[a] = l2 < lo[a] ? l2 : lo[a];
            hi[a] = h2 > hi[a] ? h2 : hi[a];
        }
        skipped += __shfl_xor(skipped, d);
    }
    // one set of atomics per block: they all land on the same seven words
    __shared__ unsigned part[WAVES][7];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            part[wv][a] = lo[a];
            part[wv][3 + a] = hi[a];
        }
        part[wv][6] = skipped;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int t = threadIdx.x;
        unsigned v = part[0][t];
        for (int w = 1; w < WAVES; ++w) {
            const unsigned o = part[w][t];
            v = t < 3 ? (o < v ? o : v) : t < 6 ? (o > v ? o : v) : v + o;
        }
        // the words hold values below 2^32: a 64-bit unsigned min / max orders them as the uint32 does
        if (t < 3) atomicMin((u64 *)info + I_UMIN + t, (u64)v);
        else if (t < 6) atomicMax((u64 *)info + I_UMAX + (t - 3), (u64)v);
        else if (v) atomicAdd((u64 *)info + I_SKIPPED, (u64)v);
    }
}

// one thread: the cells of the box's two corners bound every row's cell (the map is monotone)
__global__ void k_voxel_plan(i64 *info, Lattice L) {
    if (threadIdx.x || blockIdx.x) return;
    i64 clo[3] = {0, 0, 0}, span[3] = {0, 0, 0}, err = 0;
    if (info[I_UMIN] <= info[I_UMAX]) {   // there is a finite row
        for (int a = 0; a < 3; ++a) {
            const float lo = cellf(dec((unsigned)info[I_UMIN + a]), L.o[a], L.inv[a]);
            const float hi = cellf(dec((unsigned)info[I_UMAX + a]), L.o[a], L.inv[a]);
            if (!isfinite(lo) || !isfinite(hi)) {
                err |= PCM_VOXEL_E_NONFINITE;
            } else if (fabsf(lo) > CELL_ABS_MAX || fabsf(hi) > CELL_ABS_MAX) {
                err |= PCM_VOXEL_E_MAGNITUDE;
            } else {
                clo[a] = (i64)lo;
                span[a] = (i64)hi - clo[a] + 1;
                if (span[a] > AXIS_MAX + 1) err |= PCM_VOXEL_E_SPAN;
            }
        }
        // the key of the last cell of a full 2^21-cubed lattice would be the skip key
        if (!err && span[0] == AXIS_MAX + 1 && span[1] == AXIS_MAX + 1 && span[2] == AXIS_MAX + 1) err |= PCM_VOXEL_E_SPAN;
    }
    info[I_ERR] = err;
    for (int a = 0; a < 3; ++a) {
        info[I_CLO + a] = clo[a];
        info[I_SPAN + a] = span[a];
    }
}

__global__ __launch_bounds__(TPB) void k_voxel_keys(const float *__restrict__ X, i64 n, const i64 *__restrict__ info,
                                                    Lattice L, i64 *__restrict__ keys) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const float z = X[i * 3], y = X[i * 3 + 1], x = X[i * 3 + 2];
    i64 key = SKIP_KEY;
    if (!info[I_ERR] && isfinite(z) && isfinite(y) && isfinite(x)) {   // after an error every row is skipped
        const i64 cz = (i64)cellf(z, L.o[0], L.inv[0]) - info[I_CLO], cy = (i64)cellf(y, L.o[1], L.inv[1]) - info[I_CLO + 1],
                  cx = (i64)cellf(x, L.o[2], L.inv[2]) - info[I_CLO + 2];
        key = (((cz << AXIS_BITS) | cy) << AXIS_BITS) | cx;   // each in [0, 2^21): k_voxel_plan
    }
    keys[i] = key;
}

// a wave's segment heads: valid rows whose key differs from the previous sorted row's
__device__ __forceinline__ u64 wave_heads(const i64 *__restrict__ skeys, i64 pos, i64 n, int lane, i64 &key, bool &valid) {
    key = pos < n ? skeys[pos] : SKIP_KEY;
    valid = key != SKIP_KEY;
    i64 prev = __shfl_up(key, 1);
    if (lane == 0) prev = pos > 0 && pos < n ? skeys[pos - 1] : (i64)-1;   // -1: no key
    return __ballot(valid && key != prev);
}

__global__ __launch_bounds__(TPB) void k_voxel_heads(const i64 *__restrict__ skeys, i64 n, int32_t *__restrict__ wave_base) {
    const int lane = threadIdx.x & 63;
    const i64 w = (i64)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w * 64 >= n) return;
    i64 key;
    bool valid;
    const u64 heads = wave_heads(skeys, w * 64 + lane, n, lane, key, valid);
    if (lane == 0) wave_base[w] = __popcll(heads);
}

// one tile of SCAN_TPB waves per block: wave_base[w] becomes the number of heads before wave w in
// its tile, tile_base[b] the heads of tile b
__global__ __launch_bounds__(SCAN_TPB) void k_voxel_scan_tiles(int32_t *__restrict__ wave_base, i64 nw,
                                                               int32_t *__restrict__ tile_base) {
    __shared__ int part[SCAN_TPB / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const i64 i = (i64)blockIdx.x * SCAN_TPB + t;
    const int c = i < nw ? wave_base[i] : 0;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) part[wv] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_TPB / 64; ++w) {
        before += w < wv ? part[w] : 0;
        total += part[w];
    }
    if (i < nw) wave_base[i] = before + incl - c;
    if (t == 0) tile_base[blockIdx.x] = total;
}

// one block: tile_base[b] becomes the number of heads before tile b, info[I_M] their total
__global__ __launch_bounds__(SCAN_TPB) void k_voxel_scan_top(int32_t *__restrict__ tile_base, i64 nt, i64 *info) {
    __shared__ i64 part[SCAN_TPB];
    const int t = threadIdx.x;
    const i64 per = (nt + SCAN_TPB - 1) / SCAN_TPB;
    const i64 a = (i64)t * per < nt ? (i64)t * per : nt, b = a + per < nt ? a + per : nt;
    i64 s = 0;
    for (i64 i = a; i < b; ++i) s += tile_base[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < SCAN_TPB; d <<= 1) {
        const i64 v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    i64 run = part[t] - s;   // exclusive
    for (i64 i = a; i < b; ++i) {
        const int32_t c = tile_base[i];
        tile_base[i] = (int32_t)run;
        run += c;
    }
    if (t == SCAN_TPB - 1) info[I_M] = part[t];
}

__global__ __launch_bounds__(TPB) void k_voxel_fill(i64 m, int32_t *__restrict__ counts, i64 *__restrict__ sums,
                                                    int32_t *__restrict__ first, i64 *__restrict__ mask) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    counts[i] = 0;
    sums[i * 3] = sums[i * 3 + 1] = sums[i * 3 + 2] = 0;
    first[i] = 0x7fffffff;
    if (mask) mask[i] = 0;
}

struct QExp {
    int q[3];
};

template <bool GROUPS>
__global__ __launch_bounds__(TPB) void k_voxel_reduce(const float *__restrict__ X, const uint8_t *__restrict__ groups, i64 n,
                                                      const i64 *__restrict__ skeys, const i64 *__restrict__ perm,
                                                      const int32_t *__restrict__ wave_base,
                                                      const int32_t *__restrict__ tile_base, QExp qe, i64 m,
                                                      i64 *__restrict__ cells, int32_t *__restrict__ counts,
                                                      i64 *__restrict__ sums, int32_t *__restrict__ first,
                                                      i64 *__restrict__ mask, int32_t *__restrict__ inverse, i64 *info) {
    const int lane = threadIdx.x & 63;
    const i64 w = (i64)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w * 64 >= n) return;
    const i64 pos = w * 64 + lane;
    i64 key;
    bool valid;
    const u64 heads = wave_heads(skeys, pos, n, lane, key, valid);
    i64 row = pos < n ? perm[pos] : 0;
    if (row < 0 || row >= n) {   // not a permutation: nothing is written for this row
        info[I_BADPERM] = 1;
        row = -1;
        valid = false;
    }
    const u64 vmask = __ballot(valid);
    if (pos < n && row >= 0 && !valid) inverse[row] = -1;
    if (!vmask) return;
    const u64 upto = lane == 63 ? ~0ull : (2ull << lane) - 1;          // lanes 0..lane
    const u64 mine = heads & upto;
    const int start = mine ? 63 - __clzll(mine) : 0;                    // first lane of my segment in this wave
    const i64 seg = (i64)tile_base[w / SCAN_TPB] + wave_base[w] + __popcll(mine) - 1;
    i64 s[3] = {0, 0, 0};
    u64 gm = 0;
    int rmin = 0x7fffffff;
    if (valid) {
        // trunc(x * 2^q): the engine's fixed_i
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = (i64)(int)__builtin_ldexpf(X[row * 3 + a], qe.q[a]);
        if (GROUPS) gm = 1ull << (groups[row] & 63);
        rmin = (int)row;
    }
    // segmented inclusive scan: a lane takes from lane - d only inside its own segment
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool take = valid && lane - d >= start;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const i64 o = __shfl_up(s[a], d);
            if (take) s[a] += o;
        }
        if (GROUPS) {
            const u64 o = __shfl_up(gm, d);
            if (take) gm |= o;
        }
        const int o = __shfl_up(rmin, d);
        if (take && o < rmin) rmin = o;
    }
    if (!valid) return;
    const bool ok = seg >= 0 && seg < m;   // always, when skeys is what k_voxel_heads saw
    if (!ok) {
        info[I_BADPERM] = 1;
        return;
    }
    inverse[row] = (int32_t)seg;
    if ((heads >> lane) & 1) {   // every voxel has one head
        cells[seg * 3] = info[I_CLO] + (key >> (2 * AXIS_BITS));
        cells[seg * 3 + 1] = info[I_CLO + 1] + ((key >> AXIS_BITS) & AXIS_MAX);
        cells[seg * 3 + 2] = info[I_CLO + 2] + (key & AXIS_MAX);
    }
    // the last lane of my segment in this wave holds the segment's totals
    const bool tail = lane == 63 || !((vmask >> (lane + 1)) & 1) || ((heads >> (lane + 1)) & 1);
    if (!tail) return;
    const int cnt = lane - start + 1;
    const bool began = mine != 0;                                                     // its head is in this wave
    const bool ended = lane < 63 || pos + 1 >= n || skeys[pos + 1] != key;            // it does not go on in the next
    if (began && ended) {
        counts[seg] = cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) sums[seg * 3 + a] = s[a];
        first[seg] = rmin;
        if (GROUPS) mask[seg] = (i64)gm;
    } else {
        atomicAdd(counts + seg, cnt);
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicAdd((u64 *)sums + seg * 3 + a, (u64)s[a]);
        atomicMin(first + seg, rmin);
        if (GROUPS) atomicOr((u64 *)mask + seg, gm);
    }
}

// one int32 per wave of 64 sorted rows, then one per tile of SCAN_TPB waves
static i64 n_waves(i64 n) { return (n + 63) / 64; }
static i64 n_tiles(i64 n) { return (n_waves(n) + SCAN_TPB - 1) / SCAN_TPB; }
static size_t ws_bytes(i64 n) { return (size_t)(n_waves(n) + n_tiles(n)) * 4 + 256; }

// inv_a = float32(1 / float64(v_a)); false unless v and inv are finite, positive and normal
static bool lattice(const float *voxel, const float *origin, Lattice &L) {
    for (int a = 0; a < 3; ++a) {
        const float v = voxel[a], o = origin[a];
        if (!(v > 0.f) || !std::isfinite(v) || !std::isfinite(o)) return false;
        const float inv = (float)(1.0 / (double)v);
        if (!std::isfinite(inv) || inv < FLT_MIN) return false;
        L.o[a] = o;
        L.inv[a] = inv;
    }
    return true;
}

}  // namespace pcm_voxel

using namespace pcm_voxel;

extern "C" {

int pcm_voxel_workspace(int64_t n, size_t *bytes) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_voxel_workspace: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_voxel_workspace: n must be below 2^31");
    if (!bytes) return pcm_fail(PCM_E_ARG, "pcm_voxel_workspace: bytes is null");
    *bytes = ws_bytes(n);
    return 0;
}

int pcm_voxel_keys(const float *X, int64_t n, const float *voxel, const float *origin, int64_t *keys, int64_t *info,
                   void *stream) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_voxel_keys: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_voxel_keys: n must be below 2^31");
    if (!voxel || !origin) return pcm_fail(PCM_E_ARG, "pcm_voxel_keys: voxel or origin is null");
    Lattice L;
    if (!lattice(voxel, origin, L))
        return pcm_fail(PCM_E_ARG, "pcm_voxel_keys: voxel sizes must be finite and > 0 with a normal float32 inverse, "
                                   "the origin finite");
    if (!info) return pcm_fail(PCM_E_ARG, "pcm_voxel_keys: info is null");
    if (n > 0 && (!X || !keys)) return pcm_fail(PCM_E_ARG, "pcm_voxel_keys: X or keys is null");
    hipStream_t st = (hipStream_t)stream;
    k_voxel_init<<<1, 64, 0, st>>>((i64 *)info);
    if (n > 0) {
        const i64 blocks = (n + TPB - 1) / TPB;
        k_voxel_bbox<<<(unsigned)std::min<i64>(blocks, 1024), TPB, 0, st>>>(X, n, (i64 *)info);
        k_voxel_plan<<<1, 64, 0, st>>>((i64 *)info, L);
        k_voxel_keys<<<(unsigned)blocks, TPB, 0, st>>>(X, n, (const i64 *)info, L, (i64 *)keys);
    }
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_voxel_keys: ") + hipGetErrorString(e));
    return 0;
}

int pcm_voxel_count(const int64_t *sorted_keys, int64_t n, int64_t *info, void *workspace, size_t workspace_bytes,
                    void *stream) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_voxel_count: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_voxel_count: n must be below 2^31");
    if (n == 0) return 0;   // info[8] is already 0: no device call
    if (!sorted_keys || !info) return pcm_fail(PCM_E_ARG, "pcm_voxel_count: sorted_keys or info is null");
    if (!workspace || workspace_bytes < ws_bytes(n))
        return pcm_fail(PCM_E_ARG, "pcm_voxel_count: workspace too small (pcm_voxel_workspace)");
    hipStream_t st = (hipStream_t)stream;
    const i64 nw = n_waves(n), nt = n_tiles(n);
    int32_t *wave_base = (int32_t *)workspace, *tile_base = wave_base + nw;
    k_voxel_heads<<<(unsigned)((nw + WAVES - 1) / WAVES), TPB, 0, st>>>((const i64 *)sorted_keys, n, wave_base);
    k_voxel_scan_tiles<<<(unsigned)nt, SCAN_TPB, 0, st>>>(wave_base, nw, tile_base);
    k_voxel_scan_top<<<1, SCAN_TPB, 0, st>>>(tile_base, nt, (i64 *)info);
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_voxel_count: ") + hipGetErrorString(e));
    return 0;
}

int pcm_voxel_reduce(const float *X, int64_t n, const uint8_t *groups, int n_groups, const int32_t *q,
                     const int64_t *sorted_keys, const int64_t *perm, int64_t m, int64_t *cells, int32_t *counts,
                     int64_t *sums, int32_t *first, int64_t *day_mask, int32_t *inverse, int64_t *info,
                     const void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: n must be below 2^31");
    if (m < 0 || m > n) return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: m must be in [0, n]");
    if (n_groups < 1 || n_groups > PCM_VOXEL_MAXG)
        return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: n_groups must be 1.." + std::to_string(PCM_VOXEL_MAXG));
    if (n == 0) return 0;   // nothing to reduce: no device call
    if (!X || !q || !sorted_keys || !perm || !inverse || !info)
        return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: X, q, sorted_keys, perm, inverse or info is null");
    if (m > 0 && (!cells || !counts || !sums || !first))
        return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: cells, counts, sums or first is null");
    if ((day_mask && !groups) || (groups && !day_mask && m > 0))
        return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: groups and day_mask go together");
    if (!workspace || workspace_bytes < ws_bytes(n))
        return pcm_fail(PCM_E_ARG, "pcm_voxel_reduce: workspace too small (pcm_voxel_workspace)");
    hipStream_t st = (hipStream_t)stream;
    QExp qe = {{q[0], q[1], q[2]}};
    if (m > 0)
        k_voxel_fill<<<(unsigned)((m + TPB - 1) / TPB), TPB, 0, st>>>(m, counts, (i64 *)sums, first, (i64 *)day_mask);
    const unsigned blocks = (unsigned)((n_waves(n) + WAVES - 1) / WAVES);
    const int32_t *wave_base = (const int32_t *)workspace, *tile_base = wave_base + n_waves(n);
    if (groups && day_mask)
        k_voxel_reduce<true><<<blocks, TPB, 0, st>>>(X, groups, n, (const i64 *)sorted_keys, (const i64 *)perm,
                                                     wave_base, tile_base, qe, m, (i64 *)cells, counts, (i64 *)sums, first,
                                                     (i64 *)day_mask, inverse, (i64 *)info);
    else
        k_voxel_reduce<false><<<blocks, TPB, 0, st>>>(X, nullptr, n, (const i64 *)sorted_keys, (const i64 *)perm,
                                                      wave_base, tile_base, qe, m, (i64 *)cells, counts, (i64 *)sums, first,
                                                      nullptr, inverse, (i64 *)info);
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_voxel_reduce: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
