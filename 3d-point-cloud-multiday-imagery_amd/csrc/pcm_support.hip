// pcm_support.hip — exact fixed-radius neighbour and day-support counts of a cloud (DESIGN.md §4,
// "Support").
//
// Rows are (z, y, x) float32.  Row j is a neighbour of row i (j != i) iff, in float32 with every
// operation rounded and no contraction,
//     dz = z_i - z_j, dy = y_i - y_j, dx = x_i - x_j,   (dz*dz + dy*dy) + dx*dx <= r2 = r*r.
// counts[i] = min(number of neighbours, max_count); days[i] = number of distinct groups among row
// i and its neighbours.  A row with a non-finite coordinate has no neighbours, is nobody's
// neighbour, gets 0 / 0 and is counted in info[PCM_SUPPORT_INFO_SKIPPED].
//
// The predicate alone decides a result; the cells only prune.  A row's cell is, per axis,
// floorf(ldexpf(x, -s)) minus the cell of the bounding box's low corner; s is chosen so that two
// neighbours' cells differ by at most one on every axis (the argument is in DESIGN.md), so every
// neighbour of a row lies in the 27 cells around it.  The key packs (cz, cy, cx), 21 bits each, x
// fastest: the 27 cells are 9 runs of the key-sorted rows.  Any superset of those runs gives the
// same counts, which k_support uses: a wave takes 64 consecutive sorted rows, splits them into
// runs of equal (cz, cy), and for each run scans, for the 9 (dz, dy), the sorted rows whose key
// lies in [(cz+dz, cy+dy, cxmin-1), (cz+dz, cy+dy, cxmax+1)] -- 18 binary searches, one per lane
// of lanes 0..17, once per run.  Candidates are staged through the wave's own LDS in chunks of
// PCM_SUPPORT_CHUNK rows (coalesced 4-byte-lane loads of the sorted planes), and every lane of the
// run tests every staged candidate (a broadcast 16-byte LDS read, 8 float operations).  Count and
// group mask live in registers; there are no atomics in the scan.
//
// Integer results of an exact predicate: the same bits for any row order and any launch shape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "pcm_common.hpp"
#include "pcm_kmeans.h"

namespace pcm_support {

typedef unsigned long long u64;
typedef long long i64;

constexpr int TPB = PCM_SUPPORT_TPB;
constexpr int WAVES = TPB / 64;
constexpr int CHUNK = PCM_SUPPORT_CHUNK;
constexpr int AXIS_BITS = 21;
constexpr i64 AXIS_MAX = ((i64)1 << AXIS_BITS) - 1;
constexpr i64 SKIP_KEY = 0x7fffffffffffffffll;   // sorts behind every cell
constexpr int S_MIN = -32;                       // smallest cell exponent (tiny radii)
constexpr float CELL_ABS_MAX = 1099511627776.f;  // 2^40: |cell| stays exact in int64 arithmetic

static_assert(CHUNK % 64 == 0 && CHUNK >= 64, "a chunk is whole rounds of the wave");
static_assert(TPB % 64 == 0, "whole waves");

// info words (device int64[PCM_SUPPORT_INFO_WORDS]); 9..14 are the box as order-preserving uint32
enum { I_S = 0, I_CLO = 1, I_BITS = 4, I_SKIPPED = 7, I_S0 = 8, I_UMIN = 9, I_UMAX = 12, I_BADPERM = 15 };

__device__ __forceinline__ unsigned enc(float f) {
    const unsigned b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned u) {
    return __uint_as_float((u >> 31) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ float cellf(float x, int s) { return floorf(__builtin_ldexpf(x, -s)); }

__global__ void k_support_init(i64 *info, int s0) {
    const int t = threadIdx.x;
    if (t < PCM_SUPPORT_INFO_WORDS)
        info[t] = t == I_S0 ? (i64)s0 : (t >= I_UMIN && t < I_UMIN + 3) ? (i64)0xffffffffu : 0;
}

// bounding box of the finite rows and the number of the others
__global__ __launch_bounds__(TPB) void k_support_bbox(const float *__restrict__ X, i64 n, i64 *info) {
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
    // one set of atomics per block, not per wave: they all land on the same seven words
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

// one thread: the cell exponent s >= s0 at which the cells are exact integers and every axis
// spans at most 2^21 of them, and the cell of the box's low corner
__global__ void k_support_plan(i64 *info) {
    if (threadIdx.x || blockIdx.x) return;
    int s = (int)info[I_S0];
    i64 clo[3] = {0, 0, 0}, bits[3] = {0, 0, 0};
    if (info[I_UMIN] <= info[I_UMAX]) {   // there is a finite row
        float lo[3], hi[3], m = 0.f;
        for (int a = 0; a < 3; ++a) {
            lo[a] = dec((unsigned)info[I_UMIN + a]);
            hi[a] = dec((unsigned)info[I_UMAX + a]);
            m = fmaxf(m, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
        }
        while (!(__builtin_ldexpf(m, -s) <= CELL_ABS_MAX)) ++s;
        for (;; ++s) {
            bool fits = true;
            for (int a = 0; a < 3; ++a) {
                clo[a] = (i64)cellf(lo[a], s);
                const i64 span = (i64)cellf(hi[a], s) - clo[a] + 1;
                fits = fits && span <= AXIS_MAX + 1;
                bits[a] = span > 1 ? 64 - __clzll(span - 1) : 0;
            }
            if (fits) break;
        }
    }
    info[I_S] = s;
    for (int a = 0; a < 3; ++a) {
        info[I_CLO + a] = clo[a];
        info[I_BITS + a] = bits[a];
    }
}

__global__ __launch_bounds__(TPB) void k_support_keys(const float *__restrict__ X, i64 n, const i64 *__restrict__ info,
                                                      i64 *__restrict__ keys) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int s = (int)info[I_S];
    const float z = X[i * 3], y = X[i * 3 + 1], x = X[i * 3 + 2];
    i64 key = SKIP_KEY;
    if (isfinite(z) && isfinite(y) && isfinite(x)) {
        const i64 cz = (i64)cellf(z, s) - info[I_CLO], cy = (i64)cellf(y, s) - info[I_CLO + 1],
                  cx = (i64)cellf(x, s) - info[I_CLO + 2];
        key = (((cz << AXIS_BITS) | cy) << AXIS_BITS) | cx;   // each in [0, 2^21): k_support_plan
    }
    keys[i] = key;
}

struct Planes {
    float *z, *y, *x;
    int32_t *row;
    uint8_t *g;
};

__host__ __device__ inline Planes planes(void *ws, i64 n) {
    Planes p;
    p.z = (float *)ws;
    p.y = p.z + n;
    p.x = p.y + n;
    p.row = (int32_t *)(p.x + n);
    p.g = (uint8_t *)(p.row + n);
    return p;
}

// the cell-sorted copy: three planes, the row numbers and the group bytes
__global__ __launch_bounds__(TPB) void k_support_gather(const float *__restrict__ X, const uint8_t *__restrict__ groups,
                                                        i64 n, const i64 *__restrict__ perm, void *ws, i64 *info) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const Planes p = planes(ws, n);
    const i64 r = perm[i];
    if (r < 0 || r >= n) {   // not a permutation: nothing is written for this row
        p.z[i] = p.y[i] = p.x[i] = 0.f;
        p.row[i] = -1;
        p.g[i] = 0;
        info[I_BADPERM] = 1;
        return;
    }
    p.z[i] = X[r * 3];
    p.y[i] = X[r * 3 + 1];
    p.x[i] = X[r * 3 + 2];
    p.row[i] = (int32_t)r;
    p.g[i] = groups ? groups[r] : (uint8_t)0;
}

__device__ __forceinline__ i64 lower_bound(const i64 *__restrict__ keys, i64 n, i64 target) {
    i64 lo = 0, hi = n;
    while (lo < hi) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a value every lane holds alike, moved to scalar registers: the loops it bounds become uniform
__device__ __forceinline__ i64 uniform(i64 v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(u64)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
    return (i64)(((u64)hi << 32) | lo);
}

template <bool GROUPS>
__global__ __launch_bounds__(TPB) void k_support(const i64 *__restrict__ skeys, const void *ws, i64 n,
                                                 const i64 *__restrict__ info, float r2, int max_count,
                                                 int32_t *__restrict__ counts, int32_t *__restrict__ days) {
    __shared__ float4 stage[WAVES][CHUNK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float4 *lds = stage[wv];
    const Planes p = planes(const_cast<void *>(ws), n);
    i64 skipped = info[I_SKIPPED];
    skipped = skipped < 0 ? 0 : (skipped > n ? n : skipped);
    const i64 nv = n - skipped;                                   // the finite rows come first
    const i64 w0 = uniform(((i64)blockIdx.x * WAVES + wv) * 64);
    if (w0 >= n) return;
    const i64 me = w0 + lane;
    const bool live = me < nv;
    const i64 key = live ? skeys[me] : (i64)-1;
    const i64 khi = key >> AXIS_BITS;                              // (cz, cy)
    float z = 0.f, y = 0.f, x = 0.f;
    int g = 0;
    if (live) {
        z = p.z[me];
        y = p.y[me];
        x = p.x[me];
        if (GROUPS) g = p.g[me] & 63;
    }
    int cnt = 0;
    u64 mask = 1ull << g;
    const i64 prev = __shfl_up(khi, 1);
    u64 heads = (u64)uniform((i64)__ballot(live && (lane == 0 || khi != prev)));
    const int nlive = __popcll(__ballot(live));
    while (heads) {
        const int f = __ffsll((i64)heads) - 1;
        heads &= heads - 1;
        const int e = heads ? __ffsll((i64)heads) - 1 : nlive;    // the run is lanes [f, e)
        const bool active = lane >= f && lane < e;
        const i64 rhi = __shfl(khi, f);
        const i64 cz = rhi >> AXIS_BITS, cy = rhi & AXIS_MAX;
        const i64 cxmin = __shfl(key, f) & AXIS_MAX, cxmax = __shfl(key, e - 1) & AXIS_MAX;
        // lanes 0..8: where the 9 runs begin; lanes 9..17: where they end
        i64 bound = 0;
        if (lane < 18) {
            const int r = lane % 9;
            const i64 zc = cz + r / 3 - 1, yc = cy + r % 3 - 1;
            if (zc >= 0 && zc <= AXIS_MAX && yc >= 0 && yc <= AXIS_MAX) {
                const i64 cx = lane < 9 ? (cxmin > 0 ? cxmin - 1 : 0) : (cxmax < AXIS_MAX ? cxmax + 1 : AXIS_MAX) + 1;
                bound = lower_bound(skeys, nv, (((zc << AXIS_BITS) | yc) << AXIS_BITS) + cx);
            }
        }
        for (int r = 0; r < 9; ++r) {
            const i64 ra = uniform(__shfl(bound, r)), rb = uniform(__shfl(bound, r + 9));
            for (i64 c0 = ra; c0 < rb; c0 += CHUNK) {
                // without groups a lane is done at max_count: stop when every lane of the run is
                if (!GROUPS && !__ballot(active && cnt < max_count)) break;
                const int m = (int)(rb - c0 < CHUNK ? rb - c0 : CHUNK);
#pragma unroll
                for (int t = lane; t < CHUNK; t += 64) {
                    if (t < m) {
                        const i64 c = c0 + t;                    // < rb <= nv
                        lds[t] = make_float4(p.z[c], p.y[c], p.x[c], GROUPS ? __int_as_float((int)(p.g[c] & 63)) : 0.f);
                    }
                }
                // one wave writes and reads its own LDS, in order: only the compiler needs the fence
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (active) {
                    const int self = (int)(me - c0 >= 0 && me - c0 < m ? me - c0 : -1);
#pragma unroll 4
                    for (int j = 0; j < m; ++j) {
                        const float4 c = lds[j];
                        const float dz = z - c.x, dy = y - c.y, dx = x - c.z;
                        const float d2 = (dz * dz + dy * dy) + dx * dx;
                        if (d2 <= r2 && j != self) {
                            ++cnt;
                            if (GROUPS) mask |= 1ull << __float_as_int(c.w);
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (me < n) {
        const int32_t row = p.row[me];
        if (row >= 0) {
            counts[row] = live ? (cnt < max_count ? cnt : max_count) : 0;
            if (GROUPS) days[row] = live ? __popcll(mask) : 0;
        }
    }
}

// the smallest s with 2^s >= r (1 + 2^-20), not below S_MIN (r: a finite positive float)
static int cell_exponent(float r) {
    int e;
    const double m = std::frexp((double)r * (1.0 + 9.5367431640625e-07), &e);   // m in [0.5, 1)
    const int s = m == 0.5 ? e - 1 : e;
    return s < S_MIN ? S_MIN : s;
}

static bool bad_radius(float r) { return !(r > 0.f) || !std::isfinite(r); }

static int phase_env() {
    if (const char *e = std::getenv("PCM_SUPPORT_PHASE")) {   // measurement: 1 = gather only, 2 = count only
        const int v = std::atoi(e);
        if (v == 1 || v == 2) return v;
    }
    return 0;
}

}  // namespace pcm_support

using namespace pcm_support;

extern "C" {

int pcm_support_workspace(int64_t n, size_t *bytes) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_support_workspace: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_support_workspace: n must be below 2^31");
    if (!bytes) return pcm_fail(PCM_E_ARG, "pcm_support_workspace: bytes is null");
    *bytes = (size_t)n * 17 + 256;   // three float planes, the row numbers, the group bytes
    return 0;
}

int pcm_support_keys(const float *X, int64_t n, float radius, int64_t *keys, int64_t *info, void *stream) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_support_keys: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_support_keys: n must be below 2^31");
    if (bad_radius(radius)) return pcm_fail(PCM_E_ARG, "pcm_support_keys: radius must be finite and > 0 in float32");
    if (!info) return pcm_fail(PCM_E_ARG, "pcm_support_keys: info is null");
    if (n > 0 && (!X || !keys)) return pcm_fail(PCM_E_ARG, "pcm_support_keys: X or keys is null");
    hipStream_t st = (hipStream_t)stream;
    k_support_init<<<1, 64, 0, st>>>((i64 *)info, cell_exponent(radius));
    if (n > 0) {
        const i64 blocks = (n + TPB - 1) / TPB;
        k_support_bbox<<<(unsigned)std::min<i64>(blocks, 1024), TPB, 0, st>>>(X, n, (i64 *)info);
    }
    k_support_plan<<<1, 64, 0, st>>>((i64 *)info);
    if (n > 0) k_support_keys<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, st>>>(X, n, (const i64 *)info, (i64 *)keys);
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_support_keys: ") + hipGetErrorString(e));
    return 0;
}

int pcm_support_count(const float *X, int64_t n, const uint8_t *groups, int n_groups, float radius, int max_count,
                      const int64_t *sorted_keys, const int64_t *perm, int32_t *counts, int32_t *days,
                      int64_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0) return pcm_fail(PCM_E_ARG, "pcm_support_count: n must be >= 0");
    if (n >= (int64_t)1 << 31) return pcm_fail(PCM_E_ARG, "pcm_support_count: n must be below 2^31");
    if (bad_radius(radius)) return pcm_fail(PCM_E_ARG, "pcm_support_count: radius must be finite and > 0 in float32");
    if (n_groups < 1 || n_groups > PCM_SUPPORT_MAXG)
        return pcm_fail(PCM_E_ARG, "pcm_support_count: n_groups must be 1.." + std::to_string(PCM_SUPPORT_MAXG));
    if (n == 0) return 0;   // nothing to count: no device call
    if (!X || !sorted_keys || !perm || !counts || !info)
        return pcm_fail(PCM_E_ARG, "pcm_support_count: X, sorted_keys, perm, counts or info is null");
    if (!workspace || workspace_bytes < (size_t)n * 17 + 256)
        return pcm_fail(PCM_E_ARG, "pcm_support_count: workspace too small (pcm_support_workspace)");
    hipStream_t st = (hipStream_t)stream;
    const int phase = phase_env();
    const float r2 = radius * radius;
    const int maxc = max_count < 0 ? 0x7fffffff : max_count;
    const unsigned blocks = (unsigned)((n + TPB - 1) / TPB);
    if (phase != 2)
        k_support_gather<<<blocks, TPB, 0, st>>>(X, days ? groups : nullptr, n, (const i64 *)perm, workspace,
                                                 (i64 *)info);
    if (phase != 1) {
        if (days) k_support<true><<<blocks, TPB, 0, st>>>((const i64 *)sorted_keys, workspace, n, (const i64 *)info, r2, maxc, counts, days);
        else k_support<false><<<blocks, TPB, 0, st>>>((const i64 *)sorted_keys, workspace, n, (const i64 *)info, r2, maxc, counts, nullptr);
    }
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_support_count: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
