// pcm_nearest.hip — exact nearest row of another cloud within a radius ("Nearest").
//
// Queries X (n rows) and targets Y (m rows) are (z, y, x) float32; X and Y may be one array.
// Target j is a candidate of query i iff both rows are finite, their groups (when given) differ
// and, in float32 with every operation rounded and no contraction,
//     dz = X_i.z - Y_j.z, dy = X_i.y - Y_j.y, dx = X_i.x - Y_j.x,   d2 = (dz*dz + dy*dy) + dx*dx <= r2 = r*r.
// index[i] is the candidate that minimises (d2, j) lexicographically -- a tie in distance goes to
// the LOWEST target row --, or -1; sqdist[i] is that d2, or +inf.  A non-finite query gets
// -1 / +inf and is counted in info[7]; a non-finite target is never a candidate (info[8]).
//
// The predicate and the tie rule alone decide a result; the cells only prune.  They are
// pcm_support.hip's cells (its small helpers are restated here so that unit stays as it is),
// taken over the box of BOTH clouds: one exponent s and one low corner, so a query's and a
// target's cells compare.  s is chosen so that the cells of two rows that satisfy the predicate
// differ by at most one on every axis (the argument is about two points, whichever
// cloud each belongs to), so every candidate of a query lies in the 27 cells around it: 9 runs of
// the key-sorted targets.  A wave takes 64 consecutive SORTED queries, splits them into runs of
// equal (cz, cy), and for each run scans, for the 9 (dz, dy), the sorted targets whose key lies in
// [(cz+dz, cy+dy, cxmin-1), (cz+dz, cy+dy, cxmax+1)] -- 18 binary searches, one per lane of lanes
// 0..17, once per run.  Candidates are staged through the wave's own LDS in chunks of
// PCM_NEAREST_CHUNK rows as 16-byte records {z, y, x, row} (with groups: a 4-byte plane beside
// them), and every lane of the run tests every staged candidate.  The running best is ONE 64-bit
// word per lane, (bits of d2) << 32 | row, kept by an unsigned minimum: d2 is a sum of squares of
// finite differences, never NaN and never -0, so its bits order as its value, and the low half
// breaks a tie towards the lowest row.  No atomics in the scan.
//
// An integer and a float32 decided by one predicate and one total order: the same bits for any
// row order, any sort of equal keys and any launch shape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "pcm_common.hpp"
#include "pcm_kmeans.h"

namespace pcm_nearest {

typedef unsigned long long u64;
typedef long long i64;

constexpr int TPB = PCM_NEAREST_TPB;
constexpr int WAVES = TPB / 64;
constexpr int CHUNK = PCM_NEAREST_CHUNK;
constexpr int AXIS_BITS = 21;
constexpr i64 AXIS_MAX = ((i64)1 << AXIS_BITS) - 1;
constexpr i64 SKIP_KEY = 0x7fffffffffffffffll;   // sorts behind every cell
constexpr int S_MIN = -32;                       // smallest cell exponent (tiny radii)
constexpr float CELL_ABS_MAX = 1099511627776.f;  // 2^40: |cell| stays exact in int64 arithmetic
constexpr u64 NONE = ~0ull;                      // no candidate yet: above every (d2, row) word

static_assert(CHUNK % 64 == 0 && CHUNK >= 64, "a chunk is whole rounds of the wave");
static_assert(TPB % 64 == 0, "whole waves");

// info words (device int64[PCM_NEAREST_INFO_WORDS]); 10..15 are the box as order-preserving uint32
enum { I_S = 0, I_CLO = 1, I_BITS = 4, I_SKIPPED = 7, I_SKIPPED_T = 8, I_S0 = 9, I_UMIN = 10, I_UMAX = 13, I_BADPERM = 16 };
static_assert(I_BADPERM < PCM_NEAREST_INFO_WORDS, "the info block holds every word");

__device__ __forceinline__ unsigned enc(float f) {
    const unsigned b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned u) {
    return __uint_as_float((u >> 31) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ float cellf(float x, int s) { return floorf(__builtin_ldexpf(x, -s)); }

__global__ void k_nearest_init(i64 *info, int s0) {
    const int t = threadIdx.x;
    if (t < PCM_NEAREST_INFO_WORDS)
        info[t] = t == I_S0 ? (i64)s0 : (t >= I_UMIN && t < I_UMIN + 3) ? (i64)0xffffffffu : 0;
}

// the box of the finite rows of one cloud, merged into the common box, and the number of the others
__global__ __launch_bounds__(TPB) void k_nearest_bbox(const float *__restrict__ X, i64 n, i64 *info, int skipped_word) {
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
        else if (v) atomicAdd((u64 *)info + skipped_word, (u64)v);
    }
}

// one thread: the cell exponent s >= s0 at which the cells are exact integers and every axis
// spans at most 2^21 of them, and the cell of the box's low corner
__global__ void k_nearest_plan(i64 *info) {
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

__global__ __launch_bounds__(TPB) void k_nearest_keys(const float *__restrict__ X, i64 n, const i64 *__restrict__ info,
                                                      i64 *__restrict__ keys) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int s = (int)info[I_S];
    const float z = X[i * 3], y = X[i * 3 + 1], x = X[i * 3 + 2];
    i64 key = SKIP_KEY;
    if (isfinite(z) && isfinite(y) && isfinite(x)) {
        const i64 cz = (i64)cellf(z, s) - info[I_CLO], cy = (i64)cellf(y, s) - info[I_CLO + 1],
                  cx = (i64)cellf(x, s) - info[I_CLO + 2];
        key = (((cz << AXIS_BITS) | cy) << AXIS_BITS) | cx;   // each in [0, 2^21): k_nearest_plan
    }
    keys[i] = key;
}

struct Planes {
    float *z, *y, *x;
    int32_t *row, *g;
};

__host__ __device__ inline Planes planes(void *ws, i64 m) {
    Planes p;
    p.z = (float *)ws;
    p.y = p.z + m;
    p.x = p.y + m;
    p.row = (int32_t *)(p.x + m);
    p.g = p.row + m;
    return p;
}

__host__ inline size_t workspace_bytes(i64 m) { return (size_t)m * 20 + 256; }

// the cell-sorted copy of the targets: three planes, the row numbers and the int32 groups
__global__ __launch_bounds__(TPB) void k_nearest_gather(const float *__restrict__ Y, const int32_t *__restrict__ groups,
                                                        i64 m, const i64 *__restrict__ perm, void *ws, i64 *info) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const Planes p = planes(ws, m);
    const i64 r = perm[i];
    if (r < 0 || r >= m) {   // not a permutation: this entry can never be a candidate
        p.z[i] = p.y[i] = p.x[i] = __uint_as_float(0x7fc00000u);
        p.row[i] = -1;
        p.g[i] = 0;
        info[I_BADPERM] = 1;
        return;
    }
    p.z[i] = Y[r * 3];
    p.y[i] = Y[r * 3 + 1];
    p.x[i] = Y[r * 3 + 2];
    p.row[i] = (int32_t)r;
    p.g[i] = groups ? groups[r] : 0;
}

// no target at all: every query is without a candidate
__global__ __launch_bounds__(TPB) void k_nearest_none(i64 n, int32_t *__restrict__ index, float *__restrict__ sqdist) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    index[i] = -1;
    sqdist[i] = __uint_as_float(0x7f800000u);
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

// xskeys / xperm: the queries' sorted keys and their row numbers (n); yskeys / ws: the targets'
// sorted keys and their cell-sorted copy (m).  Queries are read as X[xperm[i]].
template <bool GROUPS>
__global__ __launch_bounds__(TPB) void k_nearest(const float *__restrict__ X, const int32_t *__restrict__ xgroups, i64 n,
                                                 const i64 *__restrict__ xskeys, const i64 *__restrict__ xperm,
                                                 const i64 *__restrict__ yskeys, const void *ws, i64 m, i64 *info,
                                                 float r2, int32_t *__restrict__ index, float *__restrict__ sqdist) {
    __shared__ float4 stage[WAVES][CHUNK];
    __shared__ int gstage[GROUPS ? WAVES : 1][GROUPS ? CHUNK : 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float4 *lds = stage[wv];
    int *ldg = gstage[GROUPS ? wv : 0];
    const Planes p = planes(const_cast<void *>(ws), m);
    i64 skq = info[I_SKIPPED], skt = info[I_SKIPPED_T];
    skq = skq < 0 ? 0 : (skq > n ? n : skq);
    skt = skt < 0 ? 0 : (skt > m ? m : skt);
    const i64 nvq = n - skq, nvt = m - skt;                        // the finite rows come first
    const i64 w0 = uniform(((i64)blockIdx.x * WAVES + wv) * 64);
    if (w0 >= n) return;
    const i64 me = w0 + lane;
    i64 row = -1;                                                  // the query's row in the caller's order
    if (me < n) {
        row = xperm[me];
        if (row < 0 || row >= n) {   // not a permutation: nothing is read or written for this entry
            row = -1;
            info[I_BADPERM] = 1;
        }
    }
    const bool live = me < nvq && row >= 0;
    const i64 key = live ? xskeys[me] : (i64)-1;
    const i64 khi = key >> AXIS_BITS;                              // (cz, cy)
    float z = 0.f, y = 0.f, x = 0.f;
    int g = 0;
    if (live) {
        z = X[row * 3];
        y = X[row * 3 + 1];
        x = X[row * 3 + 2];
        if (GROUPS) g = xgroups[row];
    }
    u64 best = NONE;
    const i64 prev = __shfl_up(khi, 1);
    const bool prev_live = __shfl_up((int)live, 1) != 0;
    u64 heads = (u64)uniform((i64)__ballot(live && (lane == 0 || !prev_live || khi != prev)));
    const u64 lives = (u64)uniform((i64)__ballot(live));
    while (heads) {
        const int f = __ffsll((i64)heads) - 1;
        heads &= heads - 1;
        // the run is the live lanes of [f, e): a lane whose permutation entry was bad is in no run
        const int e = heads ? __ffsll((i64)heads) - 1 : 64;
        const u64 span = (e < 64 ? (1ull << e) - 1 : ~0ull) & ~((1ull << f) - 1) & lives;
        const int last = 63 - __clzll(span);                       // bit f is set: the head is live
        const bool active = (span >> lane) & 1;
        const i64 rhi = __shfl(khi, f);
        const i64 cz = rhi >> AXIS_BITS, cy = rhi & AXIS_MAX;
        const i64 cxmin = __shfl(key, f) & AXIS_MAX, cxmax = __shfl(key, last) & AXIS_MAX;
        // lanes 0..8: where the 9 runs begin; lanes 9..17: where they end
        i64 bound = 0;
        if (lane < 18) {
            const int r = lane % 9;
            const i64 zc = cz + r / 3 - 1, yc = cy + r % 3 - 1;
            if (zc >= 0 && zc <= AXIS_MAX && yc >= 0 && yc <= AXIS_MAX) {
                const i64 cx = lane < 9 ? (cxmin > 0 ? cxmin - 1 : 0) : (cxmax < AXIS_MAX ? cxmax + 1 : AXIS_MAX) + 1;
                bound = lower_bound(yskeys, nvt, (((zc << AXIS_BITS) | yc) << AXIS_BITS) + cx);
            }
        }
        for (int r = 0; r < 9; ++r) {
            const i64 ra = uniform(__shfl(bound, r)), rb = uniform(__shfl(bound, r + 9));
            for (i64 c0 = ra; c0 < rb; c0 += CHUNK) {
                const int cnt = (int)(rb - c0 < CHUNK ? rb - c0 : CHUNK);
#pragma unroll
                for (int t = lane; t < CHUNK; t += 64) {
                    if (t < cnt) {
                        const i64 c = c0 + t;                    // < rb <= nvt <= m
                        lds[t] = make_float4(p.z[c], p.y[c], p.x[c], __int_as_float(p.row[c]));
                        if (GROUPS) ldg[t] = p.g[c];
                    }
                }
                // one wave writes and reads its own LDS, in order: only the compiler needs the fence
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (active) {
#pragma unroll 4
                    for (int j = 0; j < cnt; ++j) {
                        const float4 c = lds[j];
                        const float dz = z - c.x, dy = y - c.y, dx = x - c.z;
                        const float d2 = (dz * dz + dy * dy) + dx * dx;
                        bool ok = d2 <= r2;                      // false for NaN and for an overflowed +inf
                        if (GROUPS) ok = ok && ldg[j] != g;
                        const u64 cand = ((u64)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(c.w);
                        best = ok && cand < best ? cand : best;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (row >= 0) {
        const bool found = best != NONE;
        index[row] = found ? (int32_t)(unsigned)best : -1;
        sqdist[row] = __uint_as_float(found ? (unsigned)(best >> 32) : 0x7f800000u);
    }
}

// the smallest s with 2^s >= r (1 + 2^-20), not below S_MIN (r: a finite positive float)
static int cell_exponent(float r) {
    int e;
    const double m = std::frexp((double)r * (1.0 + 9.5367431640625e-07), &e);   // m in [0.5, 1)
    const int s = m == 0.5 ? e - 1 : e;
    return s < S_MIN ? S_MIN : s;
}

// the radius and its float32 square must both be finite and > 0: +inf is left to mean "none"
static bool bad_radius(float r) {
    const float r2 = r * r;
    return !(r > 0.f) || !std::isfinite(r) || !(r2 > 0.f) || !std::isfinite(r2);
}

static int phase_env() {
    if (const char *e = std::getenv("PCM_NEAREST_PHASE")) {   // measurement: 1 = gather only, 2 = scan only
        const int v = std::atoi(e);
        if (v == 1 || v == 2) return v;
    }
    return 0;
}

static const char *bad_sizes(int64_t n, int64_t m) {
    if (n < 0 || m < 0) return "n and m must be >= 0";
    if (n >= (int64_t)1 << 31 || m >= (int64_t)1 << 31) return "n and m must be below 2^31";
    return nullptr;
}

}  // namespace pcm_nearest

using namespace pcm_nearest;

extern "C" {

int pcm_nearest_workspace(int64_t m, size_t *bytes) {
    if (const char *why = bad_sizes(0, m)) return pcm_fail(PCM_E_ARG, std::string("pcm_nearest_workspace: ") + why);
    if (!bytes) return pcm_fail(PCM_E_ARG, "pcm_nearest_workspace: bytes is null");
    *bytes = workspace_bytes(m);   // three float planes, the row numbers, the int32 groups
    return 0;
}

int pcm_nearest_keys(const float *X, int64_t n, const float *Y, int64_t m, float radius, int64_t *xkeys, int64_t *ykeys,
                     int64_t *info, void *stream) {
    if (const char *why = bad_sizes(n, m)) return pcm_fail(PCM_E_ARG, std::string("pcm_nearest_keys: ") + why);
    if (bad_radius(radius))
        return pcm_fail(PCM_E_ARG, "pcm_nearest_keys: radius and its square must be finite and > 0 in float32");
    if (!info) return pcm_fail(PCM_E_ARG, "pcm_nearest_keys: info is null");
    if ((n > 0 && (!X || !xkeys)) || (m > 0 && (!Y || !ykeys)))
        return pcm_fail(PCM_E_ARG, "pcm_nearest_keys: X, Y, xkeys or ykeys is null");
    hipStream_t st = (hipStream_t)stream;
    const auto blocks = [](i64 rows) { return (unsigned)((rows + TPB - 1) / TPB); };
    k_nearest_init<<<1, 64, 0, st>>>((i64 *)info, cell_exponent(radius));
    if (n > 0) k_nearest_bbox<<<std::min(blocks(n), 1024u), TPB, 0, st>>>(X, n, (i64 *)info, I_SKIPPED);
    if (m > 0) k_nearest_bbox<<<std::min(blocks(m), 1024u), TPB, 0, st>>>(Y, m, (i64 *)info, I_SKIPPED_T);
    k_nearest_plan<<<1, 64, 0, st>>>((i64 *)info);
    if (n > 0) k_nearest_keys<<<blocks(n), TPB, 0, st>>>(X, n, (const i64 *)info, (i64 *)xkeys);
    if (m > 0) k_nearest_keys<<<blocks(m), TPB, 0, st>>>(Y, m, (const i64 *)info, (i64 *)ykeys);
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_nearest_keys: ") + hipGetErrorString(e));
    return 0;
}

int pcm_nearest_find(const float *X, int64_t n, const float *Y, int64_t m, const int32_t *groups,
                     const int32_t *target_groups, float radius, const int64_t *xkeys_sorted, const int64_t *xperm,
                     const int64_t *ykeys_sorted, const int64_t *yperm, int32_t *index, float *sqdist, int64_t *info,
                     void *workspace, size_t workspace_bytes_, void *stream) {
    if (const char *why = bad_sizes(n, m)) return pcm_fail(PCM_E_ARG, std::string("pcm_nearest_find: ") + why);
    if (bad_radius(radius))
        return pcm_fail(PCM_E_ARG, "pcm_nearest_find: radius and its square must be finite and > 0 in float32");
    if ((groups == nullptr) != (target_groups == nullptr) && n > 0 && m > 0)
        return pcm_fail(PCM_E_ARG, "pcm_nearest_find: groups and target_groups go together");
    if (n == 0) return 0;   // no query: no device call
    if (!index || !sqdist) return pcm_fail(PCM_E_ARG, "pcm_nearest_find: index or sqdist is null");
    hipStream_t st = (hipStream_t)stream;
    const unsigned qblocks = (unsigned)((n + TPB - 1) / TPB);
    if (m == 0) {           // no target: no scan
        k_nearest_none<<<qblocks, TPB, 0, st>>>(n, index, sqdist);
        if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_nearest_find: ") + hipGetErrorString(e));
        return 0;
    }
    if (!X || !Y || !xkeys_sorted || !xperm || !ykeys_sorted || !yperm || !info)
        return pcm_fail(PCM_E_ARG, "pcm_nearest_find: X, Y, the sorted keys, the permutations or info is null");
    if (!workspace || workspace_bytes_ < workspace_bytes(m))
        return pcm_fail(PCM_E_ARG, "pcm_nearest_find: workspace too small (pcm_nearest_workspace)");
    const int phase = phase_env();
    const float r2 = radius * radius;
    if (phase != 2)
        k_nearest_gather<<<(unsigned)((m + TPB - 1) / TPB), TPB, 0, st>>>(Y, target_groups, m, (const i64 *)yperm, workspace,
                                                                           (i64 *)info);
    if (phase != 1) {
        if (groups)
            k_nearest<true><<<qblocks, TPB, 0, st>>>(X, groups, n, (const i64 *)xkeys_sorted, (const i64 *)xperm,
                                                     (const i64 *)ykeys_sorted, workspace, m, (i64 *)info, r2, index, sqdist);
        else
            k_nearest<false><<<qblocks, TPB, 0, st>>>(X, nullptr, n, (const i64 *)xkeys_sorted, (const i64 *)xperm,
                                                      (const i64 *)ykeys_sorted, workspace, m, (i64 *)info, r2, index, sqdist);
    }
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_nearest_find: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
