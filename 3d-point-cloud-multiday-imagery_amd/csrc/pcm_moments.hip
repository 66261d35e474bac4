// pcm_moments.hip — exact per-point neighbourhood moments and planes ("Local moments").
//
// Queries X (n rows) and targets Y (m rows) are (z, y, x) float32; Y may be X (Y == NULL).  Target
// j is in the neighbourhood of query i iff both rows are finite and, in float32 with every
// operation rounded and no contraction,
//     dz = X_i.z - Y_j.z, dy = X_i.y - Y_j.y, dx = X_i.x - Y_j.x,   (dz*dz + dy*dy) + dx*dx <= r2 = r*r:
// pcm_nearest.hip's predicate; on one cloud pcm_support.hip's plus the row itself.  With
// yq_a = trunc(ldexp(Y_j.a, q_a)) and xq_a = trunc(ldexp(X_i.a, q_a)) (the engine's fixed_i) and
// dq_a = yq_a - xq_a, a query's ten int64 words are
//     [0] the count   [1..3] sum dq_z, dq_y, dq_x   [4..9] sum dq_a dq_b for zz, zy, zx, yy, yx, xx.
// Integer sums: the same bits for any row order, any sort of equal keys and any launch shape.
// Nothing is checked per pair: the caller's q keeps |dq_a| <= B_a < 2^31 and m B_a B_b <= 2^62
// (the predicate bounds the true gap, truncation moves a scaled coordinate by < 1).
//
// The cells, their keys and the info block are pcm_nearest.hip's (pcm_nearest_keys fills them;
// the small helpers are restated here so that unit stays as it is).  k_moments has k_nearest's
// scan: a wave takes 64 consecutive SORTED queries, splits them into runs of equal (cz, cy), finds
// the 9 target runs of a query run by 18 binary searches on lanes 0..17, and stages the
// candidates through the wave's own LDS in chunks of PCM_MOMENTS_CHUNK rows: a float record
// {z, y, x} for the predicate and an int32 record {zq, yq, xq} for the sums, so fixed_i runs once
// per target (k_moments_gather) and not once per pair.  Every lane of the run reads every staged
// candidate (one address per wave: LDS broadcasts) and adds, selected by the predicate, three
// int32 differences, six 32 x 32 -> 64 multiply-adds and three 64-bit adds.  No atomics and no
// block barrier in the scan.
//
// k_moments_planes turns a row's ten words into a plane, one lane per row in float64: the mean
// offset, the covariance, its eigen-decomposition by cyclic Jacobi, the normal, the roughness,
// the planarity and the signed distance of the query to the plane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "pcm_common.hpp"
#include "pcm_kmeans.h"

namespace pcm_moments {

typedef unsigned long long u64;
typedef long long i64;

constexpr int TPB = PCM_MOMENTS_TPB;
constexpr int WAVES = TPB / 64;
constexpr int CHUNK = PCM_MOMENTS_CHUNK;
constexpr int WORDS = PCM_MOMENTS_WORDS;
constexpr int AXIS_BITS = 21;
constexpr i64 AXIS_MAX = ((i64)1 << AXIS_BITS) - 1;
constexpr int Q_MIN = -126, Q_MAX = 62;
constexpr int SWEEPS = 8;
constexpr double SNAP = 9.313225746154785e-10;   // 2^-30: a normal's component this small counts as 0

static_assert(CHUNK % 64 == 0 && CHUNK >= 64, "a chunk is whole rounds of the wave");
static_assert(TPB % 64 == 0, "whole waves");
static_assert(WORDS == 10, "count, three sums, six products");

// the words of pcm_nearest_keys' info block that this unit reads or sets
enum { I_SKIPPED = 7, I_SKIPPED_T = 8, I_BADPERM = 16 };
static_assert(I_BADPERM < PCM_NEAREST_INFO_WORDS, "the info block holds every word");

struct Q3 {
    int q[3];
};

// trunc(x * 2^q): the engine's fixed_i (pcm_kcommon.hpp)
__device__ __forceinline__ int fixed_i(float x, int q) { return (int)__builtin_ldexpf(x, q); }

struct Planes {
    float *z, *y, *x;
    int32_t *zq, *yq, *xq;
};

__host__ __device__ inline Planes planes(void *ws, i64 m) {
    Planes p;
    p.z = (float *)ws;
    p.y = p.z + m;
    p.x = p.y + m;
    p.zq = (int32_t *)(p.x + m);
    p.yq = p.zq + m;
    p.xq = p.yq + m;
    return p;
}

__host__ inline size_t workspace_bytes(i64 m) { return (size_t)m * 24 + 256; }

// the cell-sorted copy of the targets: three float planes and their three fixed-point planes
__global__ __launch_bounds__(TPB) void k_moments_gather(const float *__restrict__ Y, i64 m, const i64 *__restrict__ perm,
                                                        Q3 qe, void *ws, i64 *info) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const Planes p = planes(ws, m);
    const i64 r = perm[i];
    float z = __uint_as_float(0x7fc00000u), y = z, x = z;
    if (r < 0 || r >= m) {   // not a permutation: this entry can never be in a neighbourhood
        info[I_BADPERM] = 1;
    } else {
        z = Y[r * 3];
        y = Y[r * 3 + 1];
        x = Y[r * 3 + 2];
    }
    const bool fin = isfinite(z) && isfinite(y) && isfinite(x);   // the others sort last and are never scanned
    p.z[i] = z;
    p.y[i] = y;
    p.x[i] = x;
    p.zq[i] = fin ? fixed_i(z, qe.q[0]) : 0;
    p.yq[i] = fin ? fixed_i(y, qe.q[1]) : 0;
    p.xq[i] = fin ? fixed_i(x, qe.q[2]) : 0;
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
// sorted keys and their cell-sorted copy (m).  Queries are read as X[xperm[i]].  skipped_t: the
// info word that counts the non-finite targets (the queries' own when the targets are the queries).
__global__ __launch_bounds__(TPB) void k_moments(const float *__restrict__ X, i64 n, const i64 *__restrict__ xskeys,
                                                 const i64 *__restrict__ xperm, const i64 *__restrict__ yskeys,
                                                 const void *ws, i64 m, i64 *info, int skipped_t, float r2, Q3 qe,
                                                 i64 *__restrict__ words) {
    __shared__ float4 fstage[WAVES][CHUNK];   // {z, y, x, -}
    __shared__ int4 istage[WAVES][CHUNK];     // {zq, yq, xq, -}
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float4 *ldf = fstage[wv];
    int4 *ldi = istage[wv];
    const Planes p = planes(const_cast<void *>(ws), m);
    i64 skq = info[I_SKIPPED], skt = info[skipped_t];
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
    if (live) {
        z = X[row * 3];
        y = X[row * 3 + 1];
        x = X[row * 3 + 2];
    }
    const bool fin = isfinite(z) && isfinite(y) && isfinite(x);   // a live row is finite: its key says so
    const int zq = fin ? fixed_i(z, qe.q[0]) : 0, yq = fin ? fixed_i(y, qe.q[1]) : 0, xq = fin ? fixed_i(x, qe.q[2]) : 0;
    int cnt_in = 0;
    i64 sz = 0, sy = 0, sx = 0, mzz = 0, mzy = 0, mzx = 0, myy = 0, myx = 0, mxx = 0;
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
                        ldf[t] = make_float4(p.z[c], p.y[c], p.x[c], 0.f);
                        ldi[t] = make_int4(p.zq[c], p.yq[c], p.xq[c], 0);
                    }
                }
                // one wave writes and reads its own LDS, in order: only the compiler needs the fence
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (active) {
#pragma unroll 2
                    for (int j = 0; j < cnt; ++j) {
                        const float4 c = ldf[j];
                        const int4 ci = ldi[j];
                        const float dz = z - c.x, dy = y - c.y, dx = x - c.z;
                        const float d2 = (dz * dz + dy * dy) + dx * dx;
                        const bool ok = d2 <= r2;                // false for NaN and for an overflowed +inf
                        // the differences wrap for a pair far apart; such a pair fails and adds 0
                        const int ez = ok ? (int)((unsigned)ci.x - (unsigned)zq) : 0;
                        const int ey = ok ? (int)((unsigned)ci.y - (unsigned)yq) : 0;
                        const int ex = ok ? (int)((unsigned)ci.z - (unsigned)xq) : 0;
                        cnt_in += ok ? 1 : 0;
                        sz += ez;
                        sy += ey;
                        sx += ex;
                        mzz += (i64)ez * ez;
                        mzy += (i64)ez * ey;
                        mzx += (i64)ez * ex;
                        myy += (i64)ey * ey;
                        myx += (i64)ey * ex;
                        mxx += (i64)ex * ex;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (row >= 0) {   // a non-finite query was in no run: ten zeros
        i64 *w = words + row * WORDS;
        w[0] = cnt_in;
        w[1] = sz;
        w[2] = sy;
        w[3] = sx;
        w[4] = mzz;
        w[5] = mzy;
        w[6] = mzx;
        w[7] = myy;
        w[8] = myx;
        w[9] = mxx;
    }
}

// one Jacobi rotation that annihilates a_pq of a symmetric 3 x 3 matrix; r is the third index and
// (vp, vq) the columns p and q of the eigenvector matrix
__device__ __forceinline__ void rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double *vp,
                                       double *vq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    // the smaller root of t^2 + 2 t theta - 1 = 0; an overflowed theta^2 gives t = 0
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double g = arp, h = arq;
    arp = g - s * (h + g * tau);
    arq = h + s * (g - h * tau);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = vp[k], b = vq[k];
        vp[k] = a - s * (b + a * tau);
        vq[k] = b + s * (a - b * tau);
    }
}

__device__ __forceinline__ void order(double &la, double &lb, double *va, double *vb) {
    if (lb < la) {
        const double t = la;
        la = lb;
        lb = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double u = va[k];
            va[k] = vb[k];
            vb[k] = u;
        }
    }
}

// a row's ten words -> its plane, in float64 (every operation rounded, no contraction)
__global__ __launch_bounds__(TPB) void k_moments_planes(const i64 *__restrict__ words, i64 n, Q3 qe, i64 min_count,
                                                        float *__restrict__ normal, float *__restrict__ distance,
                                                        float *__restrict__ roughness, float *__restrict__ planarity) {
    const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const i64 *w = words + i * WORDS;
    const i64 cnt = w[0];
    const float nan = __uint_as_float(0x7fc00000u);
    if (cnt < min_count) {
        normal[i * 3] = normal[i * 3 + 1] = normal[i * 3 + 2] = nan;
        distance[i] = roughness[i] = planarity[i] = nan;
        return;
    }
    const double c = (double)cnt;
    double mu[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) mu[a] = ldexp((double)w[1 + a], -qe.q[a]) / c;
    // C_ab = M_ab 2^-(q_a + q_b) / c - mu_a mu_b
    double azz = ldexp((double)w[4], -2 * qe.q[0]) / c - mu[0] * mu[0];
    double azy = ldexp((double)w[5], -(qe.q[0] + qe.q[1])) / c - mu[0] * mu[1];
    double azx = ldexp((double)w[6], -(qe.q[0] + qe.q[2])) / c - mu[0] * mu[2];
    double ayy = ldexp((double)w[7], -2 * qe.q[1]) / c - mu[1] * mu[1];
    double ayx = ldexp((double)w[8], -(qe.q[1] + qe.q[2])) / c - mu[1] * mu[2];
    double axx = ldexp((double)w[9], -2 * qe.q[2]) / c - mu[2] * mu[2];
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};   // the columns
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        if (azy == 0.0 && azx == 0.0 && ayx == 0.0) break;
        rotate(azz, ayy, azy, azx, ayx, v0, v1);   // (p, q) = (z, y): the third index is x
        rotate(azz, axx, azx, azy, ayx, v0, v2);   // (z, x): y
        rotate(ayy, axx, ayx, azy, azx, v1, v2);   // (y, x): z
    }
    double l0 = azz, l1 = ayy, l2 = axx;
    order(l0, l1, v0, v1);
    order(l1, l2, v1, v2);
    order(l0, l1, v0, v1);                         // l0 <= l1 <= l2
    const double len = sqrt((v0[0] * v0[0] + v0[1] * v0[1]) + v0[2] * v0[2]);
    double nz = v0[0] / len, ny = v0[1] / len, nx = v0[2] / len;
    // a component within SNAP of 0 is 0: rounding noise around an exact 0 (a vertical plane) must not pick the sign
    nz = fabs(nz) <= SNAP ? 0.0 : nz;
    ny = fabs(ny) <= SNAP ? 0.0 : ny;
    nx = fabs(nx) <= SNAP ? 0.0 : nx;
    // surface_elements' sign, branch-free: one factor +-1 for the three components
    const bool flip = nz < 0.0 || (nz == 0.0 && (ny < 0.0 || (ny == 0.0 && nx < 0.0)));
    const double sg = flip ? -1.0 : 1.0;
    nz *= sg;
    ny *= sg;
    nx *= sg;
    normal[i * 3] = (float)nz;
    normal[i * 3 + 1] = (float)ny;
    normal[i * 3 + 2] = (float)nx;
    distance[i] = (float)-((nz * mu[0] + ny * mu[1]) + nx * mu[2]);
    roughness[i] = (float)sqrt(l0 > 0.0 ? l0 : 0.0);
    planarity[i] = l2 > 0.0 ? (float)((l1 - l0) / l2) : 0.f;
}

// the radius and its float32 square must both be finite and > 0 (nearest's rule)
static bool bad_radius(float r) {
    const float r2 = r * r;
    return !(r > 0.f) || !std::isfinite(r) || !(r2 > 0.f) || !std::isfinite(r2);
}

static int phase_env() {
    if (const char *e = std::getenv("PCM_MOMENTS_PHASE")) {   // measurement: 1 = gather only, 2 = scan only
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

static const char *bad_q(const int32_t *q) {
    if (!q) return "q is null";
    for (int a = 0; a < 3; ++a)
        if (q[a] < Q_MIN || q[a] > Q_MAX) return "q must lie in [-126, 62]";
    return nullptr;
}

}  // namespace pcm_moments

using namespace pcm_moments;

extern "C" {

int pcm_moments_workspace(int64_t m, size_t *bytes) {
    if (const char *why = bad_sizes(0, m)) return pcm_fail(PCM_E_ARG, std::string("pcm_moments_workspace: ") + why);
    if (!bytes) return pcm_fail(PCM_E_ARG, "pcm_moments_workspace: bytes is null");
    *bytes = workspace_bytes(m);   // three float planes and three int32 planes
    return 0;
}

int pcm_moments_scan(const float *X, int64_t n, const float *Y, int64_t m, float radius, const int32_t *q,
                     const int64_t *xkeys_sorted, const int64_t *xperm, const int64_t *ykeys_sorted, const int64_t *yperm,
                     int64_t *words, int64_t *info, void *workspace, size_t workspace_bytes_, void *stream) {
    const bool self = Y == nullptr;   // the targets are the queries
    if (self) m = n;
    if (const char *why = bad_sizes(n, m)) return pcm_fail(PCM_E_ARG, std::string("pcm_moments_scan: ") + why);
    if (bad_radius(radius))
        return pcm_fail(PCM_E_ARG, "pcm_moments_scan: radius and its square must be finite and > 0 in float32");
    if (const char *why = bad_q(q)) return pcm_fail(PCM_E_ARG, std::string("pcm_moments_scan: ") + why);
    if (n == 0) return 0;   // no query: no device call
    if (!words) return pcm_fail(PCM_E_ARG, "pcm_moments_scan: words is null");
    hipStream_t st = (hipStream_t)stream;
    if (m == 0) {           // no target: zeros without a scan
        if (hipError_t e = hipMemsetAsync(words, 0, (size_t)n * WORDS * sizeof(int64_t), st))
            return pcm_fail(PCM_E_HIP, std::string("pcm_moments_scan: ") + hipGetErrorString(e));
        return 0;
    }
    if (self) {
        Y = X;
        ykeys_sorted = xkeys_sorted;
        yperm = xperm;
    }
    if (!X || !xkeys_sorted || !xperm || !ykeys_sorted || !yperm || !info)
        return pcm_fail(PCM_E_ARG, "pcm_moments_scan: X, the sorted keys, the permutations or info is null");
    if (!workspace || workspace_bytes_ < workspace_bytes(m))
        return pcm_fail(PCM_E_ARG, "pcm_moments_scan: workspace too small (pcm_moments_workspace)");
    const int phase = phase_env();
    const float r2 = radius * radius;
    const Q3 qe = {{q[0], q[1], q[2]}};
    if (phase != 2)
        k_moments_gather<<<(unsigned)((m + TPB - 1) / TPB), TPB, 0, st>>>(Y, m, (const i64 *)yperm, qe, workspace, (i64 *)info);
    if (phase != 1)
        k_moments<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, st>>>(X, n, (const i64 *)xkeys_sorted, (const i64 *)xperm,
                                                                   (const i64 *)ykeys_sorted, workspace, m, (i64 *)info,
                                                                   self ? I_SKIPPED : I_SKIPPED_T, r2, qe, (i64 *)words);
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_moments_scan: ") + hipGetErrorString(e));
    return 0;
}

int pcm_moments_planes(const int64_t *words, int64_t n, const int32_t *q, int64_t min_count, float *normal, float *distance,
                       float *roughness, float *planarity, void *stream) {
    if (const char *why = bad_sizes(n, 0)) return pcm_fail(PCM_E_ARG, std::string("pcm_moments_planes: ") + why);
    if (const char *why = bad_q(q)) return pcm_fail(PCM_E_ARG, std::string("pcm_moments_planes: ") + why);
    if (min_count < 0) return pcm_fail(PCM_E_ARG, "pcm_moments_planes: min_count must be >= 0");
    if (n == 0) return 0;   // no row: no device call
    if (!words || !normal || !distance || !roughness || !planarity)
        return pcm_fail(PCM_E_ARG, "pcm_moments_planes: words, normal, distance, roughness or planarity is null");
    const Q3 qe = {{q[0], q[1], q[2]}};
    k_moments_planes<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, (hipStream_t)stream>>>(
        (const i64 *)words, n, qe, min_count < 1 ? 1 : min_count, normal, distance, roughness, planarity);
    if (hipError_t e = hipGetLastError()) return pcm_fail(PCM_E_HIP, std::string("pcm_moments_planes: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
