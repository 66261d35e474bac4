// pcm_layout.hpp (a part of pcm_kernels.hpp) — layout kernels (once per cloud): bbox, sort key, tiles, compression, tile lists
#pragma once
#include "pcm_kcommon.hpp"

namespace pcm {

// Up to 5 buffers of 64-bit words := 0 in one launch (pcm_fit_begin).
struct ZeroSpans {
    unsigned long long *p[4];
    long long n[4];
};
inline __global__ __launch_bounds__(256) void k_zero_spans(ZeroSpans z) {
    const long long st = (long long)gridDim.x * blockDim.x;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < z.n[q]; i += st) z.p[q][i] = 0ull;
}

// ------------------------------------------------------------------ layout
// Per-block min/max/maxabs (+ non-finite flag) of an AoS (n, D) array.
template <typename T, int D>
__global__ __launch_bounds__(256) void k_bbox_partial(const T *__restrict__ X, long long n, float *__restrict__ part,
                                                      unsigned *__restrict__ nonfinite) {
    float mn[D], mx[D];
    for (int a = 0; a < D; ++a) { mn[a] = __builtin_inff(); mx[a] = -__builtin_inff(); }
    bool bad = false;
    const long long st = (long long)gridDim.x * blockDim.x;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    for (; i + 3 * st < n; i += 4 * st) {   // 4 rows' loads in flight per round
        float v[4][D];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < D; ++a) v[u][a] = to_f<T>(X[(i + u * st) * D + a]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < D; ++a) {
                bad |= !__builtin_isfinite(v[u][a]);
                mn[a] = fminf(mn[a], v[u][a]);
                mx[a] = fmaxf(mx[a], v[u][a]);
            }
    }
    for (; i < n; i += st) {
        for (int a = 0; a < D; ++a) {
            float v = to_f<T>(X[i * D + a]);
            bad |= !__builtin_isfinite(v);
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
    }
    __shared__ float smn[D][256], smx[D][256];
    for (int a = 0; a < D; ++a) { smn[a][threadIdx.x] = mn[a]; smx[a][threadIdx.x] = mx[a]; }
    if (bad) atomicOr(nonfinite, 1u);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < D; ++a) {
                smn[a][threadIdx.x] = fminf(smn[a][threadIdx.x], smn[a][threadIdx.x + s]);
                smx[a][threadIdx.x] = fmaxf(smx[a][threadIdx.x], smx[a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int a = 0; a < D; ++a) {
            part[(size_t)blockIdx.x * 2 * D + a] = smn[a][0];
            part[(size_t)blockIdx.x * 2 * D + D + a] = smx[a][0];
        }
}

template <int D>
__global__ __launch_bounds__(256) void k_bbox_final(const float *__restrict__ part, int nblk, double *__restrict__ out) {
    // out: lo[D], hi[D]; one block, strided per-thread pass then an LDS tree
    __shared__ float smn[D][256], smx[D][256];
    const int tid = threadIdx.x;
    for (int a = 0; a < D; ++a) {
        float mn = __builtin_inff(), mx = -__builtin_inff();
        for (int b = tid; b < nblk; b += 256) {
            mn = fminf(mn, part[(size_t)b * 2 * D + a]);
            mx = fmaxf(mx, part[(size_t)b * 2 * D + D + a]);
        }
        smn[a][tid] = mn;
        smx[a][tid] = mx;
    }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st)
            for (int a = 0; a < D; ++a) {
                smn[a][tid] = fminf(smn[a][tid], smn[a][tid + st]);
                smx[a][tid] = fmaxf(smx[a][tid], smx[a][tid + st]);
            }
        __syncthreads();
    }
    if (tid == 0)
        for (int a = 0; a < D; ++a) {
            out[a] = smn[a][0];
            out[D + a] = smx[a][0];
        }
}

// Sort key of the Lloyd layout: the cell id << D | the sub-cell (bit D-1-a set
// when the point lies in the upper half of its cell along axis a), so that
// within a cell the points of one sub-cell are contiguous.  The half test uses
// the same fp64 cell coordinate as the binning (clamped cells: a point on the
// top face lands in the upper half); sub-cell boxes carry the binning margin on
// both sides of the split (k_lloyd1).  Crowded layouts (zlev > 0) instead append
// a Morton code of zlev bisections of the cell (level 1 = the sub-cell bits,
// then the next finer halves, axis 0 first within a level), so the tiles of a
// crowded cell are compact boxes (tile lists, k_tile_cand).
template <int D>
__device__ __forceinline__ uint32_t sort_key_f(const float (&x)[D], const Grid &g, int with_sub, int zlev) {
    int idx[MAXD];
    uint32_t sub = 0, fz[MAXD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double t = ((double)x[a] - g.lo[a]) * g.inv[a];
        int v = (int)floor(t);
        v = v < 0 ? 0 : (v >= g.G[a] ? g.G[a] - 1 : v);
        idx[a] = v;
        const double fr = t - (double)v;
        sub = (sub << 1) | ((fr >= 0.5) ? 1u : 0u);
        fz[a] = 0u;
        if (zlev > 0) {
            const int top = (1 << zlev) - 1;
            int m = (int)floor(fr * (double)(1 << zlev));
            fz[a] = (uint32_t)(m < 0 ? 0 : (m > top ? top : m));
        }
    }
    const uint32_t cell = (uint32_t)encode(idx, g.G, D);
    if (zlev > 0) {
        uint32_t z = 0;
        for (int l = zlev - 1; l >= 0; --l)
#pragma unroll
            for (int a = 0; a < D; ++a) z = (z << 1) | ((fz[a] >> l) & 1u);
        return (cell << (D * zlev)) | z;
    }
    return with_sub ? (cell << D) | sub : cell;
}

// Point record carried through the layout sort (coordinates + caller row), so
// that the sort itself moves the points and no random row gather follows.
template <typename T, int D> struct PRec {
    T c[D];
    uint32_t row;
};

// cell_start[c] = sub_start[c << d], c in [0, ncells]
inline __global__ __launch_bounds__(256) void k_cell_from_sub(const uint32_t *__restrict__ sub_start, long long ncells, int d,
                                                       uint32_t *__restrict__ cell_start) {
    long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c <= ncells) cell_start[c] = sub_start[c << d];
}

// Sorted point layout "AoSoA-4": the points in cell order, in groups of 4
// consecutive points stored coordinate-major -- [x0 x1 x2 x3][y0 .. y3][z0 .. z3]
// -- so one lane's 4 points arrive from b128 loads already paired for the
// packed (v_pk_*) distance arithmetic, with no register shuffling.
template <int D>
__device__ __forceinline__ long long xs_index(long long i, int a) {
    return ((i >> 2) * D + a) * 4 + (i & 3);
}

inline __global__ __launch_bounds__(256) void k_tile_counts(const uint32_t *__restrict__ start, long long ncells,
                                                     uint32_t *__restrict__ cnt, uint32_t cap) {
    long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    uint32_t n = start[c + 1] - start[c];
    cnt[c] = (n + cap - 1) / cap;
}

// tile_off[nc] and the tile count (the scan is exclusive: add the last cell's count)
inline __global__ void k_tile_total(uint32_t *__restrict__ off, const uint32_t *__restrict__ cnt, long long ncells,
                             uint32_t *__restrict__ ntiles) {
    if (threadIdx.x != 0) return;
    const uint32_t t = off[ncells - 1] + cnt[ncells - 1];
    off[ncells] = t;
    *ntiles = t;
}

inline __global__ __launch_bounds__(256) void k_tile_write(const uint32_t *__restrict__ start, const uint32_t *__restrict__ off,
                                                    long long ncells, uint4 *__restrict__ tiles, uint32_t cap) {
    long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    uint32_t s = start[c], e = start[c + 1];
    uint32_t n = e - s;
    if (n == 0) return;
    uint32_t nt = (n + cap - 1) / cap;
    uint32_t per = (n + nt - 1) / nt;
    uint32_t o = off[c];
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t a = s + t * per;
        uint32_t b = a + per < e ? a + per : e;
        tiles[o + t] = make_uint4((uint32_t)c, a, b, 0u);
    }
}

// Longest-list-first tile order (pcm_fit_begin): key = 0xffff - the list
// length of the tile's cell at the first lists (FULL: the longest), value = the
// tile; a stable radix sort, then the records gathered in that order.
inline __global__ __launch_bounds__(256) void k_tile_lpt_keys(const uint4 *__restrict__ tiles, const uint32_t *__restrict__ fc_cnt,
                                                       unsigned nt, uint32_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nt) return;
    const uint32_t c = fc_cnt[tiles[t].x];
    key[t] = 0xffffu - (c == FULL ? 0xffffu : min(c, 0xfffeu));
    idx[t] = t;
}

// The per-tile sums `tsum` ([tile][d] int64, k_tile_compress / k_tile_sums) move
// with their tiles, and the list builders' map from a tile's layout-time index
// (tile_off[cell] + i) to its current position is kept: torig (position ->
// layout index; null = identity, the first reorder of a layout) is permuted,
// tpos (its inverse) rewritten.
inline __global__ __launch_bounds__(256) void k_tile_gather(const uint4 *__restrict__ tiles, const uint4 *__restrict__ tmeta,
                                                     const uint32_t *__restrict__ idx, unsigned nt,
                                                     uint4 *__restrict__ t2, uint4 *__restrict__ m2,
                                                     const long long *__restrict__ tsum, long long *__restrict__ s2, int d,
                                                     const uint32_t *__restrict__ torig, uint32_t *__restrict__ o2,
                                                     uint32_t *__restrict__ tpos) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nt) return;
    const uint32_t j = idx[t];
    t2[t] = tiles[j];
    if (tmeta) m2[t] = tmeta[j];
    for (int a = 0; a < d; ++a) s2[(size_t)t * d + a] = tsum[(size_t)j * d + a];
    const uint32_t o = torig ? torig[j] : j;
    o2[t] = o;
    tpos[o] = t;
}

// Compressed point stream (fp32, D = 3).  Inside one tile (one cell, <= TILE
// points) each axis spans a short range, so every coordinate's fp32 bit pattern
// is the tile's minimum pattern on that axis plus a small unsigned delta (the
// patterns of same-signed floats are ordered by magnitude).  When every axis is
// single-signed over the tile and the three delta widths sum to <= 64 bits, the
// tile's points are stored as 8-byte records d0 | d1 << w0 | d2 << (w0 + w1) in
// `xz` (lo and hi words, zword() below); k_lloyd1 then streams 8 instead of 12 bytes per point and
// rebuilds the EXACT fp32 values (lossless: labels and sums are unchanged).
// tmeta[t] = {min0, min1, min2, 1 << 31 | w0 | w1 << 8 | w2 << 16}, or .w = 0
// (raw tile: 12-B AoSoA-4 `xs`).  Uniform [0,1)^3 cloud with 32^3 cells: cells
// with an axis index >= 1 need <= 23 + 21 + 20 bits; ~91 % of the points.
__device__ __forceinline__ unsigned zwidth(unsigned span) { return span ? 32u - (unsigned)__clz(span) : 0u; }

// Word offset in `xz` of the lo word of point i (its hi word: + ZHI): blocks
// of 256 points, 1 KB of lo words then 1 KB of hi words, each
// group of 4 points' words 16 B at (i % 256) / 4 -- a wave's 64 lanes x 4 points
// load 2 x 1 KB of consecutive bytes (two b128 per lane, each instruction one
// contiguous run).  (The per-group layout [lo0..lo3][hi0..hi3], 32 B per lane so
// that each b128 instruction reads every other 16 B, was no faster: profiles/rd4_zwave_ab.txt.)
// Record fields: x = bits [0, w0), y = [w0, w0 + w1), z = the top w2 bits (x by
// a mask, y by one funnel shift of the two words, z by one shift of the high
// word: 7 VALU per point; z after y took two 64-bit shifts, ~11 VALU, and
// measured ~1.5 % slower per k_lloyd1 launch at config 3, profiles/rd4_ztop_ab.txt).
constexpr unsigned ZHI = 256;
__host__ __device__ __forceinline__ size_t zword(size_t i) { return (i >> 8) * 512u + (i & 255u); }

inline __global__ __launch_bounds__(256) void k_tile_compress(const float *__restrict__ xs, const uint4 *__restrict__ tiles,
                                                       const uint32_t *__restrict__ ntiles, uint4 *__restrict__ tmeta,
                                                       unsigned *__restrict__ xz, unsigned long long *__restrict__ zpts,
                                                       QExp qe, long long *__restrict__ tsum) {
    const unsigned t = blockIdx.x;
    if (t >= *ntiles) return;
    const uint4 tr = tiles[t];
    const unsigned start = tr.y, end = tr.z;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the whole tile (<= TILE = 16 x 256 points) in registers: every load in
    // flight at once, one read of xs (a strided loop waited one latency per
    // round, twice: 505-530 us for 100M points).  Round 6: a thread takes whole
    // AoSoA-4 groups -- 4 consecutive points, three 16-B loads (x4, y4, z4) --
    // instead of one coordinate word per point and axis (4-B loads at a 12-B
    // lane stride), and writes a full group's records as two 16-B stores
    constexpr int GPT = TILE / 1024 + 1;   // groups per thread (a tile spans <= TILE / 4 + 1 groups)
    const unsigned g0 = start >> 2, g1 = (end + 3u) >> 2;
    const float4 *xs4 = reinterpret_cast<const float4 *>(xs);
    float4 q[GPT][3];
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
        const unsigned gg = g0 + (unsigned)tid + 256u * u;
        if (gg < g1) {
#pragma unroll
            for (int a = 0; a < 3; ++a) q[u][a] = xs4[(size_t)gg * 3 + a];
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) q[u][a] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    auto word = [&](int u, int a, int k) -> unsigned {
        const float4 &v = q[u][a];
        return __float_as_uint(k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)));
    };
    unsigned mn[3] = {~0u, ~0u, ~0u}, mx[3] = {0u, 0u, 0u}, sor[3] = {0u, 0u, 0u}, sand[3] = {1u, 1u, 1u};
    // the tile's fixed-point coordinate sums (tsum, sole-owner tiles of k_lloyd1),
    // compressed or raw: a thread's <= 4 GPT points of |xq| < 2^25 fit int32
    static_assert(4 * GPT <= 32, "per-thread fixed-point sums stay below 2^31");
    int fs[3] = {0, 0, 0};
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
        const unsigned gg = g0 + (unsigned)tid + 256u * u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned i = 4u * gg + (unsigned)k;
            if (gg >= g1 || i < start || i >= end) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const unsigned b = word(u, a, k);
                mn[a] = min(mn[a], b);
                mx[a] = max(mx[a], b);
                sor[a] |= b >> 31;
                sand[a] &= b >> 31;
                fs[a] += fixed_i(__uint_as_float(b), qe.q[a]);
            }
        }
    }
    __shared__ unsigned smn[4][3], smx[4][3], sso[4][3], ssa[4][3];
    __shared__ long long ssum[4][3];
    __shared__ uint4 meta;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        long long fl = fs[a];
        for (int o = 32; o > 0; o >>= 1) fl += __shfl_xor(fl, o);
        if (lane == 0) ssum[wv][a] = fl;
        for (int o = 32; o > 0; o >>= 1) {
            mn[a] = min(mn[a], (unsigned)__shfl_xor((int)mn[a], o));
            mx[a] = max(mx[a], (unsigned)__shfl_xor((int)mx[a], o));
            sor[a] |= (unsigned)__shfl_xor((int)sor[a], o);
            sand[a] &= (unsigned)__shfl_xor((int)sand[a], o);
        }
        if (lane == 0) { smn[wv][a] = mn[a]; smx[wv][a] = mx[a]; sso[wv][a] = sor[a]; ssa[wv][a] = sand[a]; }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned w[3], lo[3], total = 0;
        bool ok = true;
        for (int a = 0; a < 3; ++a) tsum[(size_t)t * 3 + a] = (ssum[0][a] + ssum[1][a]) + (ssum[2][a] + ssum[3][a]);
        for (int a = 0; a < 3; ++a) {
            unsigned m0 = ~0u, m1 = 0u, so = 0u, sa = 1u;
            for (int k = 0; k < 4; ++k) { m0 = min(m0, smn[k][a]); m1 = max(m1, smx[k][a]); so |= sso[k][a]; sa &= ssa[k][a]; }
            lo[a] = m0;
            w[a] = zwidth(m1 - m0);
            ok = ok && (so == sa) && w[a] <= 31u;
            total += w[a];
        }
        // the z field sits at the top of the 64-bit record (decoded by one shift of
        // the high word): at least 1 bit wide, so the shift stays below 32
        // (w0 + w1 <= 62: the extra bit always fits)
        if (w[2] == 0u) { w[2] = 1u; ++total; }
        ok = ok && total <= 64u;
        meta = make_uint4(lo[0], lo[1], lo[2], ok ? (0x80000000u | w[0] | (w[1] << 8) | (w[2] << 16)) : 0u);
        tmeta[t] = meta;
        if (ok) atomicAdd(zpts + (t % 32u) * 16u, (unsigned long long)(end - start));   // 32 replica lines
    }
    __syncthreads();
    const uint4 m = meta;
    if (!(m.w >> 31)) return;
    const unsigned w0 = m.w & 0xffu, w2 = (m.w >> 16) & 0xffu;
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
        const unsigned gg = g0 + (unsigned)tid + 256u * u;
        if (gg >= g1) continue;
        unsigned lw[4], hw[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long d0 = word(u, 0, k) - m.x;
            const unsigned long long d1 = word(u, 1, k) - m.y;
            const unsigned long long d2 = word(u, 2, k) - m.z;
            const unsigned long long v = d0 | (d1 << w0) | (d2 << (64u - w2));
            lw[k] = (unsigned)v;
            hw[k] = (unsigned)(v >> 32);
        }
        const unsigned i0 = 4u * gg;
        const size_t zg = zword(i0);   // 4 consecutive words, 16-B aligned (i0 % 4 == 0, same 256-point block)
        if (i0 >= start && i0 + 4u <= end) {
            *reinterpret_cast<uint4 *>(xz + zg) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
            *reinterpret_cast<uint4 *>(xz + zg + ZHI) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        } else {   // a group at the tile's edge: only this tile's points
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned i = i0 + (unsigned)k;
                if (i < start || i >= end) continue;
                xz[zg + k] = lw[k];
                xz[zg + k + ZHI] = hw[k];
            }
        }
    }
}

// tsum[t][a] = sum over the tile's points of fixed_i(x_a, q_a), for the layouts
// k_tile_compress does not see (fp16, D != 3, PCM_XZ=0): one block per tile.
template <typename T, int D>
__global__ __launch_bounds__(256) void k_tile_sums(const T *__restrict__ xs, const uint4 *__restrict__ tiles,
                                                   const uint32_t *__restrict__ ntiles, QExp qe,
                                                   long long *__restrict__ tsum) {
    const unsigned t = blockIdx.x;
    if (t >= *ntiles) return;
    const uint4 tr = tiles[t];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long fs[D];
#pragma unroll
    for (int a = 0; a < D; ++a) fs[a] = 0;
    for (unsigned i = tr.y + tid; i < tr.z; i += 256)
#pragma unroll
        for (int a = 0; a < D; ++a) fs[a] += fixed_i(to_f<T>(xs[xs_index<D>(i, a)]), qe.q[a]);
    __shared__ long long ssum[4][MAXD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        for (int o = 32; o > 0; o >>= 1) fs[a] += __shfl_xor(fs[a], o);
        if (lane == 0) ssum[wv][a] = fs[a];
    }
    __syncthreads();
    if (tid < D) tsum[(size_t)t * D + tid] = (ssum[0][tid] + ssum[1][tid]) + (ssum[2][tid] + ssum[3][tid]);
}

// ------------------------------------------------------------------ crowded cells: tile lists
// A uniform grid cannot follow tight clusters: a cell that holds a whole
// cluster holds its hundreds of centres too, its list overflows CAPF (FULL) and
// every point of it scans all K (a 16-cluster K = 4096 cloud: 20 ms per
// iteration, VALU-bound).  When the layout finds crowded cells (an occupancy
// sample, pcm_layout_build) it orders each cell's points by a Morton code of
// `zlev` further bisections (sort_key), so a tile -- a run of <= TILE points of
// one cell -- covers a compact piece of the cell; k_tile_box records each
// tile's exact point box, and before every assign launch k_tile_cand builds,
// for the tiles of FULL cells, a list over that box with the same exact
// dominance test as the cell lists (any box holding the points is valid).

// Occupancy sample: counts[cell of point i * stride] += 1, i < m; counts[ncells]
// := the largest count afterwards (k_umax).
template <typename T, int D>
__global__ __launch_bounds__(256) void k_zsample(const T *__restrict__ X, long long m, long long stride, Grid g,
                                                 uint32_t *__restrict__ counts) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= m) return;
    const long long p = i * stride;
    int idx[MAXD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const double t = ((double)to_f<T>(X[p * D + a]) - g.lo[a]) * g.inv[a];
        int v = (int)floor(t);
        idx[a] = v < 0 ? 0 : (v >= g.G[a] ? g.G[a] - 1 : v);
    }
    atomicAdd(counts + encode(idx, g.G, D), 1u);
}

inline __global__ __launch_bounds__(256) void k_umax(const uint32_t *__restrict__ v, long long n, uint32_t *__restrict__ out) {
    uint32_t m = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        m = max(m, v[i]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// Exact fp32 box of every tile's points: tbox[2t] = lower, tbox[2t + 1] = upper corner.
template <typename T, int D>
__global__ __launch_bounds__(256) void k_tile_box(const T *__restrict__ xs, const uint4 *__restrict__ tiles,
                                                  const uint32_t *__restrict__ ntiles, float4 *__restrict__ tbox) {
    const unsigned t = blockIdx.x;
    if (t >= *ntiles) return;
    const uint4 tr = tiles[t];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float mn[D], mx[D];
#pragma unroll
    for (int a = 0; a < D; ++a) { mn[a] = __builtin_inff(); mx[a] = -__builtin_inff(); }
    for (unsigned i = tr.y + tid; i < tr.z; i += 256)
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const float v = to_f<T>(xs[xs_index<D>(i, a)]);
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
    __shared__ float smn[4][MAXD], smx[4][MAXD];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        for (int o = 32; o > 0; o >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
        }
        if (lane == 0) { smn[wv][a] = mn[a]; smx[wv][a] = mx[a]; }
    }
    __syncthreads();
    if (tid == 0) {
        float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < D; ++a) {
            lo[a] = fminf(fminf(smn[0][a], smn[1][a]), fminf(smn[2][a], smn[3][a]));
            hi[a] = fmaxf(fmaxf(smx[0][a], smx[1][a]), fmaxf(smx[2][a], smx[3][a]));
        }
        tbox[2 * (size_t)t] = make_float4(lo[0], lo[1], lo[2], lo[3]);
        tbox[2 * (size_t)t + 1] = make_float4(hi[0], hi[1], hi[2], hi[3]);
    }
}

// List of one tile of a crowded cell (list FULL or longer than TL_MIN) over its
// point box, at the current centres:
// reference r = a centre of least max distance to the box, then every centre
// not provably dominated by r (prunable), compacted in ascending centroid index
// (the strict-'<' scan keeps the lowest index on ties).  tl_cnt[t] = the length,
// or FULL when it is not shorter than the cell's list or exceeds CAPF.  Tiles of
// other cells are skipped (k_lloyd1 reads tl_cnt only for cells past TL_MIN).
template <int D>
__global__ __launch_bounds__(256) void k_tile_cand(const uint4 *__restrict__ tiles, const uint32_t *__restrict__ ntiles,
                                                   const uint32_t *__restrict__ fc_cnt, const float4 *__restrict__ tbox,
                                                   const float4 *__restrict__ C, int K, uint32_t *__restrict__ tl_cnt,
                                                   float4 *__restrict__ tl_rec, int32_t *__restrict__ tl_lab,
                                                   const Ctrl *__restrict__ ctrl, int gate) {
    const unsigned t = blockIdx.x;
    if (gate && gated(ctrl)) return;
    if (t >= *ntiles) return;
    const uint4 tr = tiles[t];
    const uint32_t cc = fc_cnt[tr.x];
    if (cc <= TL_MIN) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float4 lo4 = tbox[2 * (size_t)t], hi4 = tbox[2 * (size_t)t + 1];
    double blo[MAXD], bhi[MAXD];
#pragma unroll
    for (int a = 0; a < D; ++a) { blo[a] = (double)comp(lo4, a); bhi[a] = (double)comp(hi4, a); }
    double best = __builtin_inf();
    int bj = 0;
    for (int j = tid; j < K; j += 256) {
        const double md = maxdist<D>(blo, bhi, C[j]);
        if (md < best) { best = md; bj = j; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    __shared__ double s_b[4];
    __shared__ int s_j[4];
    __shared__ unsigned s_w[4];
    if (lane == 0) { s_b[wv] = best; s_j[wv] = bj; }
    __syncthreads();
    int rj = s_j[0];
    double rb = s_b[0];
    for (int w = 1; w < 4; ++w)
        if (s_b[w] < rb || (s_b[w] == rb && s_j[w] < rj)) { rb = s_b[w]; rj = s_j[w]; }
    const float4 r = C[rj];
    unsigned base = 0;
    for (int j0 = 0; j0 < K; j0 += 256) {
        const int j = j0 + tid;
        const bool keep = j < K && !prunable<D>(blo, bhi, C[j < K ? j : 0], r);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_w[wv] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned off = base, total = 0;
        for (int w = 0; w < 4; ++w) {
            off += (w < wv) ? s_w[w] : 0u;
            total += s_w[w];
        }
        const unsigned pos = off + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (keep && pos < (unsigned)TLMAX) {
            tl_rec[(size_t)t * TLMAX + pos] = C[j];
            tl_lab[(size_t)t * TLMAX + pos] = j;
        }
        base += total;
        __syncthreads();   // s_w is rewritten by the next chunk
        if (base > (unsigned)TLMAX) break;   // block-uniform
    }
    // FULL: no shorter list than the cell's (the tile scans the cell list, or all K)
    if (tid == 0) tl_cnt[t] = (base <= (unsigned)TLMAX && base < cc) ? base : FULL;
}

// Tile-list summary: out[0] += tiles of cells past TL_MIN, out[1] += those with a
// tile list, out[2] += the lengths of those lists; out[3] += tile lists longer
// than TLCAP (k_lloyd1 scans them through LDS chunks), out[4] += all-K tiles (a
// FULL cell whose tile got no list either), out[5] = the longest tile list.
inline __global__ __launch_bounds__(256) void k_tile_list_stats(const uint4 *__restrict__ tiles,
                                                         const uint32_t *__restrict__ ntiles,
                                                         const uint32_t *__restrict__ fc_cnt,
                                                         const uint32_t *__restrict__ tl_cnt,
                                                         unsigned long long *__restrict__ out) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= *ntiles) return;
    const uint32_t cc = fc_cnt[tiles[t].x];
    if (cc <= TL_MIN) return;
    atomicAdd(out, 1ull);
    const uint32_t c = tl_cnt[t];
    if (c != FULL) {
        atomicAdd(out + 1, 1ull);
        atomicAdd(out + 2, (unsigned long long)c);
        if (c > (uint32_t)TLCAP) atomicAdd(out + 3, 1ull);
        atomicMax(out + 5, (unsigned long long)c);
    } else if (cc == FULL) {
        atomicAdd(out + 4, 1ull);
    }
}

}  // namespace pcm
