// pcm_assign.hpp (a part of pcm_kernels.hpp) — E-step kernels: k_label (labels + inertia) and k_lloyd1 (assign + accumulation)
#pragma once
#include "pcm_kcommon.hpp"
#include "pcm_layout.hpp"   // zword, ZHI

namespace pcm {

// ------------------------------------------------------------------ assign
// Nearest of mm candidates for 4 points per lane: strict '<' in ascending
// candidate order, so the lowest index wins ties (_k_means_lloyd.pyx:205-213).
template <int D, typename P>
__device__ __forceinline__ void scan4(P rec, int mm, const float (&x)[4][D], float (&bd)[4], int (&bj)[4]) {
    {
        const float4 c = rec[0];
        for (int e = 0; e < 4; ++e) { bd[e] = dist_canon<D>(x[e], c); bj[e] = 0; }
    }
#pragma unroll 2
    for (int j = 1; j < mm; ++j) {
        const float4 c = rec[j];
        for (int e = 0; e < 4; ++e) {
            float dd = dist_canon<D>(x[e], c);
            bool lt = dd < bd[e];
            bd[e] = lt ? dd : bd[e];
            bj[e] = lt ? j : bj[e];
        }
    }
}

// Same scan over the list positions set in a wave-uniform mask (ascending, so
// the lowest index still wins ties); m has at least one bit set.
template <int D, typename P>
__device__ __forceinline__ void scan4_m(P rec, unsigned long long m, const float (&x)[4][D], float (&bd)[4],
                                        int (&bj)[4]) {
    {
        const int j = __builtin_ctzll(m);
        m &= m - 1ull;
        const float4 c = rec[j];
        for (int e = 0; e < 4; ++e) { bd[e] = dist_canon<D>(x[e], c); bj[e] = j; }
    }
    while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1ull;
        const float4 c = rec[j];
        for (int e = 0; e < 4; ++e) {
            float dd = dist_canon<D>(x[e], c);
            bool lt = dd < bd[e];
            bd[e] = lt ? dd : bd[e];
            bj[e] = lt ? j : bj[e];
        }
    }
}

typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ rsrc_t make_rsrc(const void *base, unsigned long long bytes) {
    const unsigned long long b = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    const unsigned nb = __builtin_amdgcn_readfirstlane((unsigned)(bytes > 0xffffffffull ? 0xffffffffull : bytes));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), (short)0, (int)nb,
                                             0x00020000);
}

// Lane-local 4 consecutive points in the packed AoS layout ([npad][D] of T):
// 4*D*sizeof(T) bytes = NW 32-bit words, loaded as b128 pieces (+ a b64 tail).
template <typename T, int D> struct Raw {
    static constexpr int NW = 4 * D * (int)sizeof(T) / 4;
    unsigned w[NW];
};
template <typename LT> struct RawLab;
template <> struct RawLab<uint16_t> {
    u32x2 w;
};
template <> struct RawLab<int32_t> {
    u32x4 w;
};

// The point stream loads with the default cache policy (0; NT, 2, measured 22%
// slower: 349 vs 282 us per launch, and no gain in the other kernels).
// off_pt = index of the lane's first point; one descriptor for the whole AoS array.
template <typename T, int D>
__device__ __forceinline__ void load_x(Raw<T, D> &r, rsrc_t rs, unsigned off_pt) {
    constexpr int NW = Raw<T, D>::NW;
    const unsigned boff = off_pt * (unsigned)(D * sizeof(T));
    for (int k = 0; k + 4 <= NW; k += 4) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, boff + 4u * k, 0, 0);
        r.w[k] = v[0]; r.w[k + 1] = v[1]; r.w[k + 2] = v[2]; r.w[k + 3] = v[3];
    }
    if (NW % 4 == 2) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, boff + 4u * (NW - 2), 0, 0);
        r.w[NW - 2] = v[0]; r.w[NW - 1] = v[1];
    }
}
// compressed item: 4 points' 8-B records, lo words then hi words (AoSoA-4)
// (templated so that k_lloyd1's other instances, which never call it, compile)
template <typename R>
__device__ __forceinline__ void load_z2(R &r, rsrc_t rA, unsigned off_pt) {
    static_assert(sizeof(r.w) >= 8 * sizeof(unsigned), "compressed items fill 8 words");
    // off_pt is a multiple of 4 (or the out-of-range 0x0ffffff0: offsets past any
    // buffer, zeros without memory traffic)
    const unsigned boff = off_pt >= 0x0ffffff0u ? 0xfffff000u : (unsigned)zword(off_pt) * 4u;
    const u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(rA, boff, 0, 0);
    const u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(rA, boff + 4u * ZHI, 0, 0);
    r.w[0] = v0[0]; r.w[1] = v0[1]; r.w[2] = v0[2]; r.w[3] = v0[3];
    r.w[4] = v1[0]; r.w[5] = v1[1]; r.w[6] = v1[2]; r.w[7] = v1[3];
}
// exact fp32 coordinates of a compressed item (k_tile_compress): base + delta bits
// (sh1 = w0, sh2 = 32 - w2)
template <typename R, int DD>
__device__ __forceinline__ void unpack_z(const R &r, float (&x)[4][DD], const uint4 &zm, unsigned sh1,
                                         unsigned sh2, unsigned m0, unsigned m1) {
    static_assert(DD == 3 && sizeof(r.w) >= 8 * sizeof(unsigned), "compressed tiles: fp32 D = 3");
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned lo = r.w[e], hi = r.w[4 + e];
        x[e][0] = __uint_as_float(zm.x + (lo & m0));
        x[e][1] = __uint_as_float(zm.y + (__builtin_amdgcn_alignbit(hi, lo, sh1) & m1));
        x[e][2] = __uint_as_float(zm.z + (hi >> sh2));
    }
}
// AoSoA-4 (xs_index): word a*4 + e holds coordinate a of the lane's point e
template <int D>
__device__ __forceinline__ void unpack_x(const Raw<float, D> &r, float (&x)[4][D]) {
    for (int e = 0; e < 4; ++e)
        for (int a = 0; a < D; ++a) x[e][a] = __uint_as_float(r.w[a * 4 + e]);
}
template <int D>
__device__ __forceinline__ void unpack_x(const Raw<__half, D> &r, float (&x)[4][D]) {
    for (int e = 0; e < 4; ++e)
        for (int a = 0; a < D; ++a) {
            const int k = a * 4 + e;
            const unsigned word = r.w[k >> 1];
            const unsigned short hb = (unsigned short)((k & 1) ? (word >> 16) : (word & 0xffffu));
            x[e][a] = __half2float(__ushort_as_half(hb));
        }
}
__device__ __forceinline__ void store_l4(rsrc_t rs, unsigned off, const int (&l)[4], const bool (&v)[4],
                                         RawLab<uint16_t> *) {
    if (v[0] & v[1] & v[2] & v[3]) {
        u32x2 w;
        w[0] = ((unsigned)l[0] & 0xffffu) | ((unsigned)l[1] << 16);
        w[1] = ((unsigned)l[2] & 0xffffu) | ((unsigned)l[3] << 16);
        __builtin_amdgcn_raw_buffer_store_b64(w, rs, off * 2u, 0, 0);
    } else {
        for (int e = 0; e < 4; ++e)
            if (v[e]) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)l[e], rs, (off + e) * 2u, 0, 0);
    }
}
__device__ __forceinline__ void store_l4(rsrc_t rs, unsigned off, const int (&l)[4], const bool (&v)[4],
                                         RawLab<int32_t> *) {
    if (v[0] & v[1] & v[2] & v[3]) {
        u32x4 w;
        for (int e = 0; e < 4; ++e) w[e] = (unsigned)l[e];
        __builtin_amdgcn_raw_buffer_store_b128(w, rs, off * 4u, 0, 0);
    } else {
        for (int e = 0; e < 4; ++e)
            if (v[e]) __builtin_amdgcn_raw_buffer_store_b32((unsigned)l[e], rs, (off + e) * 4u, 0, 0);
    }
}

#ifndef PCM_LSLOT
#define PCM_LSLOT 16
#endif
constexpr int LSLOT = PCM_LSLOT;

// Lane-minor accumulator words shared by threads tid and tid + AW = TPB / 2 (different
// waves, so an instruction never hits one word twice): word (slot, a) of column
// c = tid & 127 at (slot*(D+1)+a)*128 + c -- a wave's ds_add_u32 hits 32 distinct
// banks per half-wave whatever the slots.  A word sums <= 2 x 32 points of
// |xq| < 2^25 per tile: < 2^31, exact in int32.
constexpr int AW = TPB >= 128 ? TPB / 2 : TPB;   // one wave per block: no sharing (same-instruction lanes must not collide)
template <int D, int LS = LSLOT> struct AccL {
    static constexpr int rows = (LS + 1) * (D + 1);   // + junk slot
    static constexpr int words = AW * rows;
    // crowded layouts launch k_lloyd1 with this much more dynamic LDS: int64
    // words of long tile lists' positions (LDS atomics, one global atomic per
    // word and tile at the end instead of one per point: contended global
    // atomics made a 16-cluster K = 4096 cloud L2-atomic-bound)
    static constexpr int gwords = TLCAP * (D + 1);
    static constexpr size_t bytes_crowded = ((size_t)words * 4 + 7) / 8 * 8 + (size_t)gwords * 8;
};

// XCD-aware block order (a speed choice only: every kernel using it is
// correct under any dispatch).  The dispatcher deals a grid's blocks round-robin
// over the 8 XCDs, each with its own L2, so by default neighbouring chunks or
// tiles -- which share the cache lines at their boundaries and often their
// cell's records -- run on different XCDs.  This maps the blocks one XCD
// receives (b % 8 labels them) onto one contiguous range of chunk ids, in
// dispatch order; bijective on [0, nb) for any nb.
__device__ __forceinline__ unsigned xcd_block(unsigned b, unsigned nb) {
    const unsigned q = nb >> 3, r = nb & 7u, x = b & 7u, k = b >> 3;
    return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + k;
}

struct LloydArgs {
    const void *xs;                 // packed AoS [npad][D] of T, cell order
    const unsigned *xz;             // compressed 8-B records (fp32 D = 3 tiles with tmeta .w bit 31), or null
    const uint4 *tmeta;             // per-tile compression record (k_tile_compress), or null
    long long npad;
    const uint4 *tiles;             // {cell, start, end, owner word (SoleW)}
    const long long *tsum;          // [tile][D] fixed-point coordinate sums of the tile's points (layout time)
    const uint32_t *fc_cnt;         // candidate count per cell (FULL: all K)
    const uint32_t *ntiles;         // device: tile count of the layout
    const float4 *fc_rec;
    const int32_t *fc_lab;
    const float4 *C;                // all centres (FULL cells)
    int K;
    int q[MAXD];
    unsigned long long *stats;      // accumulation target: [K][D+1] integer statistics
    const Ctrl *ctrl;
    const uint32_t *sub_start;      // [(ncells << D) + 1] sub-cell starts (k_lloyd1's per-round candidate masks)
    int sub;                        // the layout is sorted by sub-cell (else sub_start is [ncells + 1])
    Grid g;
    const uint32_t *tl_cnt;         // crowded layouts: per-tile list length for tiles of FULL cells (or FULL), else null
    const float4 *tl_rec;           // [tile][TLCAP] records of the tile lists (k_tile_cand)
    const float4 *tbox;             // crowded layouts: [tile][2] exact point box (lo, hi), else null
    const int32_t *tl_lab;
    int xcd;                        // k_lloyd1 takes its tile through xcd_block
    int fast;                       // short-list tiles take k_lloyd1's lean rounds (PCM_FAST=0: none does)
    int tilecost;                   // a wave with no point of the tile in a round skips it (PCM_TILECOST=0: it computes it)
};

struct TileL {
    unsigned cell, start, end, base0;
    int mm, full, nr, pad_;
};

// t.w = the cell's candidate count (fc_cnt[t.x], or FULL)
__device__ __forceinline__ TileL make_tile(const uint4 &t, int K) {
    TileL h;
    h.cell = t.x;
    h.start = t.y;
    h.end = t.z;
    h.full = (t.w == FULL) ? 1 : 0;
    h.mm = h.full ? K : (int)t.w;
    h.base0 = h.start & ~3u;
    h.nr = (int)((h.end - h.base0 + 4 * TPB - 1) / (4 * TPB));
    h.pad_ = 0;
    return h;
}

// Exact, order-independent inertia: a point adds w = trunc(d * 2^s) (d the
// canonical fp32 distance; s from the global fixed-point exponents so that
// w < 2^64, see inertia_scale); per-thread 128-bit sums are split into three
// 32-bit limbs, which are summed with integer atomics.  The total is the same
// integer for any block order, grid size or number of ranks
// (oracle/lloyd_ref.py inertia_exact).
__device__ __forceinline__ void inert_add(unsigned long long &lo, unsigned long long &hi, unsigned &ovf, float d,
                                          int s) {
    const double v = __builtin_ldexp((double)d, s);
    unsigned long long w;
    if (v < 18446744073709551616.0) {
        w = (unsigned long long)v;   // truncation (d >= 0)
    } else {
        w = ~0ull;
        ++ovf;
    }
    lo += w;
    hi += (lo < w) ? 1ull : 0ull;
}

// Block-wide: the limbs of all threads summed, then one add per limb into the
// block's replica line out[blockIdx % INERT_REP][0..3] (k_inert_fold sums them).
__device__ __forceinline__ void inert_flush(unsigned long long lo, unsigned long long hi, unsigned ovf,
                                            unsigned long long *__restrict__ out) {
    __shared__ unsigned long long s_l[TPB / 64][4];
    unsigned long long l[4] = {lo & 0xffffffffull, lo >> 32, hi, (unsigned long long)ovf};
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int o = 32; o > 0; o >>= 1) l[q] += __shfl_xor(l[q], o);
        if ((threadIdx.x & 63) == 0) s_l[wv][q] = l[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long v = 0ull;
        for (int w = 0; w < TPB / 64; ++w) v += s_l[w][threadIdx.x];
        if (v) atomicAdd(out + (size_t)(blockIdx.x % INERT_REP) * 16 + threadIdx.x, v);
    }
}

// inert[0..3] += the replica sums; replicas := 0 (one 64-thread block)
inline __global__ void k_inert_fold(unsigned long long *__restrict__ rep, unsigned long long *__restrict__ inert) {
    const int q = threadIdx.x;
    if (q >= 4) return;
    unsigned long long v = 0ull;
    for (int r = 0; r < INERT_REP; ++r) {
        v += rep[r * 16 + q];
        rep[r * 16 + q] = 0ull;
    }
    inert[q] += v;
}

// E-step with the current centres writing labels (sorted order) and the
// inertia (final E-step of _kmeans.py:736-750, relocation keys).  Not gated.
// Same tiles and candidate lists as k_lloyd1 (blocks walk tiles b, b + G, ...;
// the engine launches one block per tile); 4 points per lane per round,
// the loads of the next round in flight while one is computed; compressed
// tiles read their 8-B records (round 4), like k_lloyd1.
template <typename T, int D, typename LT>
__global__ __launch_bounds__(TPB) void k_label(LloydArgs A, void *lab, unsigned long long *inert_out, int iscale) {
    __shared__ float4 crec[CAPF];
    __shared__ int32_t cid[CAPF];
    const int tid = threadIdx.x;
    const unsigned G = gridDim.x;
    const unsigned nt = *A.ntiles;
    const float4 *lrec = A.fc_rec;
    const int32_t *llab = A.fc_lab;
    const rsrc_t rx = make_rsrc(A.xs, (unsigned long long)A.npad * D * sizeof(T));
    const rsrc_t rl = make_rsrc(lab, (unsigned long long)A.npad * sizeof(LT));
    constexpr bool ZOK = sizeof(T) == 4 && D == 3;   // compressed tiles exist only for fp32 D = 3
    const rsrc_t rz = make_rsrc(A.xz ? (const void *)A.xz : A.xs,
                                A.xz ? (unsigned long long)(A.npad + 255) / 256 * 256 * 8 : 0ull);
    unsigned long long ilo = 0ull, ihi = 0ull;
    unsigned iovf = 0u;
    for (unsigned t = blockIdx.x; t < nt; t += G) {
        uint4 tr = A.tiles[t];
        tr.w = A.fc_cnt[tr.x];
        const float4 *trec = lrec + (size_t)tr.x * CAPF;
        const int32_t *tlab = llab + (size_t)tr.x * CAPF;
        const float4 *Cs = A.C;             // all-K / long-list scans read these records
        const int32_t *glab = nullptr;      // long tile list: position -> centroid index
        if (tr.w > TL_MIN && A.tl_cnt && A.tl_cnt[t] != FULL) {   // crowded cell: the tile's own list
            const uint32_t tc = A.tl_cnt[t];
            trec = A.tl_rec + (size_t)t * TLMAX;
            tlab = A.tl_lab + (size_t)t * TLMAX;
            tr.w = tc;
            if (tc > (uint32_t)CAPF) { Cs = trec; glab = tlab; }
        }
        TileL h = make_tile(tr, A.K);
        if (glab) { h.full = 1; h.mm = (int)tr.w; }
        // compressed tile (fp32 D = 3): its 8-B records, decoded exactly as in k_lloyd1
        uint4 zm = make_uint4(0u, 0u, 0u, 0u);
        if (ZOK && A.tmeta) zm = A.tmeta[t];
        __syncthreads();
        if (!h.full && tid < h.mm) {
            crec[tid] = trec[tid];
            cid[tid] = tlab[tid];
        }
        __syncthreads();
        // one instance per point format (block-uniform per tile), so each keeps a
        // constant load count per item for hipcc's waitcnt pass
        auto run = [&](auto ZCc) {
            constexpr bool ZC = decltype(ZCc)::value;
            const unsigned zw0 = zm.w & 0xffu, zw1 = (zm.w >> 8) & 0xffu, zw2 = (zm.w >> 16) & 0xffu;
            const unsigned zsh1 = zw0, zsh2 = 32u - zw2, zm0 = (1u << zw0) - 1u, zm1 = (1u << zw1) - 1u;
            auto ldx = [&](Raw<T, D> &dst, unsigned off) {
                if constexpr (ZC) load_z2(dst, rz, off);
                else load_x<T, D>(dst, rx, off);
            };
            Raw<T, D> cur, nxt;
            ldx(cur, h.base0 + 4u * tid);
            for (int r = 0; r < h.nr; ++r) {
                const unsigned i0 = h.base0 + (unsigned)r * 4u * TPB + 4u * tid;
                ldx(nxt, r + 1 < h.nr ? i0 + 4u * TPB : 0x0ffffff0u);
                float x[4][D];
                if constexpr (ZC) unpack_z(cur, x, zm, zsh1, zsh2, zm0, zm1);
                else unpack_x<D>(cur, x);
                float bd[4];
                int bj[4];
                if (h.full) scan4<D>(Cs, h.mm, x, bd, bj);
                else scan4<D>(crec, h.mm, x, bd, bj);
                int lbl[4];
                bool v[4];
                for (int e = 0; e < 4; ++e) {
                    lbl[e] = h.full ? (glab ? glab[bj[e]] : bj[e]) : cid[bj[e]];
                    v[e] = (i0 + e >= h.start) && (i0 + e < h.end);
                    if (v[e] && inert_out) inert_add(ilo, ihi, iovf, bd[e], iscale);
                }
                if (i0 < h.end) store_l4(rl, i0, lbl, v, (RawLab<LT> *)nullptr);
                cur = nxt;
            }
        };
        if constexpr (ZOK) {
            if (zm.w >> 31) run(std::true_type{});
            else run(std::false_type{});
        } else {
            run(std::false_type{});
        }
    }
    if (inert_out) inert_flush(ilo, ihi, iovf, inert_out);
}

// ------------------------------------------------------------------ Lloyd iteration
// One Lloyd iteration's E-step + accumulation (sklearn's lloyd_iter_chunked_dense
// with update_centers=True, _k_means_lloyd.pyx:23-165).  It streams ONLY the
// points (12 B/pt at fp32 D=3): no label array is read or written.  sklearn's
// strict-convergence test (labels equal, _kmeans.py:717-723) is replaced by
// "the raw integer statistics equal the previous iteration's" in the update kernels (upd_row): equal
// labels give equal statistics, and equal statistics give equal centres, i.e.
// shift 0 <= tol, so sklearn stops at that same iteration either way (DESIGN.md
// "Convergence").
//
// Per tile (a run of one cell's points): the candidate list (ascending centroid
// index, so the strict-'<' scan keeps the lowest index on ties,
// _k_means_lloyd.pyx:205-213) in LDS; a winner's fixed-point coordinates and
// count are summed into LDS words of its lane slot (ds_add_u32, lane-minor:
// conflict-free), winners without a slot into int64 words; out-of-tile lanes of
// a partial round add into a junk slot (never read).  A tile whose list fits
// the lane slots -- nearly every tile of a fine grid -- takes lean rounds (see
// `lean` below): no slot map, no overflow test, and in the rounds that lie
// wholly inside the tile no in-tile test either (config 3: 72.1M -> 67.1M VALU
// and 32.8M -> 25.4M SALU wave-instructions per launch, k_lloyd1 164 -> 155 us,
// profiles/fastpath_ab.txt).  Outside the rounds a tile zeroes only the slot rows
// its fold reads and folds them with 16-byte reads and DPP row sums
// (zero_and_stage, fold below), and a wave computes only the rounds in
// which it has a point of the tile (`nrw`; config 3: 66.6M -> 61.9M VALU and
// 8.25M -> 6.40M LDS wave-instructions per launch, profiles/tilecost_ab.txt).
// Nearest of mm centres read through scalar loads (FULL tiles: the whole
// uniform centre array); same scan order and tie rule as scan4.
template <int D>
__device__ __forceinline__ void scan4_s(const float4 *__restrict__ C, int mm, const float (&x)[4][D], float (&bd)[4],
                                        int (&bj)[4]) {
    {
        const float4 c = C[0];
        for (int e = 0; e < 4; ++e) { bd[e] = dist_canon<D>(x[e], c); bj[e] = 0; }
    }
    for (int j = 1; j < mm; ++j) {
        const float4 c = C[j];
        for (int e = 0; e < 4; ++e) {
            float dd = dist_canon<D>(x[e], c);
            bool lt = dd < bd[e];
            bd[e] = lt ? dd : bd[e];
            bj[e] = lt ? j : bj[e];
        }
    }
}

#ifndef PCM_WPE
#define PCM_WPE 4
#endif
#ifndef PCM_WPE_FINE
#define PCM_WPE_FINE 7
#endif
#ifndef PCM_WPE_D4
#define PCM_WPE_D4 6
#endif
// One Lloyd iteration's E-step + accumulation, ONE TILE PER BLOCK (the round-1
// persistent tile walk, removed in round 5, measured 211 vs 238 us at config 3).
// The block's start-up: the tile record, the candidate count and the first
// LSPEC list records (vector loads, speculative: the count is not known yet)
// and the first two work items' point loads are all issued before anything
// is waited for, so a block starts scanning one point-load latency after it
// starts (the tile record -> count -> records chain cost ~3.8 us per block,
// a quarter of its lifetime at config 3).  The list loads precede the point
// loads, so the in-order vmcnt wait for the first work item covers them.
// Sole-owner tiles (SoleW above): the tile record's owner word and the tile's
// layout-time sums (tsum) arrive in that first latency too; when the word is
// set the block adds the D sums and the point count to that centroid's row
// and returns before any list or point load is issued -- the statistics are
// exact integers, so the result is the one the streamed tile would give
// (config 3: 23-24 % of the tiles, k_lloyd1 198 -> 169 us, profiles/sole_tiles_ab.txt).
constexpr int LSPEC = 16;   // list records loaded before the count is known
#ifndef PCM_MASK_MIN
#define PCM_MASK_MIN 2
#endif
constexpr int MASK_MIN = PCM_MASK_MIN;   // sub-cell masks for lists of at least this length
// Minimum waves per SIMD the compiler must fit (a VGPR budget): the fine-grid
// fp32 variant (LS = 8, no masks) fits 6 without spilling (70 VGPRs instead of
// 82 at 4: 10 -> 12 resident blocks per CU; config 3 assign 214.7 -> 209.8 us
// on one box, tools/wpe_sweep.sh -- across boxes the rocprof average moved
// only 212.5 -> 211.3 us: the kernel is memory-bound, residency was not the
// limit); the masked 16-slot variant spills at 6 (12.5M shard
// 42.0 -> 45.5 us) and D = 4 gains nothing, so they keep 4.  Round 5: once the
// D <= 3 overflow words left LDS (10.9 KB per block), the fine-grid variant at
// 7 waves (71 VGPRs, 94 SGPRs; 4 VGPRs spilled outside the rounds) measured
// 198.3-199.0 -> 195.0-196.3 us per launch at config 3 (events, one box,
// profiles/rd5_wpe7_ab.txt), so PCM_WPE_FINE is 7.  Likewise the D = 4
// 8-slot variant without its LDS overflow words (positions
// past the slots go to global atomics) fits 6 waves at 74 VGPRs: config-5
// 62.5M shard assign 332.7 -> 308.8-312.2 us, 8-way slab ~195 -> ~188 us per
// rank (profiles/rd5_d4_wpe6_ab.txt), so PCM_WPE_D4 is 6.
// Work items of a compressed tile in flight while one is computed (raw tiles: 2;
// depths 3 and 4 were measured and dropped, profiles/rd4_prefetch_ab.txt).
constexpr int ZPF = 2;
// A tile's fixed cost outside its rounds.  Only the slot rows
// the fold reads are zeroed (min(list, slots) * (D + 1) rows of AW words, 16-byte
// stores, once the list's length is in; kZeroLive) -- never the junk slot, which is
// written and never read.  The fold reads each thread's four words
// with one 16-byte load, sums their low and high 16-bit halves in int32 and
// reduces both over the 16-lane DPP row (no ds_bpermute, no 64-bit shuffles).
// (The full zeroing and the 64-bit shuffle fold they replaced: profiles/tilecost_ab.txt.)
// sum of v over the lane's DPP row (16 lanes), valid in the row's last lane:
// row_shr 8, 4, 2, 1, lanes shifted in from outside the row read 0
__device__ __forceinline__ int row16_sum_last(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
    return v;
}
template <typename T, int D, int LS, bool MASK>
constexpr int lloyd1_wpe() {
    return (sizeof(T) == 4 && D <= 3 && LS < LSLOT && !MASK) ? PCM_WPE_FINE
                                                             : ((D == 4 && LS < LSLOT && !MASK) ? PCM_WPE_D4 : PCM_WPE);
}
// the crowded-layout instance (tile lists, LDS-chunked long lists) does not fit
// a 6-wave budget: 80 VGPRs spilled 6 to scratch (round 5), so it keeps 5
template <typename T, int D, int LS, bool MASK, bool CROWD>
constexpr int lloyd1_wpe_c() { return CROWD ? (lloyd1_wpe<T, D, LS, MASK>() > 5 ? 5 : lloyd1_wpe<T, D, LS, MASK>()) : lloyd1_wpe<T, D, LS, MASK>(); }

// One point's fixed-point coordinates and its count added to an int64 row of
// D + 1 words, in LDS or in global memory -- one address space per call site
// (a pointer select would make FLAT atomics, which count in vmcnt and lgkmcnt
// and drain the prefetch).
template <int D>
__device__ __forceinline__ void add_point_row(unsigned long long *pp, const float (&x)[D], const int (&q)[MAXD]) {
    for (int a = 0; a < D; ++a) atomicAdd(pp + a, (unsigned long long)(long long)fixed_i(x[a], q[a]));
    atomicAdd(pp + D, 1ull);
}

// Sole-owner exit (SoleW, owner word w = centroid + 1): the tile's layout-time
// sums ts and its point count into that centroid's row of the statistics; no
// list or point load is issued.
template <int D>
__device__ __forceinline__ void lloyd1_sole_owner(unsigned long long *stats, unsigned w, unsigned start, unsigned end,
                                                  const long long (&ts)[D], int tid) {
    DBG_LV(7, 1ull | ((unsigned long long)(end - start) << 16));
    DBG_L(1);
    DBG_L(2);
    unsigned long long *pp = stats + (size_t)(w - 1u) * (D + 1);
    unsigned long long v = (unsigned long long)(end - start);
#pragma unroll
    for (int a = 0; a < D; ++a) v = tid == a ? (unsigned long long)ts[a] : v;
    if (tid <= D) atomicAdd(pp + tid, v);
    DBG_L(3);
}

// Sub-cell candidate masks: for every half-cell box (one per axis
// combination) the list positions its reference does not dominate (the
// exact test of the candidate lists, at the current centres), then per
// round the union over the sub-cells the round's points occupy.  Points are
// sorted by sub-cell within the cell, so a round (512 points) spans one or
// two sub-cells and scans ~the candidates of a cell half as wide; any
// superset of the undominated candidates, scanned in ascending order, gives
// the exact labels (a dominated candidate is strictly farther for every
// point of the box, so every tied minimiser is kept).
// only coarse grids (MASK: the 16-slot D <= 3 variant, lists of ~6 at a
// 12.5M shard: 47.8 -> 43.5 us per launch); at config 3 (lists of ~2.7)
// and D = 4 (16 sub-cells) the mask phase at the block's start cost more
// than the shorter scans saved (217 -> 225 us, 415 -> 488 us)
template <int D>
__device__ __forceinline__ void lloyd1_round_masks(const LloydArgs &A, unsigned cell, int mm, int nr, unsigned base0,
                                                   unsigned start, unsigned end, const uint32_t (&ss)[(1 << D) + 1],
                                                   const float4 *crec, uint32_t *okey, unsigned long long *omask,
                                                   unsigned long long *rmask, int tid) {
    constexpr int NSUB = 1 << D;
    int ci[MAXD];
    for (int a = D - 1, c = (int)cell; a >= 0; --a) {   // cell ids fit 32 bits (sort keys)
        ci[a] = (int)((unsigned)c % (unsigned)A.g.G[a]);
        c = (int)((unsigned)c / (unsigned)A.g.G[a]);
    }
    double cblo[MAXD], cbhi[MAXD], mid[MAXD];
    cell_box<D>(A.g, ci, ci, cblo, cbhi);
#pragma unroll
    for (int a = 0; a < D; ++a) mid[a] = A.g.lo[a] + ((double)ci[a] + 0.5) * A.g.w[a];
    auto sub_box = [&](int o, double *blo, double *bhi) {
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const bool up = (o >> (D - 1 - a)) & 1;
            blo[a] = up ? mid[a] - A.g.mg[a] : cblo[a];
            bhi[a] = up ? cbhi[a] : mid[a] + A.g.mg[a];
        }
    };
    if (tid < NSUB) { okey[tid] = ~0u; omask[tid] = 0ull; }
    __syncthreads();
    // (sub-cell o, list position j) pairs: reference = a candidate nearest
    // the sub-cell's centre (LDS atomic min of the key of the candidate lists. children)
    const int np = NSUB * mm;
    for (int p = tid; p < np; p += TPB) {
        const int o = p / mm, j = p - o * mm;
        double blo[MAXD], bhi[MAXD];
        sub_box(o, blo, bhi);
        const float4 c = crec[j];
        float dsum = 0.f;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const float dd = (float)(0.5 * (blo[a] + bhi[a])) - comp(c, a);
            dsum += dd * dd;
        }
        atomicMin(&okey[o], (__float_as_uint(dsum) & ~0x3Fu) | (uint32_t)j);
    }
    __syncthreads();
    for (int p = tid; p < np; p += TPB) {
        const int o = p / mm, j = p - o * mm;
        double blo[MAXD], bhi[MAXD];
        sub_box(o, blo, bhi);
        uint32_t bl = okey[o] & 0x3Fu;
        if (bl >= (uint32_t)mm) bl = 0;
        if (!prunable<D>(blo, bhi, crec[j], crec[bl])) atomicOr(&omask[o], 1ull << j);
    }
    __syncthreads();
    if (tid < nr) {
        const unsigned rb = base0 + (unsigned)tid * 4u * TPB;
        const unsigned rbeg = rb > start ? rb : start;
        const unsigned rend = rb + 4u * TPB < end ? rb + 4u * TPB : end;
        unsigned long long m = 0ull;
#pragma unroll
        for (int o = 0; o < NSUB; ++o)
            if (ss[o] < rend && ss[o + 1] > rbeg) m |= omask[o];
        rmask[tid] = m;
    }
    __syncthreads();
}

// Slot zeroing: only the rows the fold reads (16-byte stores, once the list's
// length mm is in) -- never the junk slot, which is written and never read.
template <int D, int LS>
__device__ __forceinline__ void lloyd1_zero_live(uint32_t *acc, int mm, int tid) {
    // the rows the fold reads: winners with a lane slot land in slots below
    // min(mm, LS) on every path (short list: position; slot map: rank < LS;
    // all-K scan: centroid < min(K, LS)); everything else goes to the junk slot
    const int nz = (mm < LS ? mm : LS) * (D + 1) * (AW / 4);
    uint4 *const a4 = reinterpret_cast<uint4 *>(acc);
    for (int e = tid; e < nz; e += TPB) a4[e] = make_uint4(0u, 0u, 0u, 0u);
}

// CROWD: the crowded-layout instance (tile lists, long lists, AccL::gwords of
// dynamic LDS); the other instances compile without that code.
template <typename T, int D, int LS, bool MASK, bool CROWD = false>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(lloyd1_wpe_c<T, D, LS, MASK, CROWD>(), 8))) void k_lloyd1(
    LloydArgs A, const uint4 *__restrict__ tiles, const float4 *__restrict__ fc_rec, const int32_t *__restrict__ fc_lab,
    const float4 *__restrict__ Call, const uint32_t *__restrict__ fc_cnt, const float4 *__restrict__ tl_rec) {
    extern __shared__ __attribute__((aligned(16))) uint32_t acc[];   // [(LS+1)*(D+1)][AW]
    // crowded layouts stage tile lists of up to TLCAP records in LDS (the long
    // lists of clustered clouds scan from LDS instead of one scalar load per
    // candidate) and sum list positions >= LS into the block-shared int64 words
    // AccL::gwords (one global atomic per word and tile at the end, not one per point)
    constexpr int LCAP = CROWD ? TLCAP : CAPF;
    __shared__ float4 crec[LCAP];
    __shared__ int32_t cid[LCAP];
    // Lists longer than LS: the LS candidates nearest the tile's centre own the
    // lane slots (smap: list position -> slot; sid: slot -> centroid), the
    // rest sum into int64 words per list position -- global atomics (rare
    // positions), AccL::gwords when
    // crowded.  Points mostly pick a candidate near their tile, so the lane
    // slots take nearly all of them whatever the list's length.
    // (D <= 3, 8 slots: lists past 8 are rare on the fine grids that take 8
    // slots, so their overflow goes to global atomics; dropping the 2 KB of LDS
    // words, 13.0 -> 10.9 KB per block, gave config 3's assign 203.6-204.3 ->
    // 199.3-199.6 us on one box, round 5, profiles/rd5_lds_ovf_ab.txt; the D = 4
    // 8-slot instances' LDS words went the same way, profiles/rd5_d4_wpe6_ab.txt)
    __shared__ uint16_t smap[LCAP];
    __shared__ float skey[LCAP];
    __shared__ int32_t sid[LS];
    const int tid = threadIdx.x;
    const unsigned t = A.xcd ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
    // the gate flags, the device tile count and the tile record are loaded
    // together (one memory latency, not three in a row): the tiles buffer holds
    // ntiles_cap >= gridDim.x records, so the record load is in bounds before
    // the count says whether this block has work
    uint4 tr = tiles[t];
    unsigned nt = *A.ntiles;
    unsigned gate = A.ctrl->halt | A.ctrl->done;
    // the tile's layout-time sums (uniform: scalar loads beside the record's): used
    // only when the owner word is set, loaded here so that such a tile costs one
    // latency in all
    long long ts[D];
#pragma unroll
    for (int a = 0; a < D; ++a) ts[a] = A.tsum[(size_t)t * D + a];
    constexpr bool ZOK = sizeof(T) == 4 && D == 3;   // compressed tiles exist only for fp32 D = 3
    uint4 zm = make_uint4(0u, 0u, 0u, 0u);
    if (ZOK && A.tmeta) zm = A.tmeta[t];
    asm volatile("" : "+s"(tr.x), "+s"(tr.y), "+s"(tr.z), "+s"(tr.w), "+s"(nt), "+s"(gate));   // keep the loads above the exits
    asm volatile("" : "+s"(zm.x), "+s"(zm.y), "+s"(zm.z), "+s"(zm.w));
#pragma unroll
    for (int a = 0; a < D; ++a) asm volatile("" : "+s"(ts[a]));
    if (gate != 0u || t >= nt) return;
    DBG_L(0);
    DBG_LV(5, __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)));    // HW_REG_HW_ID, 32 bits
    DBG_LV(6, __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (15 << 11)));   // HW_REG_XCC_ID, 16 bits
    const unsigned cell = tr.x, start = tr.y, end = tr.z;
    // ---- phase 1: the sole-owner exit
    if (tr.w != 0u) {   // block-uniform: a sole-owner tile (SoleW), no list or point load is issued
        lloyd1_sole_owner<D>(A.stats, tr.w, start, end, ts, tid);
        return;
    }
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f);
    int l0 = 0;
    if (tid < LSPEC) {
        r0 = fc_rec[(size_t)cell * CAPF + tid];
        l0 = fc_lab[(size_t)cell * CAPF + tid];
    }
    uint32_t cnt = fc_cnt[cell];
    // Lean rounds (below) exist in the 8-slot instances that keep their parent's
    // waves per SIMD with them: not fp16 D = 3 and 4 (64 -> 69 and 72 VGPRs,
    // 8 -> 7 waves) nor the D = 4 16-slot instance (fp32 80 -> 101 VGPRs, 6 -> 4).
    constexpr bool kFast = !MASK && !CROWD && LS < LSLOT && !(sizeof(T) == 2 && D >= 3);
    DBG_LV(7, (unsigned long long)(cnt & 0xFFFFu) | ((unsigned long long)(end - start) << 16));
    // crowded cell (list FULL or past TL_MIN): the tile's own list when k_tile_cand built a shorter one
    // (lists past TLCAP and all-K scans go through LDS in chunks, below)
    const float4 *lrec = fc_rec + (size_t)cell * CAPF;
    const int32_t *llab = fc_lab + (size_t)cell * CAPF;
    bool tl = false;
    if (CROWD && cnt > TL_MIN) {
        const uint32_t tc = A.tl_cnt[t];
        if (tc != FULL) {
            cnt = tc;
            lrec = tl_rec + (size_t)t * TLMAX;
            llab = A.tl_lab + (size_t)t * TLMAX;
            tl = true;
        }
    }
    constexpr int NSUB = 1 << D;
    uint32_t ss[NSUB + 1];   // the cell's sub-cell starts (uniform: scalar loads)
#pragma unroll
    for (int o = 0; o <= NSUB; ++o) ss[o] = (MASK && A.sub) ? A.sub_start[((size_t)cell << D) + o] : 0u;
    const unsigned base0 = start & ~3u;
    const int nr = (int)((end - base0 + 4 * TPB - 1) / (4 * TPB));
    const rsrc_t rx = make_rsrc(A.xs, (unsigned long long)A.npad * D * sizeof(T));
    // compressed tile (k_tile_compress): 8-B records from xz, decoded exactly
    const bool zc = ZOK && (zm.w >> 31);
    const unsigned zw0 = zm.w & 0xffu, zw1 = (zm.w >> 8) & 0xffu, zw2 = (zm.w >> 16) & 0xffu;
    const unsigned zsh1 = zw0, zsh2 = 32u - zw2;
    const unsigned zm0 = (1u << zw0) - 1u, zm1 = (1u << zw1) - 1u;
    const unsigned bpp = zc ? 8u : (unsigned)(D * sizeof(T));
    const rsrc_t rA = make_rsrc(zc ? (const void *)A.xz : A.xs, (unsigned long long)(zc ? (A.npad + 255) / 256 * 256 : A.npad) * bpp);
    // lanes past the tile's end get the out-of-range offset: zeros, no memory traffic
    auto item_off = [&](int rr) -> unsigned {
        const unsigned o = base0 + (unsigned)rr * 4u * TPB + 4u * tid;
        return (rr < nr && o < end) ? o : 0x0ffffff0u;
    };
    __shared__ unsigned long long omask[NSUB];
    __shared__ uint32_t okey[NSUB];
    __shared__ unsigned long long rmask[TILE / (4 * TPB) + 1];   // rounds of one tile
    // The rest of the kernel, instantiated per point format: compressed tiles
    // (fp32 D = 3, 8-B records) issue 2 b128 loads per work item, raw tiles
    // D * sizeof(T) / 4 -- one constant load count per instance keeps hipcc's
    // waitcnt bookkeeping exact, and compressed items no longer issue a third,
    // out-of-range load just to match the raw path's count.
    auto body = [&](auto ZCc) {
    constexpr bool ZC = decltype(ZCc)::value;
    auto ldx = [&](Raw<T, D> &dst, unsigned off) {
        if constexpr (ZC) load_z2(dst, rA, off);
        else load_x<T, D>(dst, rx, off);
    };
    // work items r+1 .. r+PF in flight while item r is computed: a ring of PF+1
    // register sets (compile-time indices after unrolling)
    constexpr int PF = ZC ? ZPF : 2;
    Raw<T, D> xr[PF + 1];
#pragma unroll
    for (int k = 0; k < PF; ++k) ldx(xr[k], item_off(k));
    // ---- phase 2: slot zeroing + list staging (the staging inline: as a function it moved the registers
    // of 21 of the 32 instances, e.g. fp16 D = 1 masked 79 -> 100 SGPRs, fp32 D = 3 masked 97 -> 101 VGPRs)
    // (not the crowded D = 1 instances: the later zeroing took them from 99 to 103 SGPRs, 8 -> 7 waves)
    constexpr bool kZeroLive = !(CROWD && D == 1);
    if constexpr (!kZeroLive)
        for (int e = tid; e < AccL<D, LS>::words; e += TPB) acc[e] = 0u;
    // long tile lists: block-shared int64 words per list position (AccL::gwords, crowded launches only)
    unsigned long long *const govf =
        reinterpret_cast<unsigned long long *>(acc + (AccL<D, LS>::words + 1) / 2 * 2);
    const bool full = (cnt == FULL);
    const int mm = (cnt == FULL) ? A.K : (int)cnt;
    // crowded: an all-K scan or a tile list longer than the LDS list: scanned in
    // LDS chunks (below), no list staging
    const bool chunked = CROWD && (full || mm > LCAP);
    // block-uniform: the list is longer than the lane slots (not an all-K scan)
    const bool use_map = !full && !chunked && mm > LS;
    // block-uniform: a winner can lack a lane slot only in an all-K scan or a
    // list longer than the slots (the per-round test below is skipped otherwise)
    const bool can_over = full || mm > LS;
    if constexpr (kZeroLive) lloyd1_zero_live<D, LS>(acc, mm, tid);
    if (full || chunked) {
        if (tid < LS) sid[tid] = tid;
        // (crowded: positions >= LS of an all-K scan go to global atomics, as the 16-slot variant's)
    } else {
        if (tid < LSPEC && tid < mm) {
            int lab = l0;
            if (tl) {   // block-uniform: crowded cells only (r0/l0 hold the cell list)
                crec[tid] = lrec[tid];
                lab = llab[tid];
            } else {
                crec[tid] = r0;
            }
            cid[tid] = lab;
            if (!use_map) sid[tid] = lab;   // short list: position p owns lane slot p
        }
        for (int j = LSPEC + tid; j < mm; j += TPB) {   // long lists (rare at D <= 3)
            crec[j] = lrec[j];
            cid[j] = llab[j];
        }
        if (CROWD && use_map)
            for (int j = tid; j < mm * (D + 1); j += TPB) govf[j] = 0ull;
    }
    uint32_t *const myacc = acc + (tid & (AW - 1));
    unsigned long long *prep = A.stats;
    __syncthreads();
    // ---- phase 3: the crowded chunked scan (the whole tile: it returns; inline: as a function one copy of
    // htag served both point formats, 8768 -> 7744 B of LDS, and fp16 D = 3 went 74 -> 76 SGPRs)
    if constexpr (CROWD) {
        if (chunked) {   // block-uniform
            // Crowded tile with a list longer than TLCAP (up to TLMAX), or FULL (no
            // list: every centre): the candidates are staged through LDS in chunks
            // of TLCAP -- the scalar-load scan of a 64-KB centre array missed the
            // scalar cache every few candidates (~2 ms per 4096-point tile at
            // K = 4096) -- in ascending centroid index with the strict '<' of scan4
            // (ties: lowest index).  Winners sum into a direct-mapped LDS table of
            // int64 words (govf, TLCAP entries tagged with the centroid; a slot
            // taken by another centroid sends the point to global atomics), folded
            // into the statistics once at the end.
            constexpr uint32_t EMPTY = 0xFFFFFFFFu;
            __shared__ uint32_t htag[TLCAP];
            for (int h = tid; h < TLCAP; h += TPB) htag[h] = EMPTY;
            for (int e = tid; e < TLCAP * (D + 1); e += TPB) govf[e] = 0ull;
            const rsrc_t rxf = make_rsrc(A.xs, (unsigned long long)A.npad * D * sizeof(T));
            for (int r = 0; r < nr; ++r) {
                const unsigned rbase = base0 + (unsigned)r * 4u * TPB;
                const unsigned i0 = rbase + 4u * tid;
                const unsigned off = (i0 < end) ? i0 : 0x0ffffff0u;
                float x[4][D];
                if constexpr (ZOK) {
                    Raw<float, 3> raw;
                    if (zc) {
                        load_z2(raw, rA, off);
                        unpack_z(raw, x, zm, zsh1, zsh2, zm0, zm1);
                    } else {
                        load_x<float, 3>(raw, rxf, off);
                        unpack_x<3>(raw, x);
                    }
                } else {
                    Raw<T, D> raw;
                    load_x<T, D>(raw, rxf, off);
                    unpack_x<D>(raw, x);
                }
                float bd[4];
                int bj[4];
                for (int c0 = 0; c0 < mm; c0 += TLCAP) {
                    const int mc = min(TLCAP, mm - c0);
                    __syncthreads();   // the previous chunk has been scanned
                    if (full) {
                        for (int j = tid; j < mc; j += TPB) { crec[j] = Call[c0 + j]; cid[j] = c0 + j; }
                    } else {
                        for (int j = tid; j < mc; j += TPB) { crec[j] = lrec[c0 + j]; cid[j] = llab[c0 + j]; }
                    }
                    __syncthreads();
                    int j = 0;
                    if (c0 == 0) {
                        const float4 c = crec[0];
                        const int cj = cid[0];
                        for (int e = 0; e < 4; ++e) { bd[e] = dist_canon<D>(x[e], c); bj[e] = cj; }
                        j = 1;
                    }
                    for (; j < mc; ++j) {
                        const float4 c = crec[j];
                        const int cj = cid[j];
                        for (int e = 0; e < 4; ++e) {
                            const float dd = dist_canon<D>(x[e], c);
                            const bool lt = dd < bd[e];
                            bd[e] = lt ? dd : bd[e];
                            bj[e] = lt ? cj : bj[e];
                        }
                    }
                }
                for (int e = 0; e < 4; ++e) {
                    if (!((i0 + e >= start) && (i0 + e < end))) continue;
                    const uint32_t h = (uint32_t)bj[e] & (uint32_t)(TLCAP - 1);
                    const uint32_t old = atomicCAS(&htag[h], EMPTY, (uint32_t)bj[e]);
                    if (old == EMPTY || old == (uint32_t)bj[e]) add_point_row<D>(govf + h * (D + 1), x[e], A.q);
                    else add_point_row<D>(prep + (size_t)bj[e] * (D + 1), x[e], A.q);
                }
            }
            __syncthreads();
            for (int i = tid; i < TLCAP * (D + 1); i += TPB) {
                const uint32_t c = htag[i / (D + 1)];
                const unsigned long long w = govf[i];
                if (c != EMPTY && w) atomicAdd(prep + (size_t)c * (D + 1) + i % (D + 1), w);
            }
            return;
        }
    }
    // ---- phase 4: the slot-map ranking (inline: as a function the crowded fp16 D = 3 pair went 76 / 74 -> 72 SGPRs)
    if (use_map) {
        // rank the list by the fp32 squared distance of each candidate to the
        // tile's centre (ties by position): ranks < LS get the lane slots
        float ctr[D];
        if (CROWD && tl && A.tbox) {   // crowded tile: its exact point box
            const float4 blo = A.tbox[(size_t)t * 2], bhi = A.tbox[(size_t)t * 2 + 1];
#pragma unroll
            for (int a = 0; a < D; ++a) ctr[a] = 0.5f * (comp(blo, a) + comp(bhi, a));
        } else {   // the cell's centre
            int ci[MAXD];
            for (int a = D - 1, c = (int)cell; a >= 0; --a) {
                ci[a] = (int)((unsigned)c % (unsigned)A.g.G[a]);
                c = (int)((unsigned)c / (unsigned)A.g.G[a]);
            }
#pragma unroll
            for (int a = 0; a < D; ++a) ctr[a] = (float)(A.g.lo[a] + ((double)ci[a] + 0.5) * A.g.w[a]);
        }
        // (kept rolled: interleaved eight-fold this rare loop held 24 VGPRs, the peak of the fp32 D = 3
        // instance: 71 -> 69)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int j = tid; j < mm; j += TPB) skey[j] = dist_canon<D>(ctr, crec[j]);
        __syncthreads();
        for (int j = tid; j < mm; j += TPB) {
            const float kj = skey[j];
            int rank = 0;
            for (int q = 0; q < mm; ++q) {
                const float kq = skey[q];
                rank += (kq < kj || (kq == kj && q < j)) ? 1 : 0;
            }
            smap[j] = (uint16_t)(rank < LS ? rank : LS + j);
            if (rank < LS) sid[rank] = cid[j];
        }
        __syncthreads();
    }
    // ---- phase 5: the per-round sub-cell masks
    const bool use_mask = MASK && A.sub && !full && !tl && mm >= MASK_MIN && A.g.prune;
    if (use_mask) lloyd1_round_masks<D>(A, cell, mm, nr, base0, start, end, ss, crec, okey, omask, rmask, tid);
    DBG_L(1);

    // ---- phase 6: the rounds (step: nearest candidate, then lean or generic accumulation; all inline: the
    // generic one as a function took the crowded fp32 D = 2 pair 55 -> 56 VGPRs; nearest, lean and the fold
    // as functions kept every register figure but measured slower, profiles/phases_ab.txt)
    // loads per work item; after item r+PF's are issued, items r+1 .. r+PF may
    // stay outstanding while r is computed
    constexpr int NL = ZC ? 2 : Raw<T, D>::NW / 4 + (Raw<T, D>::NW % 4 ? 1 : 0);
    constexpr int VM = PF * NL;
    constexpr int WAIT_PREV = 0x0F70 | (VM & 0xF) | ((VM >> 4) << 14);   // vmcnt(VM) expcnt(7) lgkmcnt(15)
    // lean: a list no longer than the lane slots (never an all-K scan; never
    // MASK or CROWD, so no masks, tile lists or chunks): list position = lane
    // slot, so a round skips everything that exists for winners without a
    // slot -- the slot map, the `sm >= LS` test, the `over` reduction, the
    // int64 words.  Block-uniform, decided once per block; the generic code
    // serves every other tile, and every tile when PCM_FAST=0.
    const bool lean = kFast && A.fast && !can_over;
    // The rounds in which this wave has a point of the tile (wave-uniform, in a
    // scalar register).  A wave covers 256 of a round's points, and base0 <= start
    // < base0 + 4, so its rounds are 0 .. nrw - 1: of a last round that holds a
    // few dozen points the upper wave owns none, and a tile below 256 points
    // gives it no round at all.  It takes the padding step there -- there is
    // no barrier inside the round loop -- and its loop ends at nrw.
    // PCM_TILECOST=0: nrw = nr, every wave computes every round.
    const unsigned wfirst = base0 + (unsigned)__builtin_amdgcn_readfirstlane((tid >> 6) * (4 * 64));
    const int nrw = !A.tilecost ? nr : (end > wfirst ? (int)((end - wfirst + 4 * TPB - 1) / (4 * TPB)) : 0);
    auto step = [&](Raw<T, D> &cx, Raw<T, D> &nx, int r) {
        ldx(nx, item_off(r + PF));
        if (r >= nrw) {
            // padding step (nr not a multiple of 3, or a round in which this
            // wave has no point): no compute, but the same
            // wait as a computing step, so that every path reaches the loop
            // latch with the same outstanding loads (a skipped step left the
            // waitcnt pass a pessimistic merge: vmcnt(0) before each prefetch)
            __builtin_amdgcn_s_waitcnt(WAIT_PREV);
            return;
        }
        const unsigned rbase = base0 + (unsigned)r * 4u * TPB;
        const unsigned i0 = rbase + 4u * tid;
        float x[4][D];
        if constexpr (ZC) unpack_z(cx, x, zm, zsh1, zsh2, zm0, zm1);
        else unpack_x<D>(cx, x);
        int bj[4];
        if (mm == 1) {
            for (int e = 0; e < 4; ++e) bj[e] = 0;
        } else if (use_mask) {
            const unsigned long long m0 = rmask[r];
            const unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m0 >> 32)) << 32) |
                                         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m0);
            if ((m & (m - 1ull)) == 0ull) {   // one candidate for the whole round
                const int j = m ? __builtin_ctzll(m) : 0;
                for (int e = 0; e < 4; ++e) bj[e] = j;
            } else {
                float bd[4];
                scan4_m<D>(crec, m, x, bd, bj);
            }
        } else {
            float bd[4];
            if (full) {
                scan4_s<D>(Call, mm, x, bd, bj);
            } else {
                scan4<D>(crec, mm, x, bd, bj);
            }
        }
        if (kFast && lean) {
            // list position = lane slot.  A round that lies wholly inside the
            // tile (block-uniform; all but a tile's first and last) takes the
            // slot address straight from the winner; the others send their
            // out-of-tile points to the junk slot.  Neither arm issues or waits
            // for a point load, so both reach the loop latch with the same
            // outstanding loads (see the padding step above).
            auto add4 = [&](const int (&sl)[4]) {
                for (int e = 0; e < 4; ++e) {
                    uint32_t *ap = myacc + sl[e] * ((D + 1) * AW);
                    for (int a = 0; a < D; ++a) atomicAdd(ap + a * AW, (uint32_t)fixed_i(x[e][a], A.q[a]));
                    atomicAdd(ap + D * AW, 1u);
                }
            };
            const bool whole = (rbase >= start) && (rbase + 4u * TPB <= end);
            if (whole) {
                add4(bj);
            } else {
                int sl[4];
                for (int e = 0; e < 4; ++e) sl[e] = ((i0 + e >= start) && (i0 + e < end)) ? bj[e] : LS;
                add4(sl);
            }
            return;
        }
        // block-uniform: every point of the round lies inside the tile
        const bool whole = (rbase >= start) && (rbase + 4u * TPB <= end);
        // slot of each point's winner: its lane slot (< LS), else LS + its list
        // position (use_map) or, in an all-K scan, LS + (centroid - LS)
        int sl[4], so[4];
        bool over = false;
        for (int e = 0; e < 4; ++e) {
            const bool v = whole || ((i0 + e >= start) && (i0 + e < end));
            const int sm = use_map ? (int)smap[bj[e]] : bj[e];
            const bool hi = sm >= LS;
            over |= v && hi;
            sl[e] = (v && !hi) ? sm : LS;
            so[e] = (v && hi) ? (use_map ? sm - LS : bj[e]) : -1;
        }
        for (int e = 0; e < 4; ++e) {
            uint32_t *ap = myacc + sl[e] * ((D + 1) * AW);
            for (int a = 0; a < D; ++a) atomicAdd(ap + a * AW, (uint32_t)fixed_i(x[e][a], A.q[a]));
            atomicAdd(ap + D * AW, 1u);
        }
        if (can_over && over) {   // winners without a lane slot (long lists only)
            for (int e = 0; e < 4; ++e) {
                const int o = so[e];   // list position (use_map) or centroid (all-K scan)
                if (o < 0) continue;
                if (CROWD && !full) add_point_row<D>(govf + o * (D + 1), x[e], A.q);   // crowded list: block-shared words, folded at the end
                else add_point_row<D>(prep + (size_t)(full ? o : cid[o]) * (D + 1), x[e], A.q);
            }
        }
    };
    // PF+1 rotating register sets; a tile spans at most TILE / (4 TPB) + 1 = 9 rounds
    for (int r = 0; r < nrw; r += PF + 1) {
#pragma unroll
        for (int k = 0; k <= PF; ++k) step(xr[k], xr[(k + PF) % (PF + 1)], r + k);
    }
    DBG_L(2);
    // ---- phase 7: the fold of the slot words into the int64 statistics, 16 threads per (slot, a) row
    __syncthreads();
    static_assert(AW == 64, "the fold reads a row as 16 lanes x one 16-byte load (a DPP row of 16 lanes)");
    const int nslots = mm < LS ? mm : LS;
    const int npairs = nslots * (D + 1);
    // thread `sub` of a row takes words 4 sub .. 4 sub + 3 (any partition of
    // the 64 words is the same integer sum).  w = (w >> 16) * 2^16 +
    // (w & 0xffff) with an arithmetic shift; 64 low halves sum below 2^22
    // and 64 high halves within +-2^21, so both int32 sums are exact, and
    // the row's last lane rebuilds the int64 sum.  Count words are <= 64,
    // so reading them as signed changes nothing.
    for (int p0 = 0; p0 < npairs; p0 += TPB / 16) {
        const int pi = p0 + tid / 16, sub = tid & 15;
        int lo = 0, hi = 0;
        if (pi < npairs) {
            const uint4 w = reinterpret_cast<const uint4 *>(acc + pi * AW)[sub];
            lo = (int)((w.x & 0xffffu) + (w.y & 0xffffu) + (w.z & 0xffffu) + (w.w & 0xffffu));
            hi = ((int32_t)w.x >> 16) + ((int32_t)w.y >> 16) + ((int32_t)w.z >> 16) + ((int32_t)w.w >> 16);
        }
        lo = row16_sum_last(lo);
        hi = row16_sum_last(hi);
        const long long sacc = (long long)hi * 65536 + (long long)lo;
        if (pi < npairs && sub == 15 && sacc) {
            const int slot = pi / (D + 1), qq = pi % (D + 1);
            atomicAdd(prep + (size_t)sid[slot] * (D + 1) + qq, (unsigned long long)sacc);
        }
    }
    // the int64 words of the positions without a lane slot (use_map lists)
    if (CROWD && use_map)
        for (int i = tid; i < mm * (D + 1); i += TPB) {
            const unsigned long long w = govf[i];
            if (w) atomicAdd(prep + (size_t)cid[i / (D + 1)] * (D + 1) + i % (D + 1), w);
        }
    DBG_L(3);
    };
    if constexpr (ZOK) {
        if (zc) body(std::true_type{});
        else body(std::false_type{});
    } else {
        body(std::false_type{});
    }
}

}  // namespace pcm
