// pcm_cand.hpp (a part of pcm_kernels.hpp) — exact candidate lists per grid cell (k_cand, k_coarse, refresh)
#pragma once
#include "pcm_kcommon.hpp"

namespace pcm {

// ------------------------------------------------------------------ candidates
// Candidate lists of every fine cell, in one launch, without global-memory
// round trips inside the per-cell work.  Block (I, b) owns coarse cell I
// (F^D fine cells) and children [b*cpb, (b+1)*cpb):
//  1. coarse list (block-wide, into LDS): reference r = a centre minimising the
//     max distance to the coarse box (LDS atomic min of a packed key: any centre
//     is a valid reference, the choice only affects pruning power); every
//     centre not provably dominated by r is marked in an LDS bitmap, and one
//     wave compacts the bitmap in ascending centroid index.  More than CAPC
//     survivors -> all K (FULL parent);
//  2. one wave per child cell: reference = a parent candidate nearest the cell
//     centre (again an LDS atomic-min key), keep the parent candidates it does
//     not dominate, in ascending centroid order (the scan's tie rule); the count
//     goes to fc_cnt[cell] (FULL = more than CAPF, or pruning disabled).
// D = 4: a coarse cell has 4^4 = 256 fine cells and a longer coarse list
template <int D> constexpr int cand_capc() { return D >= 4 ? 1024 : CAPC; }
#ifndef PCM_CAND_TPB
#define PCM_CAND_TPB 512   // round-2 fused update at config 3: 25.7 vs 28.7 us (the pair passes are latency-bound)
#endif
constexpr int CAND_TPB = PCM_CAND_TPB;   // threads per candidate block (one child cell per wave at a time)
constexpr int CAND_KBITS = 4096;         // bitmap capacity (larger K: direct ballot compaction)
constexpr int CAND_CBW = 512;            // pair path: child bitmap words (4 KB)
constexpr int CAND_MAXCH = 64;           // pair path: children per block


// Wave-wide minimum through DPP (row_shr 1/2/4/8 scan, then row_bcast 15/31;
// lane 63 ends with the minimum).  The whole wave must be active.  Used only to
// pick pruning references, where any candidate is correct (callers clamp).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    const int id = -1;   // 0xFFFFFFFF: the identity of unsigned min
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x111, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x112, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x114, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x118, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x142, 0xA, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x143, 0xC, 0xF, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// C: the K centres, in global memory (k_cand, k_lists, k_coarse).
// Coarse lists computed once per coarse cell (CoarseL, D = 4 layouts): k_coarse
// writes them (out); the blocks of the next level read them (in).
struct CoarseL {
    const uint32_t *in_cnt = nullptr;   // [ncoarse] list length or FULL
    const int32_t *in_idx = nullptr;    // [ncoarse][cand_capc] centroid ids, ascending
    uint32_t *out_cnt = nullptr;
    int32_t *out_idx = nullptr;
};
// FC: fine cells per axis of the block's cell.  FC = 4: a coarse cell (4^D
// children) whose list is computed from all K centres (or read from k_coarse);
// FC = 2: a mid cell (2^D children, D = 4 layouts) whose list REFINES its
// coarse parent's k_coarse list -- the same exact test against the mid box --
// so the fine lists prune ~2^D-times shorter lists than the coarse ones.
// Owner words (tiles[t].w): 0 = k_lloyd1 streams the tile; 1 + j = the tile's
// cell has the one-entry list {j}, so every point of it goes to centroid j
// whatever its coordinates and k_lloyd1 adds the tile's layout-time sums (tsum)
// instead of reading its points.  0 is always correct.  The thread that stores
// a cell's list length (pair path: thread `ch` of child ch, which loaded the
// cell's tile range before the passes so that no latency is left at the block's
// end) stores the word of each of the cell's tiles, on every
// list build (a longer list clears it; a refresh leaves the lists and so the
// words as they are).  tile_off: the layout's first tile of every cell; tpos:
// layout tile index -> current position once the tiles were reordered
// (k_tile_gather), else null.  Cells of more than SOLE_MAXT tiles keep the 0 of
// k_tile_write: the store loop of that one lane stays short (a cell holds
// SOLE_MAXT x TILE = 32768 points only when the grid is far too coarse for the
// cloud, where lists are long anyway).
constexpr uint32_t SOLE_MAXT = 8;
struct SoleW {
    uint4 *tiles = nullptr;             // null: the caller keeps no owner words
    const uint32_t *tile_off = nullptr;
    const uint32_t *tpos = nullptr;
    int on = 0;                         // 0: every word written is 0 (PCM_SOLE=0)
};
__device__ __forceinline__ void sole_store(const SoleW &sw, long long cell, uint32_t cnt, int label) {
    if (!sw.tiles) return;
    const uint32_t t0 = sw.tile_off[cell], t1 = sw.tile_off[cell + 1];
    if (t1 - t0 > SOLE_MAXT) return;
    const uint32_t w = (sw.on && cnt == 1u) ? 1u + (uint32_t)label : 0u;
    for (uint32_t t = t0; t < t1; ++t) sw.tiles[sw.tpos ? sw.tpos[t] : t].w = w;
}

template <int D, int FC = 4, int TPB = CAND_TPB>
__device__ __forceinline__ void cand_body(const Grid &g, const float4 *C, int K, uint32_t *__restrict__ fc_cnt,
                                          float4 *__restrict__ fc_rec, int32_t *__restrict__ fc_lab, int BPC,
                                          double dl = 0.0, CoarseL cl = CoarseL{}, SoleW sw = SoleW{}) {
    static_assert(FC == 4 || FC == 2, "children per axis");
    constexpr int CAP = cand_capc<D>();
    constexpr int FS = FC == 4 ? 2 : 1;   // log2(FC)
    const long long I = blockIdx.x / BPC;
    const int bsub = blockIdx.x % BPC;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ float4 prec[CAP];
    __shared__ int pidx[CAP];
    __shared__ int sidx[FC == 2 ? CAP : 1];   // refine: the coarse parent's list
    __shared__ unsigned long long kbits[CAND_KBITS / 64];
    __shared__ unsigned long long rkey;
    __shared__ uint32_t s_mp, s_np;
    __shared__ unsigned long long cbits[CAND_CBW];   // pair path: per-child keep bitmaps over the coarse list
    int ci[MAXD];
    long long Ipar = I;   // the coarse cell whose k_coarse list this block reads
    if (FC == 4) {
        decode(I, g.GC, D, ci);
    } else {
        int GM[MAXD], pc[MAXD];
        for (int a = 0; a < MAXD; ++a) GM[a] = a < D ? (g.G[a] + 1) / 2 : 1;
        decode(I, GM, D, ci);
        for (int a = 0; a < D; ++a) pc[a] = ci[a] / 2;
        Ipar = encode(pc, g.GC, D);
    }
    int nchild = 1;
    for (int a = 0; a < D; ++a) nchild *= FC;
    const int cpb = (nchild + BPC - 1) / BPC;
    const bool refine = FC == 2 && cl.in_cnt != nullptr;

    // ---- 1. this block's cell list
    if (cl.in_cnt && !refine) {   // computed by k_coarse for this iteration's centres
        for (int w = tid; w < CAND_CBW; w += TPB) cbits[w] = 0ull;
        if (tid == 0) s_mp = cl.in_cnt[I];
        __syncthreads();
        const uint32_t m0 = s_mp;
        if (m0 != FULL)
            for (uint32_t l = tid; l < m0; l += TPB) {
                const int j = cl.in_idx[(size_t)I * CAP + l];
                pidx[l] = j;
                prec[l] = C[j];
            }
    } else if (g.prune) {
        int f0[MAXD], f1[MAXD];
        for (int a = 0; a < D; ++a) {
            f0[a] = ci[a] * FC;
            f1[a] = min(f0[a] + FC, g.G[a]) - 1;
        }
        double blo[MAXD], bhi[MAXD];
        cell_box<D>(g, f0, f1, blo, bhi);
        // source candidates: every centre, or (refine) the coarse parent's list
        int nsrc = K;
        bool from_list = false;
        if (refine) {
            if (tid == 0) s_np = cl.in_cnt[Ipar];
            __syncthreads();
            const uint32_t m0 = s_np;
            if (m0 != FULL) {
                nsrc = (int)m0;
                from_list = true;
                for (int l = tid; l < nsrc; l += TPB) sidx[l] = cl.in_idx[(size_t)Ipar * CAP + l];
            }
        }
        auto src = [&](int p) -> int { return from_list ? sidx[p] : p; };
        const bool bitmap = nsrc <= CAND_KBITS;
        if (tid == 0) rkey = ~0ull;
        if (bitmap)
            for (int w = tid; w < CAND_KBITS / 64; w += TPB) kbits[w] = 0ull;
        for (int w = tid; w < CAND_CBW; w += TPB) cbits[w] = 0ull;
        __syncthreads();
        // reference key: fp32 bits of the max distance (any centre is a valid
        // reference; the key only ranks them) with the low 11 bits replaced by
        // j's wave-local rank -> per-wave DPP minimum, then one LDS atomic per wave
        uint32_t best = ~0u;
        int bjj = 0;
        for (int p = tid; p < nsrc; p += TPB) {
            const int j = src(p);
            const float m = (float)maxdist<D>(blo, bhi, C[j]);
            if (__float_as_uint(m) < best) { best = __float_as_uint(m); bjj = j; }
        }
        const uint32_t wbest = wave_min_u32(best);
        const unsigned long long bal = __ballot(best == wbest);
        if (lane == (int)(__ffsll((long long)bal) - 1)) atomicMin(&rkey, ((unsigned long long)wbest << 32) | (unsigned)bjj);
        __syncthreads();
        DBG_T(4);
        const float4 r = C[(int)min((unsigned long long)(K - 1), rkey & 0xFFFFFFFFull)];
        const double mr = dl > 0.0 ? sqrt(maxdist<D>(blo, bhi, r)) : 0.0;
        if (bitmap) {
            // a wave's 64 consecutive source positions fill one bitmap word: a
            // ballot and a plain store (no 64-way contended LDS atomic)
            for (int p0 = 0; p0 < nsrc; p0 += TPB) {
                const int p = p0 + tid;
                const bool keep = p < nsrc && !prunable<D>(blo, bhi, C[src(p < nsrc ? p : 0)], r, dl, mr);
                const unsigned long long bal = __ballot(keep);
                if (lane == 0 && p0 + wv * 64 < nsrc) kbits[(p0 >> 6) + wv] = bal;
            }
            __syncthreads();
            DBG_T(5);
            // ordered compaction (ascending source position = ascending centroid
            // index): word prefix counts by one wave-wide scan, then every wave
            // compacts the words w = wv (mod waves) in parallel
            __shared__ uint32_t wpre[CAND_KBITS / 64];
            const int nwk = (nsrc + 63) / 64;   // <= 64
            if (wv == 0) {
                const uint32_t c = lane < nwk ? (uint32_t)__popcll(kbits[lane]) : 0u;
                uint32_t x = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(x, o);
                    if (lane >= o) x += y;
                }
                wpre[lane] = x - c;
                if (lane == 63) s_mp = x <= (uint32_t)CAP ? x : FULL;
            }
            __syncthreads();
            for (int w = wv; w < nwk; w += TPB / 64) {
                const unsigned long long word = kbits[w];
                const uint32_t pos = wpre[w] + __popcll(word & ((1ull << lane) - 1ull));
                if (((word >> lane) & 1ull) && pos < (uint32_t)CAP) {
                    const int j = src(w * 64 + lane);
                    prec[pos] = C[j];
                    pidx[pos] = j;
                }
            }
        } else {
            // large K: ordered compaction by ballots (one barrier pair per TPB centres)
            __shared__ uint32_t wcnt[TPB / 64];
            uint32_t total = 0;
            for (int base = 0; base < nsrc; base += TPB) {
                const int p = base + tid;
                const int j = src(p < nsrc ? p : 0);
                const bool keep = p < nsrc && !prunable<D>(blo, bhi, C[j], r, dl, mr);
                const unsigned long long bal = __ballot(keep);
                if (lane == 0) wcnt[wv] = __popcll(bal);
                __syncthreads();
                uint32_t woff = 0;
                for (int w = 0; w < wv; ++w) woff += wcnt[w];
                const uint32_t pos = total + woff + __popcll(bal & ((1ull << lane) - 1ull));
                if (keep && pos < (uint32_t)CAP) {
                    prec[pos] = C[j];
                    pidx[pos] = j;
                }
                for (int w = 0; w < TPB / 64; ++w) total += wcnt[w];
                __syncthreads();
            }
            if (tid == 0) s_mp = total <= (uint32_t)CAP ? total : FULL;
        }
    } else if (tid == 0) {
        s_mp = FULL;
    }
    __syncthreads();
    uint32_t mp = s_mp;
    const bool pfull = (mp == FULL);
    if (cl.out_cnt) {   // k_coarse: publish the coarse list, no children
        if (tid == 0) cl.out_cnt[I] = mp;
        if (!pfull)
            for (uint32_t l = tid; l < mp; l += TPB) cl.out_idx[(size_t)I * CAP + l] = pidx[l];
        return;
    }
    if (pfull) mp = (uint32_t)K;
    DBG_T(1);
    DBG_V(8, mp);

    // ---- 2. children (FC per axis) of this block: c0 .. c1-1
    const int c0 = bsub * cpb, c1 = min(nchild, (bsub + 1) * cpb);
    const int nwc = (int)((mp + 63u) / 64u);   // bitmap words per child
    // pair path when each wave would otherwise walk >= 8 children one after the
    // other (100M: 64 children per block, 15 -> 9.6 us); with few children per
    // block (12.5M shard: 8) the wave path's two chains per wave are shorter
    // (mid blocks, FC = 2: 16 children over lists of tens to hundreds: the pair path too)
    if (!pfull && ((c1 - c0) >= 2 * TPB / 16 || FC == 2) && (c1 - c0) <= CAND_MAXCH &&
        (c1 - c0) * nwc <= CAND_CBW) {
        // Pair path: one thread per (child, coarse-list position) in three
        // block-wide passes -- (A) reference = a parent candidate nearest the
        // child's centre (LDS atomic min of the key of the wave path below),
        // (B) keep bits of the candidates that reference does not dominate,
        // (C) ordered compaction (ascending centroid index) by popcounts.  The
        // lists equal the wave path's; all pairs run in parallel instead of one
        // child per wave after another (100M: 15 -> ~2 us per block).
        const int nch = c1 - c0, npair = nch * (int)mp;
        const int dch = TPB / (int)mp, dlp = TPB % (int)mp;
        constexpr uint32_t LM = CAP > 256 ? 0x3FFu : 0xFFu;
        // (0) per-child cell id, fp64 box and centre, once per child
        __shared__ double s_blo[CAND_MAXCH][D], s_bhi[CAND_MAXCH][D];
        __shared__ float s_ctr[CAND_MAXCH][D];
        __shared__ long long s_cell[CAND_MAXCH];
        __shared__ float4 s_ref[CAND_MAXCH];   // the child's reference centre (pass A)
        __shared__ double s_mr[CAND_MAXCH];    // max distance from the child's box to it (drift budget > 0)
        // owner words: thread ch < nch (<= CAND_MAXCH < TPB: one child per thread) loads its
        // cell's tile range here and stores the words after pass (C), the latency hidden
        static_assert(CAND_MAXCH <= TPB, "one child per thread");
        uint32_t ot0 = 0u, ot1 = 0u;
        for (int ch = tid; ch < nch; ch += TPB) {
            int f[MAXD];
            bool inside = true;
#pragma unroll
            for (int a = D - 1, t = c0 + ch; a >= 0; --a, t >>= FS) {
                f[a] = ci[a] * FC + (t & (FC - 1));
                inside &= f[a] < g.G[a];
            }
            double blo[MAXD], bhi[MAXD];
            cell_box<D>(g, f, f, blo, bhi);
#pragma unroll
            for (int a = 0; a < D; ++a) {
                s_blo[ch][a] = blo[a];
                s_bhi[ch][a] = bhi[a];
                s_ctr[ch][a] = (float)(0.5 * (blo[a] + bhi[a]));
            }
            s_cell[ch] = inside ? encode(f, g.G, D) : -1ll;
            if (inside && sw.tiles) {
                const long long cell = encode(f, g.G, D);
                ot0 = sw.tile_off[cell];
                ot1 = sw.tile_off[cell + 1];
            }
        }
        __syncthreads();
        DBG_T(10);
        // (A) reference per child: TPC threads per child scan its share of
        // the coarse list, then a min over the TPC lanes (shuffles, no atomics:
        // an LDS atomic per pair serialised ~25-way on the child's word)
        {
            int tpc = 64;
            while (tpc > 1 && tpc * nch > TPB) tpc >>= 1;
            const int ch = tid / tpc, sub = tid % tpc;
            uint32_t best = ~0u;
            if (ch < nch && s_cell[ch] >= 0)
                for (int l = sub; l < (int)mp; l += tpc) {
                    const float4 c = prec[l];
                    float dsum = 0.f;
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        const float dd = s_ctr[ch][a] - comp(c, a);
                        dsum += dd * dd;
                    }
                    const uint32_t key = (__float_as_uint(dsum) & ~LM) | (uint32_t)l;
                    best = key < best ? key : best;
                }
            for (int o = 1; o < tpc; o <<= 1) {
                const uint32_t ob = (uint32_t)__shfl_xor((int)best, o);
                best = ob < best ? ob : best;
            }
            if (ch < nch && sub == 0 && s_cell[ch] >= 0) {
                uint32_t bl = best & LM;
                if (bl >= mp) bl = 0;
                const float4 r = prec[bl];
                s_ref[ch] = r;
                if (dl > 0.0) {
                    double blo[MAXD], bhi[MAXD];
#pragma unroll
                    for (int a = 0; a < D; ++a) { blo[a] = s_blo[ch][a]; bhi[a] = s_bhi[ch][a]; }
                    s_mr[ch] = sqrt(maxdist<D>(blo, bhi, r));
                } else {
                    s_mr[ch] = 0.0;
                }
            }
        }
        __syncthreads();
        DBG_T(11);
        // (B) keep bits; the lanes of one (child, bitmap word) are contiguous in a
        // wave, so one ballot and one LDS atomic per segment
        {
            const int iters = (npair + TPB - 1) / TPB;
            int ch = tid / (int)mp, l = tid % (int)mp;
            for (int it = 0, p = tid; it < iters; ++it, p += TPB) {
                bool keep = false;
                const bool valid = p < npair && s_cell[ch < nch ? ch : 0] >= 0 && ch < nch;
                if (valid) {
                    double blo[MAXD], bhi[MAXD];
#pragma unroll
                    for (int a = 0; a < D; ++a) { blo[a] = s_blo[ch][a]; bhi[a] = s_bhi[ch][a]; }
                    keep = !prunable<D>(blo, bhi, prec[l], s_ref[ch], dl, s_mr[ch]);
                }
                const unsigned long long bal = __ballot(keep);
                const int k = min(lane, l & 63);   // lanes before this one in its segment
                if (valid && k == 0) {
                    const int len = min(64 - lane, min(64 - (l & 63), (int)mp - l));
                    const unsigned long long seg = (bal >> lane) & (len >= 64 ? ~0ull : ((1ull << len) - 1ull));
                    if (seg) atomicOr(&cbits[ch * nwc + (l >> 6)], seg << (l & 63));
                }
                l += dlp;
                ch += dch;
                if (l >= (int)mp) { l -= (int)mp; ++ch; }
            }
        }
        __syncthreads();
        DBG_T(12);
        // (C)
        for (int p = tid, ch = tid / (int)mp, l = tid % (int)mp; p < npair; p += TPB) {
            const long long cell = s_cell[ch];
            if (cell >= 0) {
                const unsigned long long *wb = cbits + ch * nwc;
                const unsigned long long word = wb[l >> 6];
                uint32_t before = 0;
                for (int w = 0; w < (l >> 6); ++w) before += __popcll(wb[w]);
                if ((word >> (l & 63)) & 1ull) {
                    const uint32_t pos = before + __popcll(word & ((1ull << (l & 63)) - 1ull));
                    if (pos < (uint32_t)CAPF) {
                        fc_rec[cell * CAPF + pos] = prec[l];
                        fc_lab[cell * CAPF + pos] = pidx[l];
                    }
                }
                if (l == 0) {
                    uint32_t total = 0;
                    for (int w = 0; w < nwc; ++w) total += __popcll(wb[w]);
                    fc_cnt[cell] = total <= (uint32_t)CAPF ? total : FULL;
                }
            }
            l += dlp;
            ch += dch;
            if (l >= (int)mp) { l -= (int)mp; ++ch; }
        }
        if (sw.tiles && tid < nch && s_cell[tid] >= 0 && ot1 - ot0 <= SOLE_MAXT) {   // sole_store, ranges preloaded
            const unsigned long long *wb = cbits + tid * nwc;
            uint32_t total = 0;
            int first = 0;   // the lowest kept position: the owner of a one-entry list
            for (int w = nwc - 1; w >= 0; --w) {
                total += __popcll(wb[w]);
                if (wb[w]) first = w * 64 + __builtin_ctzll(wb[w]);
            }
            const uint32_t ow = (sw.on && total == 1u) ? 1u + (uint32_t)pidx[first] : 0u;
            for (uint32_t t = ot0; t < ot1; ++t) sw.tiles[sw.tpos ? sw.tpos[t] : t].w = ow;
        }
        DBG_T(2);
        return;
    }
    // wave path (FULL parent, or more pairs than the LDS bitmaps hold): one wave per child cell
    auto child = [&](auto PFc) {
        constexpr bool PF = decltype(PFc)::value;
        for (int ch = c0 + wv; ch < c1; ch += TPB / 64) {
            int f[MAXD];
            bool inside = true;
#pragma unroll
            for (int a = D - 1, t = ch; a >= 0; --a, t >>= FS) {
                f[a] = ci[a] * FC + (t & (FC - 1));
                inside &= f[a] < g.G[a];
            }
            if (!inside) continue;   // wave-uniform
            const long long cell = encode(f, g.G, D);
            if (!g.prune) {
                if (lane == 0) {
                    fc_cnt[cell] = FULL;
                    sole_store(sw, cell, FULL, 0);
                }
                continue;
            }
            double blo[MAXD], bhi[MAXD];
            cell_box<D>(g, f, f, blo, bhi);
            float ctr[MAXD];
#pragma unroll
            for (int a = 0; a < D; ++a) ctr[a] = (float)(0.5 * (blo[a] + bhi[a]));
            // reference: a parent candidate nearest the centre
            int bl;
            if constexpr (PF) {   // exact wave argmin (K may exceed a packed key's index field)
                float bd = __builtin_inff();
                bl = 0x7fffffff;
                for (uint32_t l = lane; l < mp; l += 64) {
                    const float4 c = C[l];
                    float dsum = 0.f;
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        const float dd = ctr[a] - comp(c, a);
                        dsum += dd * dd;
                    }
                    if (dsum < bd) { bd = dsum; bl = (int)l; }
                }
                for (int sft = 32; sft > 0; sft >>= 1) {
                    const float ob = __shfl_xor(bd, sft);
                    const int ol = __shfl_xor(bl, sft);
                    if (ob < bd || (ob == bd && ol < bl)) { bd = ob; bl = ol; }
                }
            } else {   // key = distance bits (low bits dropped) | list position (< CAP)
                uint32_t best = ~0u;
                for (uint32_t l = lane; l < mp; l += 64) {
                    const float4 c = prec[l];
                    float dsum = 0.f;
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        const float dd = ctr[a] - comp(c, a);
                        dsum += dd * dd;
                    }
                    const uint32_t key = (__float_as_uint(dsum) & (CAP > 256 ? 0xFFFFFC00u : 0xFFFFFF00u)) | l;
                    best = key < best ? key : best;
                }
                bl = (int)(wave_min_u32(best) & (CAP > 256 ? 0x3FFu : 0xFFu));
                if (bl >= (int)mp) bl = 0;
            }
            const float4 r = PF ? C[bl] : prec[bl];
            const double mr = dl > 0.0 ? sqrt(maxdist<D>(blo, bhi, r)) : 0.0;
            uint32_t total = 0, first = 0;   // first: the lowest kept position (the owner of a one-entry list)
            for (uint32_t base = 0; base < mp; base += 64) {
                const uint32_t l = base + lane;
                const bool in = l < mp;
                const uint32_t lc = in ? l : (uint32_t)bl;
                const float4 c = PF ? C[lc] : prec[lc];
                const int j = PF ? (int)lc : pidx[lc];
                const bool keep = in && !prunable<D>(blo, bhi, c, r, dl, mr);
                const unsigned long long bal = __ballot(keep);
                const uint32_t pos = total + __popcll(bal & ((1ull << lane) - 1ull));
                if (keep && pos < (uint32_t)CAPF) {
                    fc_rec[cell * CAPF + pos] = c;
                    fc_lab[cell * CAPF + pos] = j;
                }
                if (total == 0u && bal) first = base + (uint32_t)__builtin_ctzll(bal);
                total += __popcll(bal);
            }
            if (lane == 0) {
                fc_cnt[cell] = total <= (uint32_t)CAPF ? total : FULL;
                sole_store(sw, cell, total, PF ? (int)first : pidx[first]);
            }
        }
    };
    if (pfull) child(std::integral_constant<bool, true>{});
    else child(std::integral_constant<bool, false>{});
    DBG_T(2);
}

// Standalone candidate lists, exact for the current centres C (drift budget 0;
// fit start, relocation resume, final E-step): the reference
// buffer cref[ctrl->ref_sel] := C so that k_upd measures drift from C.
template <int D, int FC = 4>
__global__ __launch_bounds__(CAND_TPB) void k_cand(Grid g, const float4 *__restrict__ C, int K,
                                              uint32_t *__restrict__ fc_cnt, float4 *__restrict__ fc_rec,
                                              int32_t *__restrict__ fc_lab, Ctrl *__restrict__ ctrl, int gate,
                                              int bpc, float4 *__restrict__ cref, CoarseL cl, SoleW sw) {
    if (gate && gated(ctrl)) return;
    float4 *ref = cref + (size_t)ctrl->ref_sel * K;
    for (long long j = blockIdx.x * (long long)CAND_TPB + threadIdx.x; j < K; j += (long long)gridDim.x * CAND_TPB)
        ref[j] = C[j];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctrl->budget = 0.0;
        if (gate) ctrl->rebuilds += 1u;   // lists rebuilt at a relocation resume
    }
    cand_body<D, FC>(g, C, K, fc_cnt, fc_rec, fc_lab, bpc, 0.0, cl, sw);
}

// Coarse lists only (one block per coarse cell), for the child blocks of
// k_cand / k_lists to read.  C: the centres the lists are for; lists: gate on
// the k_lists work flag (the iteration path) or 0 (k_cand's callers).
template <int D>
__global__ __launch_bounds__(CAND_TPB) void k_coarse(Grid g, const float4 *__restrict__ C, int K,
                                                const Ctrl *__restrict__ ctrl, int lists, uint32_t *__restrict__ cl_cnt,
                                                int32_t *__restrict__ cl_idx) {
    double dl = 0.0;
    if (lists) {
        unsigned halt = ctrl->halt;
        unsigned mode = ctrl->lists;
        dl = ctrl->lists_dl;
        asm volatile("" : "+s"(halt), "+s"(mode), "+s"(dl));
        if (halt != 0u || mode != 2u) return;   // only a rebuild needs coarse lists
    }
    CoarseL cl;
    cl.out_cnt = cl_cnt;
    cl.out_idx = cl_idx;
    cand_body<D>(g, C, K, nullptr, nullptr, nullptr, 1, dl, cl);
}

// Candidate records refreshed to the new centres (lists still valid under the
// drift budget): every fine cell's records, grid-stride over the cells with 16
// threads per cell, every load of a cell's count and ids issued in parallel.
template <int D, int TPB = CAND_TPB>
__device__ __forceinline__ void refresh_body(const Grid &g, const float4 *cn, const uint32_t *__restrict__ fc_cnt,
                                             float4 *__restrict__ fc_rec, const int32_t *__restrict__ fc_lab,
                                             unsigned nblk = 0u) {   // list blocks (0: gridDim.x)
    constexpr int PER = 16, CPB = TPB / PER;   // threads per cell, cells per block pass
    const int sub = (int)threadIdx.x % PER;
    const unsigned nb = nblk ? nblk : gridDim.x;
    for (long long cell = (long long)blockIdx.x * CPB + (int)threadIdx.x / PER; cell < g.ncells;
         cell += (long long)nb * CPB) {
        const uint32_t m = fc_cnt[cell];
        if (m == FULL) continue;
        for (uint32_t p = sub; p < m; p += PER) fc_rec[cell * CAPF + p] = cn[fc_lab[cell * CAPF + p]];
    }
}

}  // namespace pcm
