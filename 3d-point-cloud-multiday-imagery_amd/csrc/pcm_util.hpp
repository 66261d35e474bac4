// pcm_util.hpp (a part of pcm_kernels.hpp) — relocation, label/centre plumbing, synthesis, diagnostics, brute force and predict kernels
#pragma once
#include "pcm_kcommon.hpp"
#include "pcm_assign.hpp"

namespace pcm {

// ------------------------------------------------------------------ relocation
// This rank's m farthest points from their centre (_k_means_common.pyx:185-187)
// by an exact radix SELECT over unique 64-bit keys (no sort, no N-sized
// allocation: the keys live in the layout's scratch arena):
//   key = dist_bits << 32 | (0xffffffff - global index)   (distance desc, row asc)
// 8 passes pick the m-th largest key T one byte at a time (MSB first); then
// every point with key >= T writes its record (any order: k_reloc_apply ranks
// the records it receives).
template <typename T, int D, typename LT>
__global__ __launch_bounds__(256) void k_reloc_keys(const T *__restrict__ xs, long long n,
                                                    const LT *__restrict__ lab, const uint32_t *__restrict__ perm,
                                                    const float4 *__restrict__ C, long long gidx0,
                                                    const uint32_t *__restrict__ grows,
                                                    unsigned long long *__restrict__ keys) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[D];
    for (int a = 0; a < D; ++a) x[a] = to_f<T>(xs[xs_index<D>(i, a)]);
    float d = dist_canon<D>(x, C[(int)lab[i]]);
    const uint32_t r = perm[i];
    unsigned long long g = grows ? (unsigned long long)grows[r] : (unsigned long long)(gidx0 + r);
    keys[i] = ((unsigned long long)__float_as_uint(d) << 32) | (0xffffffffull - (g & 0xffffffffull));
}

struct RselState {
    unsigned long long prefix;    // selected high bytes of T
    unsigned long long m_rem;     // how many of the keys matching `prefix` still belong to the top m
    unsigned int hist[256];
    unsigned int count_out;
    unsigned int pad;
};

// Histogram of byte `pass` (0 = most significant) of the keys whose higher bytes equal the prefix.
inline __global__ __launch_bounds__(256) void k_rsel_hist(const unsigned long long *__restrict__ keys, long long n,
                                                   RselState *__restrict__ st, int pass) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const unsigned long long hmask = pass ? (~0ull << (64 - 8 * pass)) : 0ull;
    const unsigned long long prefix = st->prefix;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long k = keys[i];
        if ((k & hmask) == prefix) atomicAdd(&h[(k >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

// One thread: the byte value holding the m_rem-th largest matching key.
inline __global__ void k_rsel_pick(RselState *__restrict__ st, int pass) {
    if (threadIdx.x != 0) return;
    unsigned long long above = 0ull;
    int v = 255;
    for (; v > 0; --v) {
        if (above + st->hist[v] >= st->m_rem) break;
        above += st->hist[v];
    }
    st->prefix |= (unsigned long long)v << (56 - 8 * pass);
    st->m_rem -= above;
    for (int b = 0; b < 256; ++b) st->hist[b] = 0u;
}

struct RelocRec {
    unsigned long long key;
    int32_t label;
    int32_t valid;
    int32_t xq[4];
};

// Every point with key >= T (the top m; keys are unique) writes its record.
template <typename T, int D, typename LT>
__global__ __launch_bounds__(256) void k_reloc_gather(const unsigned long long *__restrict__ keys, long long n,
                                                      const T *__restrict__ xs, const LT *__restrict__ lab, QExp qe,
                                                      RselState *__restrict__ st, int m, RelocRec *__restrict__ out) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    if (k < st->prefix) return;
    const unsigned int slot = atomicAdd(&st->count_out, 1u);
    if (slot >= (unsigned)m) return;   // cannot happen (exactly min(m, n) keys >= T)
    RelocRec r;
    r.key = k;
    r.label = (int)lab[i];
    r.valid = 1;
    r.xq[0] = r.xq[1] = r.xq[2] = r.xq[3] = 0;
    for (int a = 0; a < D; ++a) r.xq[a] = fixed_i(to_f<T>(xs[xs_index<D>(i, a)]), qe.q[a]);
    out[slot] = r;
}

// Single block: global top-n_empty over all ranks' records, moves applied to
// the (all-reduced, offset-encoded) statistics in cluster order; then resume.
template <int D>
__global__ __launch_bounds__(256) void k_reloc_apply(const RelocRec *__restrict__ recs, int nrec,
                                                     unsigned long long *__restrict__ stats, int K,
                                                     int *__restrict__ rank_buf, int *__restrict__ empty_idx,
                                                     Ctrl *__restrict__ ctrl) {
    const int tid = threadIdx.x;
    // rank of each valid record by (key desc); keys are globally unique
    for (int i = tid; i < nrec; i += 256) {
        int r = 0;
        if (recs[i].valid) {
            for (int j = 0; j < nrec; ++j)
                if (recs[j].valid && recs[j].key > recs[i].key) ++r;
        } else {
            r = 0x7fffffff;
        }
        rank_buf[i] = r;
    }
    __syncthreads();
    if (tid == 0) {
        // max distance == 0 -> nothing to relocate (sklearn _k_means_common.pyx:189-192)
        int top = -1;
        for (int i = 0; i < nrec; ++i)
            if (rank_buf[i] == 0) top = i;
        bool doit = top >= 0 && (recs[top].key >> 32) != 0ull;
        if (doit) {
            // the empty clusters are fixed before any move (sklearn iterates a
            // precomputed list, _k_means_common.pyx:177-178): a donor cluster
            // emptied by a move is not refilled in this pass
            int n_empty = 0;
            for (int j = 0; j < K; ++j)
                if (stats[(size_t)j * (D + 1) + D] == 0ull) empty_idx[n_empty++] = j;
            int done_moves = 0;
            for (int ei = 0; ei < n_empty; ++ei) {
                const int j = empty_idx[ei];
                int pick = -1;
                for (int i = 0; i < nrec; ++i)
                    if (rank_buf[i] == done_moves) { pick = i; break; }
                if (pick < 0) break;
                const RelocRec &r = recs[pick];
                unsigned long long *so = stats + (size_t)r.label * (D + 1);
                unsigned long long *sn = stats + (size_t)j * (D + 1);
                for (int a = 0; a < D; ++a) {
                    unsigned long long u = (unsigned long long)(long long)r.xq[a];
                    so[a] -= u;
                    sn[a] = u;
                }
                so[D] -= 1ull;
                sn[D] = 1ull;
                ++done_moves;
            }
        }
        ctrl->halt = 0u;
        ctrl->resume = 1u;
    }
}

// ------------------------------------------------------------------ misc
template <typename LT>
__global__ __launch_bounds__(256) void k_unpermute(const LT *__restrict__ lab, const uint32_t *__restrict__ perm,
                                                   long long n, int32_t *__restrict__ out) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) out[perm ? perm[i] : (uint32_t)i] = (int32_t)lab[i];
}

// Scatter of the sorted-order labels into row order restricted to the rows
// [r0, r1) (destination windows small enough to stay in the Infinity Cache
// while the random writes land: partial lines merge on-die instead of each
// 2-4 B write costing an HBM burst).
template <typename LT, typename OT>
__global__ __launch_bounds__(256) void k_unpermute_win(const LT *__restrict__ lab, const uint32_t *__restrict__ perm,
                                                       long long n, uint32_t r0, uint32_t r1, OT *__restrict__ out) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = perm[i];
    if (r >= r0 && r < r1) out[r] = (OT)lab[i];
}

// uint16 row-order labels -> int32 (0xffff stays -1 only where K > 65535, which never takes this path)
inline __global__ __launch_bounds__(256) void k_widen_u16(const uint16_t *__restrict__ in, long long n, int32_t *__restrict__ out) {
    long long i = (blockIdx.x * (long long)blockDim.x + threadIdx.x) * 4;
    if (i + 4 <= n) {
        const uint2 w = *reinterpret_cast<const uint2 *>(in + i);
        *reinterpret_cast<int4 *>(out + i) = make_int4((int)(w.x & 0xffffu), (int)(w.x >> 16), (int)(w.y & 0xffffu), (int)(w.y >> 16));
    } else {
        for (; i < n; ++i) out[i] = (int32_t)in[i];
    }
}

template <int D>
__global__ void k_centers_in(const float *__restrict__ Cin, int K, float4 *__restrict__ C) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < D; ++a) v[a] = Cin[(size_t)j * D + a];
    C[j] = make_float4(v[0], v[1], v[2], v[3]);
}

template <int D>
__global__ void k_centers_out(const float4 *__restrict__ C, int K, float *__restrict__ out) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    float4 c = C[j];
    for (int a = 0; a < D; ++a) out[(size_t)j * D + a] = comp(c, a);
}

inline __global__ __launch_bounds__(256) void k_fill_i32(int32_t *__restrict__ p, long long n, int32_t v) {
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__device__ __forceinline__ float synth_value(unsigned long long ctr, unsigned long long seed) {
    unsigned long long z = seed * 0xD1B54A32D192ED03ull + (ctr + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)(uint32_t)(z >> 40) * 5.9604644775390625e-08f;
}

inline __global__ __launch_bounds__(256) void k_synth(float *__restrict__ out, long long n, int d, unsigned long long seed,
                                               long long start) {
    long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n * d) return;
    out[e] = synth_value((unsigned long long)(start * d + e), seed);
}

inline __global__ __launch_bounds__(256) void k_synth_rows(float *__restrict__ out, const long long *__restrict__ rows,
                                                    long long m, int d, unsigned long long seed) {
    long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= m * d) return;
    long long r = rows[e / d];
    out[e] = synth_value((unsigned long long)(r * d + e % d), seed);
}

// Candidate-list statistics for diagnostics.
inline __global__ __launch_bounds__(256) void k_cand_stats(const uint32_t *__restrict__ fc_cnt, long long ncells,
                                                    unsigned long long *__restrict__ out /* sum, max, full */) {
    long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    uint32_t m = fc_cnt[c];
    if (m == FULL) { atomicAdd(out + 2, 1ull); return; }
    atomicAdd(out, (unsigned long long)m);
    atomicMax(out + 1, (unsigned long long)m);
}

// Sole-owner tiles (owner word set) and their points, for diagnostics.
inline __global__ __launch_bounds__(256) void k_sole_stats(const uint4 *__restrict__ tiles, const uint32_t *__restrict__ ntiles,
                                                    unsigned long long *__restrict__ out /* tiles, points */) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const uint4 tr = t < (long long)*ntiles ? tiles[t] : make_uint4(0u, 0u, 0u, 0u);
    const bool sole = tr.w != 0u;
    unsigned long long nt = __popcll(__ballot(sole)), np = sole ? tr.z - tr.y : 0u;
    for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o);
    if ((threadIdx.x & 63) == 0 && nt) {
        atomicAdd(out, nt);
        atomicAdd(out + 1, np);
    }
}

// ------------------------------------------------------------------ brute force
// Stateless brute-force operator: centres staged in LDS (K*4 floats), each
// thread one point; statistics via global atomics (exactness over speed).
template <int D>
__global__ __launch_bounds__(256) void k_bruteforce(const float *__restrict__ X, long long n, const float *__restrict__ Cg,
                                                    int K, QExp qe, int32_t *__restrict__ labels,
                                                    unsigned long long *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float4 sc[];
    for (int j = threadIdx.x; j < K; j += blockDim.x) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < D; ++a) v[a] = Cg[(size_t)j * D + a];
        sc[j] = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float x[D];
        for (int a = 0; a < D; ++a) x[a] = X[i * D + a];
        float bd = dist_canon<D>(x, sc[0]);
        int bj = 0;
        for (int j = 1; j < K; ++j) {
            float dd = dist_canon<D>(x, sc[j]);
            if (dd < bd) { bd = dd; bj = j; }
        }
        labels[i] = bj;
        if (stats) {
            unsigned long long *p = stats + (size_t)bj * (D + 1);
            for (int a = 0; a < D; ++a) atomicAdd(p + a, (unsigned long long)(long long)fixed_i(x[a], qe.q[a]));
            atomicAdd(p + D, 1ull);
        }
    }
}

// ------------------------------------------------------------------ predict
// Centres (K, D) float32 -> the float4 records the list builders and the scans read.
inline __global__ __launch_bounds__(256) void k_predict_pack(const float *__restrict__ Cg, int K, int D,
                                                      float4 *__restrict__ C4) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < D; ++a) v[a] = Cg[(size_t)j * D + a];
    C4[j] = make_float4(v[0], v[1], v[2], v[3]);
}

// Sort-free E-step for given centres (pcm_predict): the cloud is streamed once
// in the caller's row order, one point per lane per round.  A lane bins its
// point with the layout's arithmetic (sort_key_f: fp64 floor, clamped) and scans
// its cell's exact candidate list (k_cand at drift budget 0: ids ascending, so
// strict '<' keeps the lowest index on ties); a cell without a usable list
// (FULL, i.e. more than CAPF candidates) and every point when g.prune == 0 scan
// all K centres through uniform loads.  Nothing is accumulated per centroid, so
// no order of the points is needed; raster-ordered clouds keep the lanes of a
// wave in one or two cells, whose first few records stay cache resident.
// dist (nullable): the canonical squared distance to the winner; inert_rep
// (nullable): exact inertia limbs into the replica lines (k_inert_fold).
template <typename T, int D>
__global__ __launch_bounds__(TPB) void k_predict(const T *__restrict__ X, long long n, Grid g,
                                                 const float4 *__restrict__ C, int K,
                                                 const uint32_t *__restrict__ fc_cnt,
                                                 const float4 *__restrict__ fc_rec,
                                                 const int32_t *__restrict__ fc_lab, int32_t *__restrict__ labels,
                                                 float *__restrict__ dist, unsigned long long *inert_rep, int iscale) {
    unsigned long long ilo = 0ull, ihi = 0ull;
    unsigned iovf = 0u;
    const long long st = (long long)gridDim.x * TPB;
    for (long long i = blockIdx.x * (long long)TPB + threadIdx.x; i < n; i += st) {
        float x[D];
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = to_f<T>(X[i * D + a]);
        uint32_t m = FULL;
        long long cell = 0;
        if (g.prune) {
            int idx[MAXD];
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const int v = (int)floor(((double)x[a] - g.lo[a]) * g.inv[a]);
                idx[a] = v < 0 ? 0 : (v >= g.G[a] ? g.G[a] - 1 : v);
            }
            cell = encode(idx, g.G, D);
            m = fc_cnt[cell];
        }
        float bd;
        int bj = 0;
        if (m - 1u < (uint32_t)CAPF) {   // a list of 1..CAPF candidates
            const float4 *rec = fc_rec + (size_t)cell * CAPF;
            int bp = 0;
            bd = dist_canon<D>(x, rec[0]);
            for (uint32_t p = 1; p < m; ++p) {
                const float dd = dist_canon<D>(x, rec[p]);
                if (dd < bd) { bd = dd; bp = (int)p; }
            }
            bj = fc_lab[(size_t)cell * CAPF + bp];
        } else {
            bd = dist_canon<D>(x, C[0]);
            for (int j = 1; j < K; ++j) {
                const float dd = dist_canon<D>(x, C[j]);
                if (dd < bd) { bd = dd; bj = j; }
            }
        }
        labels[i] = bj;
        if (dist) dist[i] = bd;
        if (inert_rep) inert_add(ilo, ihi, iovf, bd, iscale);
    }
    if (inert_rep) inert_flush(ilo, ihi, iovf, inert_rep);
}

}  // namespace pcm
