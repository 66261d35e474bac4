// pcm_kcommon.hpp (a part of pcm_kernels.hpp) — shared types, control block, arrival helpers and box geometry of the engine kernels
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcm_debug.hpp"   // DBG_* phase stamps (debug builds only)

namespace pcm {

constexpr int MAXD = 4;
constexpr int CAPC = 512;          // coarse candidate capacity (12.5M shard: coarse lists p90 243, max > 256)
constexpr int CAPF = 64;           // fine candidate capacity
constexpr int MSLOT = 4;           // LDS-privatised slots per lane (nearest-to-centre ranks)
#ifndef PCM_TPB
#define PCM_TPB 128   // 128 measured 9% faster than 256 at 100M (two-wave barriers), 10% at 12.5M
#endif
constexpr int TPB = PCM_TPB;       // assign block size
#ifndef PCM_TILE_PTS
#define PCM_TILE_PTS (32 * PCM_TPB)
#endif
constexpr int TILE = PCM_TILE_PTS;  // max points per tile: <= 32 per lane, 64 per shared LDS word (see AccL)
static_assert(TILE <= 64 * (TPB >= 128 ? TPB / 2 : TPB), "an LDS word sums <= 64 points (int32-exact)");
constexpr uint32_t FULL = 0xFFFFFFFFu;
constexpr int TLCAP = 256;        // tile lists staged whole in k_lloyd1's LDS (slot-map path)
constexpr int TLMAX = 1024;       // tile-list capacity (longer lists: FULL); lists past TLCAP scan in LDS chunks
constexpr uint32_t TL_MIN = 16;   // crowded layouts: tiles of cells with longer lists (or FULL) get tile lists
constexpr int QBITS = 25;
// Pruning margins (see DESIGN.md "Exactness of pruning").
constexpr double PEPS = 7.62939453125e-06;   // 2^-17  >> 6 * 2^-24 (fp32 distance error)
constexpr double PTAU = 1e-36;               // >> fp32 underflow error of a distance
constexpr double DRIFT_SAFE = 1.0 + 6.103515625e-05;   // 1 + 2^-14 >= (1 + PEPS) * fp64 rounding slack

struct Grid {
    int d;
    int prune;
    int F;
    int pad_;
    int G[MAXD];
    int GC[MAXD];
    double lo[MAXD], w[MAXD], inv[MAXD], mg[MAXD], ext[MAXD];
    long long ncells, ncoarse;
};

// Device control block (one per engine).
constexpr int INERT_REP = 32;
struct Ctrl {
    uint32_t halt, done, iter, max_iter;
    uint32_t n_empty, resume, status, pad0;
    double tol;
    unsigned long long inert[4];    // exact inertia: 32-bit limbs of sum trunc(d * 2^s), [3] = overflow count
    unsigned long long neq_saved;   // stat words changed at a halted iteration (used on resume)
    unsigned long long last_changed;
    double last_shift;
    unsigned int ref_sel;           // candidate lists: which reference-centre buffer (cref[ref_sel]) they were built at
    double budget;                  // ... and the centre drift they tolerate (0: exact for the reference only)
    unsigned int rebuilds;          // candidate-list rebuilds of this fit (diagnostics)
    unsigned int pad1;
    // k_upd: arrival counter of its blocks (the last one reduces their records and
    // resets it) and the list work it hands to k_lists
    unsigned int u_arrive, pad3;
    unsigned int lists, pad2;       // k_lists: 0 nothing, 1 refresh the records, 2 rebuild the lists
    double lists_dl;                // the rebuilt lists' drift budget
    // Same-address device atomics serialise at the memory side (~12 ns each, MI355X_MICROARCH.md
    // "fanin") and hold back loads queued behind them, so bulk per-wave adds are spread instead:
    // k_label: exact-inertia limbs added per block into replica lines (folded by k_inert_fold)
    alignas(128) unsigned long long inert_rep[INERT_REP][16];
};

// Arrival of block blockIdx.x among gridDim.x on one counter: true for the last
// one.  Release: the block's prior loads and stores precede its arrival (the
// last block then takes an acquire fence).  Round 5 measured a two-level
// arrival (8 group counters, then one) at config 3: "centres + arrival" 6.2 ->
// 7.3 us per block, so the single counter stays (profiles/rd5_updlists_phases_c3.txt).
// k_updlists' arrival, issued early and read late: a relaxed agent-scope
// fetch-add by lane 0 of the calling wave (EXEC = lane 0, or no lane when `on`
// is 0) whose returned value stays in flight -- hipcc's waitcnt pass does not
// see the asm, and __syncthreads waits only on LDS -- until arrive_read's
// explicit vmcnt(0).  (The compiler's own atomic would be rewritten into a
// wave-aggregated form whose broadcast waits for the return on the spot.)
__device__ __forceinline__ unsigned arrive_issue(unsigned *p, unsigned long long on) {
    unsigned old = 0u;
    unsigned long long save;
    asm volatile(
        "s_mov_b64 %1, exec\n\t"
        "s_mov_b64 exec, %4\n\t"
        "global_atomic_add %0, %2, %3, off sc0\n\t"
        "s_mov_b64 exec, %1"
        : "+v"(old), "=&s"(save)
        : "v"(p), "v"(1u), "s"(on)
        : "memory");
    return old;
}
__device__ __forceinline__ unsigned arrive_read(unsigned v) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v) : : "memory");
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ bool arrive_last(Ctrl *ctrl) {
    const unsigned p = __hip_atomic_fetch_add(&ctrl->u_arrive, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    return p == gridDim.x - 1u;
}

// Fixed-point exponents q_a (identical on every rank).
struct QExp {
    int q[MAXD];
};

// Control words are written by earlier kernels on the same stream; the kernel
// boundary orders them, so plain loads suffice.
__device__ __forceinline__ bool gated(const Ctrl *c) { return (c->halt | c->done) != 0u; }

// ------------------------------------------------------------------ helpers
template <int D>
__device__ __forceinline__ float dist_canon(const float (&x)[D], const float4 &c) {
    float a = x[0] - c.x;
    float acc = a * a;
    if (D > 1) { float b = x[1] - c.y; float s = b * b; acc = acc + s; }
    if (D > 2) { float b = x[2] - c.z; float s = b * b; acc = acc + s; }
    if (D > 3) { float b = x[3] - c.w; float s = b * b; acc = acc + s; }
    return acc;
}

__device__ __forceinline__ float comp(const float4 &c, int a) {
    return a == 0 ? c.x : a == 1 ? c.y : a == 2 ? c.z : c.w;
}

// Fixed-point coordinate: trunc(x * 2^q) (exact scaling, truncation toward 0).
__device__ __forceinline__ int fixed_i(float x, int q) { return (int)__builtin_ldexpf(x, q); }

__device__ __forceinline__ void decode(long long c, const int *G, int d, int *idx) {
    for (int a = d - 1; a >= 0; --a) {
        idx[a] = (int)(c % G[a]);
        c /= G[a];
    }
}

__device__ __forceinline__ long long encode(const int *idx, const int *G, int d) {
    long long c = 0;
    for (int a = 0; a < d; ++a) c = c * G[a] + idx[a];
    return c;
}

// fine-cell range [f0, f1] on every axis -> fp64 box containing every point binned there
template <int D>
__device__ __forceinline__ void cell_box(const Grid &g, const int *f0, const int *f1, double *blo, double *bhi) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        blo[a] = g.lo[a] + (double)f0[a] * g.w[a] - g.mg[a];
        bhi[a] = (f1[a] == g.G[a] - 1) ? g.lo[a] + g.ext[a] + g.mg[a]
                                       : g.lo[a] + (double)(f1[a] + 1) * g.w[a] + g.mg[a];
    }
}

template <int D>
__device__ __forceinline__ double maxdist(const double *blo, const double *bhi, const float4 &c) {
    double s = 0.0;
    for (int a = 0; a < D; ++a) {
        double ca = (double)comp(c, a);
        double l = blo[a] - ca, h = bhi[a] - ca;
        s += fmax(l * l, h * h);
    }
    return s;
}

// True iff every point of the box is provably (with margin PEPS/PTAU) strictly
// closer, in the canonical fp32 distance, to r than to c.  The objective
// (1-e)|x-c|^2 - (1+e)|x-r|^2 is separable and concave per axis, so its box
// minimum is the sum of per-axis endpoint minima.
//
// Drift budget dl > 0 (lists reused while every centre stays within dl of the
// reference position the list was built at): with |x-c| <= Mc and |x-r| <= Mr
// over the box, (1-e)(|x-c|-dl)^2 - (1+e)(|x-r|+dl)^2 >= S - 2 dl (1+e)(Mc+Mr)
// - 2 e dl^2, so S > tau + 2 dl (Mc+Mr) (1+e) + 2 dl^2 keeps c dominated by r
// for any moved centres c', r' (and forces |x-c| > 2 dl).  mr = Mr.
template <int D>
__device__ __forceinline__ bool prunable(const double *blo, const double *bhi, const float4 &c, const float4 &r,
                                         double dl = 0.0, double mr = 0.0) {
    const double em = 1.0 - PEPS, ep = 1.0 + PEPS;
    double s = 0.0;
    for (int a = 0; a < D; ++a) {
        double ca = (double)comp(c, a), ra = (double)comp(r, a);
        double cl = blo[a] - ca, ch = bhi[a] - ca, rl = blo[a] - ra, rh = bhi[a] - ra;
        double gl = em * (cl * cl) - ep * (rl * rl);
        double gh = em * (ch * ch) - ep * (rh * rh);
        s += fmin(gl, gh);
    }
    if (!(dl > 0.0)) return s > PTAU;
    const double mc = sqrt(maxdist<D>(blo, bhi, c));
    return s > PTAU + (2.0 * dl * (mc + mr) + 2.0 * dl * dl) * DRIFT_SAFE;
}

template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<__half>(__half v) { return __half2float(v); }

}  // namespace pcm
