// pcm_update.hpp (a part of pcm_kernels.hpp) — M-step kernels: k_upd, k_upd1, k_lists, k_updlists, k_resume
#pragma once
#include "pcm_kcommon.hpp"
#include "pcm_cand.hpp"   // cand_body, refresh_body, SoleW

namespace pcm {

// ------------------------------------------------------------------ centre update + candidate lists
// One Lloyd iteration's M-step (_average_centers, _center_shift, the
// convergence tests; _k_means_common.pyx:274-311, _kmeans.py:717-732) and the
// next iteration's candidate lists, in two launches:
//
//  k_upd   one thread per centroid: its row of `stats` (the summed integer
//          statistics, read and zeroed in place) -> the new centre Cn[j]
//          (computed ONCE per iteration), the statistics-equality test against
//          the previous iteration, the relocation snapshot `held`, its squared
//          shift sh[j] and drift from the lists' reference centre.  Each block
//          leaves a record (UpdPart); the last block
//          to arrive reduces the shift with the fixed 1024-lane tree of
//          oracle/lloyd_ref.py shift_total, halts on an empty cluster (the host
//          relocates, then k_resume + k_cand resume), or publishes the history,
//          flags and the list work: REFRESH the lists' records when every
//          centre is still within the lists' drift budget of the reference
//          position they were built at (the lists stay exact, see prunable),
//          else REBUILD them at the new centres with budget alpha * (largest
//          shift), capped at kappa * the smallest cell width (budget 0 above).
//  k_lists C := Cn (and the new reference buffer when rebuilding), then the
//          refresh or rebuild of this block's cells (cand_body / refresh_body
//          reading the new centres from global memory).
//
// Hand-off inside k_upd (MI355X_MICROARCH.md, hand-off table row 1): sh[] is
// written with sc1 stores, every storing wave drains them (vmcnt(0)) before
// the block barrier, one lane per block adds to the arrival counter, and the
// last arriver reads sh[] and the atomics with sc1 loads.
constexpr int UPD_TPB = 128;
constexpr int SHIFT_LANES = 1024;   // oracle/lloyd_ref.py SHIFT_LANES
constexpr int UPD_LPT = SHIFT_LANES / UPD_TPB;   // tree lanes per thread of the last block
static_assert(UPD_TPB == 128, "k_upd's last tree steps: one LDS step (h = 64), then wave shuffles");
// per-block record of k_upd: changed words, empty clusters, max squared drift, max squared shift
struct UpdPart {
    unsigned long long neq, nempty, dmax_bits, smax_bits;
};
// centroid j's loads: its statistics row, the previous row, the lists'
// reference position and the current centre
template <int D>
__device__ __forceinline__ void upd_load(int j, int K, const unsigned long long *src, const unsigned long long *prev,
                                         const float4 *cref, unsigned sel, const float4 *C,
                                         unsigned long long (&row)[D + 1], unsigned long long (&pv)[D + 1],
                                         float4 &rj, float4 &oj) {
    const size_t o = (size_t)j * (D + 1);
#pragma unroll
    for (int a = 0; a <= D; ++a) { row[a] = src[o + a]; pv[a] = prev[o + a]; }
    rj = cref[(size_t)sel * K + j];
    oj = C[j];
}
// the rows of thread tid, centroid j = tid + S r (k_upd1, k_updlists): statistics,
// previous statistics, BOTH reference buffers (selected once ref_sel is in,
// instead of a second dependent round) and the old centre.  Called before the
// gate test, so every load of the launch shares one memory latency with the
// control words.
template <int D, int R, int S>
__device__ __forceinline__ void upd_load_rows(int tid, int K, const unsigned long long *stats,
                                              const unsigned long long *prev, const float4 *cref, const float4 *C,
                                              unsigned long long (&row)[R][D + 1], unsigned long long (&pv)[R][D + 1],
                                              float4 (&rj)[R], float4 (&rk)[R], float4 (&oj)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        // a thread past K loads centroid 0 (in bounds, unused): without a branch
        // the loads of every row issue back to back (with one, the compiler
        // moved the first use into it and waited between the rows)
        const int j = tid + S * r < K ? tid + S * r : 0;
        const size_t o = (size_t)j * (D + 1);
#pragma unroll
        for (int a = 0; a <= D; ++a) { row[r][a] = stats[o + a]; pv[r][a] = prev[o + a]; }
        rj[r] = cref[j];
        rk[r] = cref[(size_t)K + j];
        oj[r] = C[j];
    }
    // keep the loads above the caller's gate test (the compiler otherwise sinks
    // them below it, behind the control words: a second latency)
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int a = 0; a <= D; ++a) asm volatile("" : "+v"(row[r][a]), "+v"(pv[r][a]));
        asm volatile("" : "+v"(rj[r].x), "+v"(rk[r].x), "+v"(oj[r].x));
    }
}
// the exact mean of a statistics row (_average_centers: the signed fixed-point
// sum, one fp64 division, one rounding to fp32); zero for an empty cluster
template <int D>
__device__ __forceinline__ float4 row_mean(const unsigned long long (&row)[D + 1], const QExp &qe) {
    const unsigned long long c = row[D];
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    if (c > 0) {
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double m = ((double)(long long)row[a] * __builtin_ldexp(1.0, -qe.q[a])) / (double)c;
            out[a] = (float)m;
        }
    }
    return make_float4(out[0], out[1], out[2], out[3]);
}
// its new centre, changed statistic words, emptiness, squared drift and squared shift
template <int D>
__device__ __forceinline__ void upd_row(const unsigned long long (&row)[D + 1], const unsigned long long (&pv)[D + 1],
                                        const float4 &rj, const float4 &oj, const QExp &qe, float4 &cnew,
                                        unsigned long long &neq, unsigned &ne, double &dr, double &ds) {
#pragma unroll
    for (int a = 0; a <= D; ++a) neq += (row[a] != pv[a]) ? 1ull : 0ull;   // raw statistics vs the previous ones
    ne += row[D] == 0ull ? 1u : 0u;
    cnew = row_mean<D>(row, qe);
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const double e1 = (double)comp(cnew, a) - (double)comp(rj, a);
        const double e2 = (double)comp(cnew, a) - (double)comp(oj, a);
        dr += e1 * e1;
        ds += e2 * e2;
    }
}
// block reduction of (changed words, empty clusters, max squared drift, max
// squared shift) over NW waves: upd_wave_sums before a block barrier, upd_block_sums
// after it (every thread gets the same totals; sums and maxima are order-free)
template <int NW>
struct UpdSums {
    unsigned long long neq[NW];
    unsigned ne[NW];
    double dr[NW], ds[NW];
};
template <int NW>
__device__ __forceinline__ void upd_wave_sums(UpdSums<NW> &s, int tid, unsigned long long neq, unsigned ne, double dr,
                                              double ds) {
    for (int o = 32; o > 0; o >>= 1) {
        neq += __shfl_xor(neq, o);
        ne += __shfl_xor(ne, o);
        dr = fmax(dr, __shfl_xor(dr, o));
        ds = fmax(ds, __shfl_xor(ds, o));
    }
    if ((tid & 63) == 0) { s.neq[tid >> 6] = neq; s.ne[tid >> 6] = ne; s.dr[tid >> 6] = dr; s.ds[tid >> 6] = ds; }
}
template <int NW>
__device__ __forceinline__ void upd_block_sums(const UpdSums<NW> &s, unsigned long long &changed,
                                               unsigned long long &n_empty, double &dmax, double &smax) {
    changed = 0ull; n_empty = 0ull; dmax = 0.0; smax = 0.0;
    for (int w = 0; w < NW; ++w) {
        changed += s.neq[w]; n_empty += s.ne[w]; dmax = fmax(dmax, s.dr[w]); smax = fmax(smax, s.ds[w]);
    }
}
// one lane: an empty cluster halts the iteration (the host relocates, then
// k_resume + k_cand resume)
__device__ __forceinline__ void upd_halt(Ctrl *ctrl, unsigned long long n_empty, unsigned long long changed) {
    ctrl->n_empty = (unsigned)n_empty;
    ctrl->neq_saved = changed;
    ctrl->lists = 0u;
    ctrl->halt = 1u;
}
// The tail of oracle/lloyd_ref.py shift_total's halving tree (lane L += lane
// L + h) over the N lanes the block's N threads stored in s[] before a barrier:
// LDS steps down to 128 lanes, the step h = 64 as they are read, then wave
// shuffles.  Block-uniform call; every wave computes the same total (no branch:
// a wave-0-only tail cost the callers a VGPR), valid in its lane 0.
template <int N>
__device__ __forceinline__ double shift_tree_tail(double *s, int tid) {
    for (int h = N / 2; h >= 128; h >>= 1) {
        if (tid < h) s[tid] = s[tid] + s[tid + h];
        __syncthreads();
    }
    double x = s[tid & 63] + s[(tid & 63) + 64];
    for (int st = 32; st > 0; st >>= 1) x = x + __shfl_down(x, st);   // lane t: x_t + x_{t+st}
    return x;
}
// rebuild the lists or refresh their records: REFRESH while every centre is
// within the lists' drift budget of its reference position; a rebuild's new
// budget is alpha * (largest shift), or 0 above the cap
constexpr double DRIFT_SLACK = 1.0 + 9.094947017729282e-13;   // 1 + 2^-40: fp64 rounding of the drift norms
__device__ __forceinline__ void upd_decide(double dmax, double smax, double budget, double alpha, double dl_cap,
                                           bool &rebuild, double &dl_new) {
    rebuild = !(sqrt(dmax) * DRIFT_SLACK <= budget);
    dl_new = alpha * sqrt(smax) * DRIFT_SLACK;
    if (!(dl_new <= dl_cap)) dl_new = 0.0;
}
// one lane: history, convergence flags and the list work of the next launch
// (it, max_iter, budget, tol: the control words as this launch found them)
__device__ __forceinline__ void upd_publish(Ctrl *ctrl, unsigned long long changed, double shift, double dmax,
                                            double smax, unsigned sel, double alpha, double dl_cap,
                                            unsigned long long *hist_changed, double *hist_shift, uint32_t it,
                                            uint32_t max_iter, double budget, double tol) {
    if (it < max_iter) {
        hist_changed[it] = changed;
        hist_shift[it] = shift;
    }
    ctrl->last_changed = changed;
    ctrl->last_shift = shift;
    ctrl->resume = 0u;
    bool rebuild;
    double dl_new;
    upd_decide(dmax, smax, budget, alpha, dl_cap, rebuild, dl_new);
    if (rebuild) {
        ctrl->ref_sel = sel ^ 1u;
        ctrl->budget = dl_new;
        ctrl->rebuilds += 1u;
    }
    ctrl->lists = rebuild ? 2u : 1u;
    ctrl->lists_dl = rebuild ? dl_new : budget;
    uint32_t done = 0;
    if (changed == 0ull) done = 1u;
    else if (shift <= tol) done = 2u;
    if (!done && it + 1 >= max_iter) done = 3u;
    ctrl->done = done;
    ctrl->iter = it + 1;
}

template <int D>
__global__ __launch_bounds__(UPD_TPB) void k_upd(unsigned long long *__restrict__ stats, int K, QExp qe,
                                                 unsigned long long *__restrict__ held,
                                                 unsigned long long *__restrict__ prev, const float4 *__restrict__ C,
                                                 float4 *__restrict__ Cn, const float4 *__restrict__ cref,
                                                 double *__restrict__ sh, UpdPart *__restrict__ upart,
                                                 unsigned long long *__restrict__ hist_changed,
                                                 double *__restrict__ hist_shift, Ctrl *__restrict__ ctrl, double alpha,
                                                 double dl_cap) {
    // the gate flags and the control word this launch reads, in one memory latency
    unsigned gate = ctrl->halt | ctrl->done;
    unsigned sel = ctrl->ref_sel;
    asm volatile("" : "+s"(gate), "+s"(sel));   // keep the loads above the exit
    if (gate != 0u) return;
    const int tid = threadIdx.x;
    const int n = K * (D + 1);
    const int j = blockIdx.x * UPD_TPB + tid;
    unsigned long long neq = 0ull;
    unsigned ne = 0u;
    double dr = 0.0, ds = 0.0;
    unsigned long long row[D + 1], pv[D + 1];
    float4 rj, oj;
    float4 cnew = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < K) {
        upd_load<D>(j, K, stats, prev, cref, sel, C, row, pv, rj, oj);
        upd_row<D>(row, pv, rj, oj, qe, cnew, neq, ne, dr, ds);
        __hip_atomic_store(sh + j, ds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // only sh[] is handed to the last block inside this launch: drain it now;
    // the other stores below are read by later launches (the kernel boundary)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (j < K) {
        const size_t o = (size_t)j * (D + 1);
#pragma unroll
        for (int a = 0; a <= D; ++a) {
            prev[o + a] = row[a];
            held[o + a] = row[a];   // the relocation snapshot, should this iteration halt
            stats[o + a] = 0ull;    // the next accumulation starts from zero
        }
        Cn[j] = cnew;
    }
    if (j == 0) {
        held[n] = 0ull;
        stats[n] = 0ull;
    }
    __shared__ UpdSums<UPD_TPB / 64> sums;
    __shared__ unsigned s_last;
    unsigned long long changed, n_empty;
    double dmax, smax;
    upd_wave_sums(sums, tid, neq, ne, dr, ds);
    __syncthreads();
    if (tid == 0) {
        upd_block_sums(sums, changed, n_empty, dmax, smax);
        // this block's record (sc1 stores, drained before the arrival like sh[])
        UpdPart *pp = upart + blockIdx.x;
        __hip_atomic_store(&pp->neq, changed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&pp->nempty, n_empty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&pp->dmax_bits, (unsigned long long)__double_as_longlong(dmax), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&pp->smax_bits, (unsigned long long)__double_as_longlong(smax), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // release (arrive_last): this block's sh[] and record stores are ordered
        // before its arrival (the sc1 stores above are drained anyway)
        s_last = arrive_last(ctrl) ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every other block's published stores are visible
    // ---- the last block: every other block's sh[] and record have landed
    changed = 0ull; n_empty = 0ull; dmax = 0.0; smax = 0.0;
    for (int b = tid; b < (int)gridDim.x; b += UPD_TPB) {
        const UpdPart *pp = upart + b;
        changed += __hip_atomic_load(&pp->neq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        n_empty += __hip_atomic_load(&pp->nempty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dmax = fmax(dmax, __longlong_as_double(
                              (long long)__hip_atomic_load(&pp->dmax_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
        smax = fmax(smax, __longlong_as_double(
                              (long long)__hip_atomic_load(&pp->smax_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    }
    // (sums of the arrival phase is reused: its readers passed the barrier above)
    upd_wave_sums(sums, tid, changed, (unsigned)n_empty, dmax, smax);
    __syncthreads();
    upd_block_sums(sums, changed, n_empty, dmax, smax);
    if (tid == 0) __hip_atomic_store(&ctrl->u_arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_empty > 0ull) {
        if (tid == 0) upd_halt(ctrl, n_empty, changed);
        return;
    }
    // total shift: lane L sums sh[L + 1024 r] in ascending r, then the halving tree
    double v[UPD_LPT];
#pragma unroll
    for (int u = 0; u < UPD_LPT; ++u) v[u] = 0.0;
    for (int r = 0; r * SHIFT_LANES < K; ++r)
#pragma unroll
        for (int u = 0; u < UPD_LPT; ++u) {
            const int idx = r * SHIFT_LANES + tid + UPD_TPB * u;
            if (idx < K) v[u] = v[u] + __hip_atomic_load(sh + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
    for (int h = UPD_LPT / 2; h >= 1; h >>= 1)   // lanes L and L + UPD_TPB * h live in this thread
#pragma unroll
        for (int u = 0; u < h; ++u) v[u] = v[u] + v[u + h];
    __shared__ double s_tree[UPD_TPB];
    s_tree[tid] = v[0];
    __syncthreads();
    const double shift = shift_tree_tail<UPD_TPB>(s_tree, tid);
    if (tid == 0)
        upd_publish(ctrl, changed, shift, dmax, smax, sel, alpha, dl_cap, hist_changed, hist_shift, ctrl->iter,
                    ctrl->max_iter, ctrl->budget, ctrl->tol);
}


// k_upd in ONE block of SHIFT_LANES threads (K <= UPD1_MAX: configs 1-4): thread L owns centroids L + 1024 r, so its tree lane's
// sum (ascending r) stays in registers and the halving tree runs in LDS -- no
// per-block records, no arrival counter, no second pass over sh[] (the
// multi-block k_upd's hand-off cost ~4 memory latencies: 9.5 us at K = 1024).
// Same arithmetic, stores and published words as k_upd.
// R = rows per thread = ceil(K / 1024).  K = 4096 (config 5) keeps the
// multi-block k_upd: one block doing 4 rows per thread (in batches, to stay
// within 128 VGPRs) measured 28 us against k_upd's 15 at an 8-way config-5 slab.
constexpr int UPD1_MAX = 2 * SHIFT_LANES;
template <int D, int R>
__global__ __launch_bounds__(SHIFT_LANES) void k_upd1(unsigned long long *__restrict__ stats, int K, QExp qe,
                                                      unsigned long long *__restrict__ held,
                                                      unsigned long long *__restrict__ prev,
                                                      const float4 *__restrict__ C, float4 *__restrict__ Cn,
                                                      const float4 *__restrict__ cref,
                                                      unsigned long long *__restrict__ hist_changed,
                                                      double *__restrict__ hist_shift, Ctrl *__restrict__ ctrl,
                                                      double alpha, double dl_cap) {
    // every load of the launch in ONE memory latency: the control words and the rows
    unsigned gate = ctrl->halt | ctrl->done;
    uint32_t it = ctrl->iter, max_iter = ctrl->max_iter;
    unsigned sel = ctrl->ref_sel;
    double budget = ctrl->budget, tol = ctrl->tol;
    const int tid = threadIdx.x;
    const int n = K * (D + 1);
    static_assert(R >= 1 && R <= 2, "K <= UPD1_MAX");
    unsigned long long row[R][D + 1], pv[R][D + 1];
    float4 rj[R], rk[R], oj[R];
    upd_load_rows<D, R, SHIFT_LANES>(tid, K, stats, prev, cref, C, row, pv, rj, rk, oj);
    // keep the control-word loads above the exit, in flight with the rows
    asm volatile("" : "+s"(gate), "+s"(it), "+s"(max_iter), "+s"(sel), "+s"(budget), "+s"(tol));
    if (gate != 0u) return;
    unsigned long long neq = 0ull;
    unsigned ne = 0u;
    double dr = 0.0, ds = 0.0, v = 0.0;
    float4 cnew[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = tid + SHIFT_LANES * r;
        if (j < K) {
            double drj = 0.0, dsj = 0.0;
            upd_row<D>(row[r], pv[r], sel ? rk[r] : rj[r], oj[r], qe, cnew[r], neq, ne, drj, dsj);
            dr = fmax(dr, drj);
            ds = fmax(ds, dsj);
            v = v + dsj;   // tree lane tid: sh[tid + 1024 r] in ascending r
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = tid + SHIFT_LANES * r;
        if (j < K) {
            const size_t o = (size_t)j * (D + 1);
#pragma unroll
            for (int a = 0; a <= D; ++a) {
                prev[o + a] = row[r][a];
                held[o + a] = row[r][a];   // the relocation snapshot, should this iteration halt
                stats[o + a] = 0ull;       // the next accumulation starts from zero
            }
            Cn[j] = cnew[r];
        }
    }
    if (tid == 0) {
        held[n] = 0ull;
        stats[n] = 0ull;
    }
    __shared__ UpdSums<SHIFT_LANES / 64> sums;
    __shared__ double s_tree[SHIFT_LANES];
    upd_wave_sums(sums, tid, neq, ne, dr, ds);
    s_tree[tid] = v;
    __syncthreads();
    unsigned long long changed, n_empty;
    double dmax, smax;
    upd_block_sums(sums, changed, n_empty, dmax, smax);
    if (n_empty > 0ull) {
        if (tid == 0) upd_halt(ctrl, n_empty, changed);
        return;
    }
    const double shift = shift_tree_tail<SHIFT_LANES>(s_tree, tid);
    if (tid == 0)
        upd_publish(ctrl, changed, shift, dmax, smax, sel, alpha, dl_cap, hist_changed, hist_shift, it, max_iter,
                    budget, tol);
}


// C := Cn (the centres k_upd published) and the next iteration's candidate
// lists: a rebuild at Cn with the published budget (the new reference buffer
// cref[ref_sel] := Cn) or a refresh of the records.  Runs after a completed
// k_upd: halted iterations leave C untouched (the relocation needs the old
// centres); queued no-op launches after convergence repeat the same copy and
// lists (idempotent).
constexpr int LISTS_STAGE_MAX = 2048;   // k_lists stages the centres in LDS up to this K (32 KB)
template <int D, int FC = 4, bool STAGE = false, int TPB = CAND_TPB>
__global__ __launch_bounds__(TPB) void k_lists(Grid g, const float4 *__restrict__ Cn, float4 *__restrict__ C,
                                                    float4 *__restrict__ cref, int K, const Ctrl *__restrict__ ctrl,
                                                    uint32_t *__restrict__ fc_cnt, float4 *__restrict__ fc_rec,
                                                    int32_t *__restrict__ fc_lab, int bpc, CoarseL cl, SoleW sw) {
    unsigned halt = ctrl->halt;
    unsigned mode = ctrl->lists;
    unsigned sel = ctrl->ref_sel;
    double dl = ctrl->lists_dl;
    // STAGE: all K new centres staged in LDS by one coalesced pass, issued with
    // the control-word loads (one memory latency for both; a gated launch
    // leaves the LDS copy unused): the list phases' reads of them (references,
    // tests, compaction) become LDS reads instead of dependent global round trips
    extern __shared__ __attribute__((aligned(16))) float4 cstage[];
    if constexpr (STAGE)
        for (int j = threadIdx.x; j < K; j += TPB) cstage[j] = Cn[j];
    asm volatile("" : "+s"(halt), "+s"(mode), "+s"(sel), "+s"(dl));
    if (halt != 0u || mode == 0u) return;
    DBG_T(0);
    if constexpr (STAGE) __syncthreads();
    for (int j = blockIdx.x * TPB + threadIdx.x; j < K; j += gridDim.x * TPB) {
        const float4 c = STAGE ? cstage[j] : Cn[j];
        C[j] = c;
        if (mode == 2u) cref[(size_t)sel * K + j] = c;
    }
    if (mode != 2u) {
        refresh_body<D, TPB>(g, Cn, fc_cnt, fc_rec, fc_lab);
        return;
    }
    if constexpr (STAGE) cand_body<D, FC, TPB>(g, cstage, K, fc_cnt, fc_rec, fc_lab, bpc, dl, cl, sw);
    else cand_body<D, FC, TPB>(g, Cn, K, fc_cnt, fc_rec, fc_lab, bpc, dl, cl, sw);
}

// Centre update and candidate lists in ONE launch (D <= 3, K <= CAND_TPB * 2 =
// 1024: configs 1-4).  Every block loads all K statistics rows, the previous
// rows, the old centres and both reference buffers together with the control
// words -- one memory latency -- and computes all K new centres into LDS plus the
// order-independent decisions every block needs identically (an empty cluster
// halts; the largest drift and shift give rebuild-or-refresh and the new
// budget).  Then one agent-scope arrival per block; the LAST block to arrive
// (every other block's loads have returned by then) publishes what k_upd does
// -- prev, held, the zeroed statistics, C and the new reference
// buffer, the shift tree of oracle/lloyd_ref.py shift_total, history and flags
// -- and every block rebuilds or refreshes its own cells' lists from the LDS
// centres.  Replaces k_upd1 + k_lists (two launches, ~16 us at an 8-way slab).
// PUB (the host takes it when one more block fits the residency, e.g.
// the 8-way slab's 256 list blocks): the LAST block of the grid builds no lists
// and is the publisher -- it waits (bounded, s_sleep) until the list blocks have
// arrived, right after their centres, and publishes while they still build
// their lists, instead of after its own lists; a wait past 2 s sets done = 5.
template <int D, int R, bool PUB = false>
__global__ __launch_bounds__(CAND_TPB) void k_updlists(
    unsigned long long *__restrict__ stats, int K, QExp qe,
    unsigned long long *__restrict__ held, unsigned long long *__restrict__ prev, float4 *__restrict__ C,
    float4 *__restrict__ cref, unsigned long long *__restrict__ hist_changed, double *__restrict__ hist_shift,
    Ctrl *__restrict__ ctrl, double alpha, double dl_cap, Grid g, uint32_t *__restrict__ fc_cnt,
    float4 *__restrict__ fc_rec, int32_t *__restrict__ fc_lab, int bpc, SoleW sw) {
    static_assert(R * CAND_TPB <= SHIFT_LANES && SHIFT_LANES % CAND_TPB == 0, "one tree lane per row");
    extern __shared__ __attribute__((aligned(16))) float4 cstage[];   // the K new centres
    DBG_CLOCK(t_start, K);   // stamp 13, stored below: a DBG_T here would turn the pinned loads into vector loads
    unsigned gate = ctrl->halt | ctrl->done;
    uint32_t it = ctrl->iter, max_iter = ctrl->max_iter;
    unsigned sel = ctrl->ref_sel;
    double budget = ctrl->budget, tol = ctrl->tol;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = K * (D + 1);
    // row r of this thread: centroid j = tid + CAND_TPB * r (tree lane j).  (The
    // publisher alone loading the previous rows, for the changed-word count,
    // measured slower: its extra latency sits on the launch's tail.)
    unsigned long long row[R][D + 1], pv[R][D + 1];
    float4 rj[R], rk[R], oj[R];
    upd_load_rows<D, R, CAND_TPB>(tid, K, stats, prev, cref, C, row, pv, rj, rk, oj);
    // keep the control-word loads above the exit, in flight with the rows
    asm volatile("" : "+s"(gate), "+s"(it), "+s"(max_iter), "+s"(sel), "+s"(budget), "+s"(tol));
    if (gate != 0u) return;
    DBG_V(13, t_start);
    DBG_T(0);
    unsigned long long neq = 0ull;
    unsigned ne = 0u;
    double dr = 0.0, ds = 0.0, sh[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = tid + CAND_TPB * r;
        sh[r] = 0.0;
        if (j < K) {
            double drj = 0.0, dsj = 0.0;
            float4 cnew;
            upd_row<D>(row[r], pv[r], sel ? rk[r] : rj[r], oj[r], qe, cnew, neq, ne, drj, dsj);
            dr = fmax(dr, drj);
            ds = fmax(ds, dsj);
            sh[r] = dsj;
            cstage[j] = cnew;
        }
    }
    __shared__ UpdSums<CAND_TPB / 64> sums;
    __shared__ unsigned s_last;
    // the shift tree's lanes: L < 1024 holds sh[L] (K <= 1024); the first halving
    // step (lane t += lane t + 512) runs in this thread's registers.  Kept in LDS
    // for the publisher, so that nothing of the centre phase stays live in
    // registers through the lists (a 2-blocks-per-CU residency at 512 blocks)
    static_assert(CAND_TPB == SHIFT_LANES / 2, "thread t holds tree lanes t and t + 512");
    __shared__ double s_tree[CAND_TPB];
    s_tree[tid] = sh[0] + (R > 1 ? sh[R > 1 ? 1 : 0] : 0.0);
    upd_wave_sums(sums, tid, neq, ne, dr, ds);
    __syncthreads();   // every load of this block has returned (its values are used above)
    // The arrival: issued now, its returned place read after this block's lists.
    // One same-address atomic per block (512 of them serialise at the memory
    // side, ~12 ns each): waiting for it here held every block's lists for its
    // place in that queue ("centres + arrival" 6.2 us of a ~17 us block at
    // config 3, rd5_updlists_phases_c3.txt).  No release fence: the rows, prev,
    // C and control words the publisher overwrites were consumed above, and the
    // lists read only the LDS centres.  The publisher is the last block to
    // ARRIVE (here), not the last to finish its lists, so its extra work lands
    // on a block of ordinary length.
    const bool pub_blk = PUB && blockIdx.x == gridDim.x - 1u;   // the dedicated publisher (PUB)
    const unsigned nlist = PUB ? gridDim.x - 1u : gridDim.x;
    unsigned tk = 0u;
    if constexpr (PUB) {
        if (!pub_blk && tid == 0) __hip_atomic_fetch_add(&ctrl->u_arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        tk = arrive_issue(&ctrl->u_arrive, (unsigned long long)__builtin_amdgcn_readfirstlane(wv == 0 ? 1 : 0));
    }
    {
        // the decisions of upd_publish, identical in every block (same data, order-free maxima)
        unsigned long long changed, n_empty;
        double dmax, smax, dl_new;
        bool rebuild;
        upd_block_sums(sums, changed, n_empty, dmax, smax);
        upd_decide(dmax, smax, budget, alpha, dl_cap, rebuild, dl_new);
        // this block's share of the writes nobody reads in this launch: the
        // relocation snapshot `held` and, on a rebuild, the new reference buffer
        // (the blocks read cref[sel ^ 1] only speculatively, and use cref[sel])
        const int share = (K + (int)gridDim.x - 1) / (int)gridDim.x;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = tid + CAND_TPB * r;
            if (j < K && j / share == (int)blockIdx.x) {
                const size_t o = (size_t)j * (D + 1);
#pragma unroll
                for (int a = 0; a <= D; ++a) held[o + a] = row[r][a];
                if (n_empty == 0ull && rebuild) cref[(size_t)(sel ^ 1u) * K + j] = cstage[j];
            }
        }
        DBG_T(15);
        // a halted iteration (identical decision in every block) builds no lists
        if (n_empty == 0ull && !pub_blk) {
            DBG_T(14);
            // this block's cells: rebuilt at the new centres with the new budget, or refreshed
            if (rebuild) cand_body<D, 4>(g, cstage, K, fc_cnt, fc_rec, fc_lab, bpc, dl_new, CoarseL{}, sw);
            else refresh_body<D>(g, cstage, fc_cnt, fc_rec, fc_lab, nlist);
        }
    }
    if constexpr (PUB) {
        if (!pub_blk) return;
        if (wv == 0) {   // every list block arrives right after its centres: a bounded wait
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
            unsigned ok = 1u;
            while (__hip_atomic_load(&ctrl->u_arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nlist) {
                __builtin_amdgcn_s_sleep(2);
                if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) { ok = 0u; break; }
            }
            if (lane == 0) s_last = ok;
        }
        __syncthreads();   // s_last
        if (!s_last) {
            if (tid == 0) ctrl->done = 5u;   // the fit is void (lloyd.run raises)
            return;
        }
    } else {
        if (wv == 0) {
            const unsigned place = arrive_read(tk);
            if (lane == 0) s_last = place == gridDim.x - 1u;
        }
        __syncthreads();   // s_last
        if (!s_last) return;
    }
    DBG_T(3);
    // ---- the publisher: every other block's loads have returned.  It reads the
    // rows again (L2; nobody has written them): prev := rows, the statistics := 0
    // for the next accumulation and (unless halted: the relocation needs the old
    // C) C := the new centres.  Invariant the zeroing relies on: every block
    // consumed its loads of prev, C and the statistics rows (their values feed
    // the centres above) before it arrived.
    unsigned long long changed, n_empty;
    double dmax, smax;
    upd_block_sums(sums, changed, n_empty, dmax, smax);
    unsigned long long v[R][D + 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = tid + CAND_TPB * r;
        const size_t o = (size_t)(j < K ? j : 0) * (D + 1);
#pragma unroll
        for (int a = 0; a <= D; ++a) v[r][a] = stats[o + a];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = tid + CAND_TPB * r;
        if (j < K) {
            const size_t o = (size_t)j * (D + 1);
#pragma unroll
            for (int a = 0; a <= D; ++a) prev[o + a] = v[r][a];
#pragma unroll
            for (int a = 0; a <= D; ++a) stats[o + a] = 0ull;   // the next accumulation starts from zero
            if (n_empty == 0ull) C[j] = cstage[j];
        }
    }
    // (read again after the stores: the totals stay out of registers through them)
    upd_block_sums(sums, changed, n_empty, dmax, smax);
    if (tid == 0) {
        held[n] = 0ull;
        stats[n] = 0ull;
        __hip_atomic_store(&ctrl->u_arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (n_empty > 0ull) {
        if (tid == 0) upd_halt(ctrl, n_empty, changed);
    } else {
        const double shift = shift_tree_tail<CAND_TPB>(s_tree, tid);
        if (tid == 0)
            upd_publish(ctrl, changed, shift, dmax, smax, sel, alpha, dl_cap, hist_changed, hist_shift, it, max_iter,
                        budget, tol);
    }
    DBG_T(6);
}

// The update of an iteration that halted on an empty cluster, after the host's
// relocation (k_reloc_apply gave the empty clusters their points in `held`,
// which the host copied to `stats`, and set ctrl->resume).  One block of
// SHIFT_LANES threads: averages (a cluster still empty takes the largest
// cluster's new centre, lowest index on ties), the shift with the tree of
// oracle/lloyd_ref.py shift_total (thread L sums j = L + 1024 r in ascending
// r), zeroes `stats` and publishes history and flags with the changed-word
// count the halted update saved.  It leaves ctrl->lists and the drift budget
// alone: the k_cand that follows rebuilds the lists at the new C.
template <int D>
__global__ __launch_bounds__(SHIFT_LANES) void k_resume(unsigned long long *__restrict__ stats, int K, QExp qe,
                                                        float4 *__restrict__ C, float4 *__restrict__ Cn,
                                                        unsigned long long *__restrict__ hist_changed,
                                                        double *__restrict__ hist_shift, Ctrl *__restrict__ ctrl) {
    if (gated(ctrl)) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = K * (D + 1);
    constexpr int NW = SHIFT_LANES / 64;
    __shared__ unsigned cnt_empty;
    __shared__ unsigned long long wmax[NW];
    __shared__ int warg[NW];
    __shared__ double ssum[SHIFT_LANES];
    if (tid == 0) cnt_empty = 0;
    __syncthreads();
    unsigned long long bmax = 0;
    int barg = 0x7fffffff;
    unsigned ne = 0;
    for (int j = tid; j < K; j += SHIFT_LANES) {
        const unsigned long long c = stats[(size_t)j * (D + 1) + D];
        if (c == 0) ne++;
        if (c > bmax) { bmax = c; barg = j; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ob = __shfl_xor(bmax, o);
        const int oa = __shfl_xor(barg, o);
        if (ob > bmax || (ob == bmax && oa < barg)) { bmax = ob; barg = oa; }
    }
    if (lane == 0) { wmax[wv] = bmax; warg[wv] = barg; }
    if (ne) atomicAdd(&cnt_empty, ne);
    __syncthreads();
    unsigned long long gmax = wmax[0];
    int argmax = warg[0];
    for (int w = 1; w < NW; ++w)
        if (wmax[w] > gmax || (wmax[w] == gmax && warg[w] < argmax)) { gmax = wmax[w]; argmax = warg[w]; }
    auto mean_of = [&](int j, float4 &cn) -> bool {
        unsigned long long row[D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a) row[a] = stats[(size_t)j * (D + 1) + a];
        cn = row_mean<D>(row, qe);
        return row[D] > 0;
    };
    auto shift_of = [&](const float4 &a4, const float4 &b4) -> double {
        double sh = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double dd = (double)comp(a4, a) - (double)comp(b4, a);
            const double sq = dd * dd;
            sh = (a == 0) ? sq : sh + sq;
        }
        return sh;
    };
    double acc = 0.0;   // tree lane tid: the shifts of j = tid + 1024 r in ascending r
    if (cnt_empty == 0) {   // the common case: no empty cluster, one pass
        for (int j = tid; j < K; j += SHIFT_LANES) {
            const float4 b4 = C[j];
            float4 cn;
            mean_of(j, cn);
            acc = acc + shift_of(cn, b4);
            C[j] = cn;
        }
    } else {   // an empty cluster copies the largest one's centre
        for (int j = tid; j < K; j += SHIFT_LANES) {
            float4 cn;
            if (mean_of(j, cn)) Cn[j] = cn;
        }
        __syncthreads();   // Cn[argmax] is read by other threads
        for (int j = tid; j < K; j += SHIFT_LANES) {
            const unsigned long long c = stats[(size_t)j * (D + 1) + D];
            if (c == 0) Cn[j] = (gmax > 0) ? Cn[argmax] : C[j];
            const float4 a4 = Cn[j], b4 = C[j];
            acc = acc + shift_of(a4, b4);
            C[j] = Cn[j];
        }
    }
    ssum[tid] = acc;
    __syncthreads();
    // zero the statistics for the next iteration's accumulation (every read above precedes the barrier)
    for (int i = tid; i < n + 1; i += SHIFT_LANES) stats[i] = 0ull;
    const double shift = shift_tree_tail<SHIFT_LANES>(ssum, tid);
    if (tid == 0) {
        const unsigned long long changed = ctrl->neq_saved;
        const uint32_t it = ctrl->iter;
        if (it < ctrl->max_iter) {
            hist_changed[it] = changed;
            hist_shift[it] = shift;
        }
        ctrl->last_changed = changed;
        ctrl->last_shift = shift;
        ctrl->resume = 0u;
        uint32_t done = 0;
        if (changed == 0ull) done = 1u;
        else if (shift <= ctrl->tol) done = 2u;
        ctrl->iter = it + 1;
        if (!done && it + 1 >= ctrl->max_iter) done = 3u;
        ctrl->done = done;
    }
}

}  // namespace pcm
