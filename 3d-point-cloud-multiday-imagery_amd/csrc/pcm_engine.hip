// pcm_engine.hip — the Lloyd engine's C ABI (include/pcm_kmeans.h) on the MI355X: errors,
// create / destroy, fit start, the iteration entry points, timing, relocation and the read-outs.
// The layout is pcm_layout.hip's.  All device work is stream-ordered; the per-iteration entry
// points allocate nothing and never synchronise, so a caller may capture them into a HIP graph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "pcm_kernels.hpp"
#include "pcm_sort.hpp"   // k_lab_gather4
#include "pcm_host.hpp"
#include "pcm_xchg.hpp"

using namespace pcm;

namespace {
thread_local std::string g_err;
}  // namespace

int pcm_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int pcm::check_device(pcm_engine *e) {
    int cur = -1;
    HIPCHK(hipGetDevice(&cur));
    if (cur != e->device)
        return fail(PCM_E_STATE, "current HIP device " + std::to_string(cur) + " != engine device " +
                                     std::to_string(e->device));
    return 0;
}

int pcm::lloyd_slots(const pcm_engine *e) {
    if (const char *ov = std::getenv("PCM_LSLOT_RT")) return std::atoi(ov) == 8 ? 8 : LSLOT;   // tuning sweeps only
    // cells per centre of the whole cloud (a spatial shard's cells cover ~n / n_global of the centres)
    const double share = e->n_global > 0 ? std::min(1.0, (double)e->n / (double)e->n_global) : 1.0;
    return (e->g.prune && (double)e->g.ncells >= 8.0 * e->k * share) ? 8 : LSLOT;
}

int pcm::host_candidates(int d, const Grid &g, const float4 *C, int k, Ctrl *ctrl, int gate, bool split, int bpc,
                         uint32_t *fc_cnt, float4 *fc_rec, int32_t *fc_lab, float4 *cref, uint32_t *cl_cnt,
                         int32_t *cl_idx, const SoleW &sw, hipStream_t s) {
    return dispatch_d(d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        if (split) {
            long long nmid = 1;
            for (int a = 0; a < D; ++a) nmid *= (g.G[a] + 1) / 2;
            k_coarse<D><<<(int)g.ncoarse, CAND_TPB, 0, s>>>(g, C, k, ctrl, 0, cl_cnt, cl_idx);
            LAUNCHCHK();
            CoarseL cl;
            cl.in_cnt = cl_cnt;
            cl.in_idx = cl_idx;
            k_cand<D, 2><<<(int)nmid, CAND_TPB, 0, s>>>(g, C, k, fc_cnt, fc_rec, fc_lab, ctrl, gate, 1, cref, cl, sw);
            LAUNCHCHK();
            return 0;
        }
        k_cand<D><<<(int)(g.ncoarse * bpc), CAND_TPB, 0, s>>>(g, C, k, fc_cnt, fc_rec, fc_lab, ctrl, gate, bpc, cref,
                                                              CoarseL{}, sw);
        LAUNCHCHK();
        return 0;
    });
}

extern "C" {

int pcm_abi_version(void) { return PCM_ABI_VERSION; }

double pcm_inertia_value(const uint64_t *limbs, int scale, uint32_t overflow) {
    if (!limbs) return 0.0;
    if (overflow) return HUGE_VAL;
    const unsigned __int128 v = (unsigned __int128)limbs[0] + ((unsigned __int128)limbs[1] << 32) +
                                ((unsigned __int128)limbs[2] << 64);
    return std::ldexp((double)v, -scale);   // one correctly rounded conversion, exact scaling
}

int pcm_last_error(char *buf, size_t n) {
    if (!buf || n == 0) return PCM_E_ARG;
    std::snprintf(buf, n, "%s", g_err.c_str());
    return 0;
}

int pcm_engine_create(int device, int d, int k, int dtype, int max_iter, pcm_engine **out) {
    if (!out) return fail(PCM_E_ARG, "out is null");
    *out = nullptr;
    if (d < 1 || d > MAXD) return fail(PCM_E_ARG, "d must be 1..4");
    if (k < 1 || k > (1 << 20)) return fail(PCM_E_ARG, "k out of range");
    if (dtype != PCM_F32 && dtype != PCM_F16) return fail(PCM_E_ARG, "dtype must be PCM_F32 or PCM_F16");
    if (max_iter < 1) return fail(PCM_E_ARG, "max_iter must be >= 1");
    pcm_engine *e = new pcm_engine();
    e->device = device;
    e->d = d;
    e->k = k;
    e->dtype = dtype;
    e->max_iter_cap = max_iter;
    int rc = check_device(e);
    if (rc) { delete e; return rc; }
    if (hipDeviceGetAttribute(&e->num_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        e->num_cu < 1)
        e->num_cu = 256;
    const size_t nstat = (size_t)k * (d + 1) + 1;
    hipError_t err = hipSuccess;
    err = err ? err : e->C.ensure((size_t)k * sizeof(float4));
    err = err ? err : e->Cn.ensure((size_t)k * sizeof(float4));
    err = err ? err : e->cref.ensure((size_t)2 * k * sizeof(float4));
    err = err ? err : e->shbuf.ensure((size_t)k * sizeof(double));
    err = err ? err : e->upart.ensure((size_t)blocks_for(k, UPD_TPB) * sizeof(UpdPart));
    err = err ? err : e->prev.ensure(nstat * sizeof(unsigned long long));
    err = err ? err : e->time_sink.ensure((size_t)k * (d + 1) * sizeof(unsigned long long));
    err = err ? err : e->stats_own.ensure(nstat * sizeof(unsigned long long));
    e->stats = e->stats_own;
    err = err ? err : e->held.ensure(nstat * sizeof(unsigned long long));
    err = err ? err : e->hist_changed.ensure((size_t)max_iter * sizeof(unsigned long long));
    err = err ? err : e->hist_shift.ensure((size_t)max_iter * sizeof(double));
    err = err ? err : e->ctrl.ensure(sizeof(Ctrl));
    err = err ? err : e->bbox_part.ensure((size_t)BBOX_BLOCKS * 2 * MAXD * sizeof(float));
    err = err ? err : e->nonfinite.ensure(sizeof(unsigned));
    err = err ? err : e->bbox_out.ensure(2 * MAXD * sizeof(double));
    err = err ? err : e->cand_stats.ensure(6 * sizeof(unsigned long long));
    err = err ? err : e->empty_idx.ensure((size_t)k * sizeof(int));
    err = err ? err : e->ntiles_dev.ensure(2 * sizeof(uint32_t));
    err = err ? err : e->zpts.ensure(32 * 16 * sizeof(unsigned long long));
    err = err ? err : hipHostMalloc((void **)&e->ntiles_host, sizeof(uint32_t), hipHostMallocDefault);
    err = err ? err : hipHostMalloc((void **)&e->ctrl_pin, sizeof(Ctrl), hipHostMallocDefault);
    err = err ? err : hipEventCreateWithFlags(&e->st_ev, hipEventDisableTiming);
    err = err ? err : hipMemset(e->ctrl, 0, sizeof(Ctrl));
    if (err != hipSuccess) {
        pcm_engine_destroy(e);
        return fail(PCM_E_NOMEM, std::string("engine allocation: ") + hipGetErrorString(err));
    }
    // candidate-list reuse: budget = alpha x the last centre shift, at most kappa x
    // the smallest cell width (tuning sweeps may override; alpha = 0 disables reuse)
    if (const char *v = std::getenv("PCM_DRIFT_ALPHA")) e->drift_alpha = std::atof(v);
    if (const char *v = std::getenv("PCM_DRIFT_KAPPA")) e->drift_kappa = std::atof(v);
    *out = e;
    return 0;
}

int pcm_engine_destroy(pcm_engine *e) {
    if (!e) return 0;
    for (int i = 0; i < pcm_engine::TEV; ++i)
        for (int j = 0; j < 4; ++j)
            if (e->ev[i][j]) (void)hipEventDestroy(e->ev[i][j]);
    for (DevMem *m : e->bufs) (void)m->release();   // every device buffer the engine owns
    if (e->ntiles_host) (void)hipHostFree(e->ntiles_host);
    if (e->ctrl_pin) (void)hipHostFree(e->ctrl_pin);
    if (e->st_ev) (void)hipEventDestroy(e->st_ev);
    delete e;
    return 0;
}

static int launch_candidates(pcm_engine *e, hipStream_t s, int gate);

int pcm_fit_begin(pcm_engine *e, const float *C0, double tol, int max_iter, void *stream) {
    if (!e || !C0) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    if (max_iter < 1 || max_iter > e->max_iter_cap) return fail(PCM_E_ARG, "max_iter exceeds the engine's cap");
    if (!(tol >= 0.0)) return fail(PCM_E_ARG, "tol must be >= 0");
    if (int rc = check_device(e)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int rc = dispatch_d(e->d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        k_centers_in<D><<<blocks_for(e->k), 256, 0, s>>>(C0, e->k, e->C);
        LAUNCHCHK();
        return 0;
    });
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(e->lab, 0xff, (size_t)e->npad * lsize(e), s));   // "no label yet" (-1 / 0xffff)
    // previous raw statistics := 0: iteration 0 "converges" only for an empty cloud,
    // as sklearn's labels-vs-(-1) comparison does
    {   // prev, stats and the histories := 0 in one launch (four memsets: ~5 us each);
        // time_sink is never read, so it is not zeroed
        const long long w = (long long)e->k * (e->d + 1);
        ZeroSpans z{};
        z.p[0] = e->prev;         z.n[0] = w + 1;
        z.p[1] = e->stats;        z.n[1] = w + 1;
        z.p[2] = e->hist_changed; z.n[2] = e->max_iter_cap;
        z.p[3] = reinterpret_cast<unsigned long long *>(e->hist_shift.get()); z.n[3] = e->max_iter_cap;   // 0.0 = all-zero bits
        long long tot = 0;
        for (int q = 0; q < 4; ++q) tot += z.n[q];
        k_zero_spans<<<(int)std::min<long long>(1024, (tot + 255) / 256), 256, 0, s>>>(z);
        LAUNCHCHK();
    }
    e->ctrl_host = Ctrl{};
    e->ctrl_host.max_iter = (uint32_t)max_iter;
    e->ctrl_host.tol = tol;
    HIPCHK(hipMemcpyAsync(e->ctrl, &e->ctrl_host, sizeof(Ctrl), hipMemcpyHostToDevice, s));
    {   // read per fit, so tests and A/B runs can switch it between fits of one process
        const char *v = std::getenv("PCM_SOLE");
        e->sole_on = !(v && std::atoi(v) == 0);
        const char *f = std::getenv("PCM_FAST");
        e->fast_on = !(f && std::atoi(f) == 0);
        const char *tc = std::getenv("PCM_TILECOST");
        e->tilecost_on = !(tc && std::atoi(tc) == 0);
    }
    e->fit_ready = true;
    // candidate lists of C0 (later iterations get theirs from k_lists / the resume path)
    if (int rc2 = launch_candidates(e, s, 0)) return rc2;
    return tiles_order_lpt(e, s);
}

// Candidate blocks per coarse cell: enough blocks to fill the chip on small
// (sharded) clouds; D = 4 coarse cells hold 256 fine cells.
// Measured (round-2 bpc sweep, tools/sweep.sh PCM_CAND_BPC_RT): 12.5M-point shard (64 coarse cells) 8 -> 39 us
// vs 4 -> 47 us per update; 100M (512 coarse cells) 1; D = 4, K = 4096: 32.
// Fine grids (short lists, the 8-slot k_lloyd1: an 8-way slab, 64 coarse cells)
// want about one block per CU (round-3 slab sweep, profiles/r3x_slab_sweep.txt:
// bpc 4 -> 18.6 us, 2 -> 19.2, 8 -> 21.0, 16 -> 31.2 per update).
static int cand_bpc(const pcm_engine *e) {
    if (const char *ov = std::getenv("PCM_CAND_BPC_RT")) return std::max(1, std::atoi(ov));   // tuning sweeps only
    if (e->d >= 4) return 32;
    const long long per = (lloyd_slots(e) == 8 ? 1LL : 2LL) * e->num_cu;
    long long b = (per + e->g.ncoarse - 1) / std::max(1LL, e->g.ncoarse);
    return (int)std::max(1LL, std::min(8LL, b));
}

// D = 4 coarse cells hold 4^4 = 256 fine cells and long lists: their lists are
// built in three levels -- k_coarse (one block per coarse cell, all K centres,
// once) -> one block per mid cell (2^4 fine cells) refining its coarse parent's
// list -> its 16 fine cells (k_cand / k_lists with FC = 2) -- instead of 32
// blocks per coarse cell each recomputing the coarse list and then pruning it
// per fine cell (config-5 shard: 252 us of k_cand per iteration).
static bool split_coarse(const pcm_engine *e) { return e->g.prune && e->d >= 4; }
static long long n_mid(const pcm_engine *e) {
    long long m = 1;
    for (int a = 0; a < e->d; ++a) m *= (e->g.G[a] + 1) / 2;
    return m;
}

// coarse-list storage of the current layout (split layouts only)
static int ensure_coarse(pcm_engine *e) {
    if (!split_coarse(e)) return 0;
    const int cap = e->d >= 4 ? cand_capc<4>() : cand_capc<3>();
    HIPCHK(e->cl_cnt.ensure((size_t)e->g.ncoarse * sizeof(uint32_t)));
    HIPCHK(e->cl_idx.ensure((size_t)e->g.ncoarse * cap * sizeof(int32_t)));
    return 0;
}

// k_lloyd1 and the per-tile kernels: one block per tile of the layout (the
// exact count, read back at layout time).  Measured at config 3: 211 us per
// launch with one tile per block vs 238 us for as many persistent blocks as are
// co-resident walking tiles b, b + G, ... (each tile's list install stalled its
// block; with one tile per block the other resident blocks keep streaming);
// config-5 shape 485 vs 536 us.
static int lloyd_grid(const pcm_engine *e) { return (int)std::max(1LL, e->ntiles >= 0 ? e->ntiles : e->ntiles_cap); }

// Owner words of the current layout for the list builders (SoleW).
static SoleW sole_args(const pcm_engine *e) {
    SoleW sw;
    sw.tiles = e->tiles;
    sw.tile_off = e->tile_off;
    sw.tpos = e->tiles_lpt ? e->tpos : nullptr;
    sw.on = e->sole_on ? 1 : 0;
    return sw;
}

static int launch_candidates(pcm_engine *e, hipStream_t s, int gate) {
    if (int rc = ensure_coarse(e)) return rc;
    return host_candidates(e->d, e->g, e->C, e->k, e->ctrl, gate, split_coarse(e), cand_bpc(e), e->fc_cnt, e->fc_rec,
                           e->fc_lab, e->cref, e->cl_cnt, e->cl_idx, sole_args(e), s);
}

// Tile lists of the crowded cells at the current centres (before every assign
// launch of a crowded layout; gate: skip when the fit has halted or finished).
static int launch_tile_lists(pcm_engine *e, hipStream_t s, int gate) {
    if (e->zlev <= 0 || e->n == 0) return 0;
    return dispatch_d(e->d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        k_tile_cand<D><<<lloyd_grid(e), 256, 0, s>>>(e->tiles, e->ntiles_dev, e->fc_cnt, e->tbox, e->C, e->k,
                                                          e->tl_cnt, e->tl_rec, e->tl_lab, e->ctrl, gate);
        LAUNCHCHK();
        return 0;
    });
}

// Persistent grid: as many 256-thread blocks as are co-resident (occupancy
// query), never more blocks than tiles.
// k_label's grid: one block per tile (round 6: 247-249 -> 235-237 us per final
// E-step at config 3 against the co-resident persistent grid, as k_lloyd1
// measured in round 2; profiles/rd6_klabel_grid_ab.txt).  PCM_ASSIGN_BLOCKS_PER_CU
// (A/B) restores a persistent grid of that many blocks per CU.
static int assign_grid(pcm_engine *e) {
    const long long nt = e->ntiles >= 0 ? e->ntiles : e->ntiles_cap;
    if (const char *ov = std::getenv("PCM_ASSIGN_BLOCKS_PER_CU"))
        return (int)std::max(1LL, std::min<long long>(nt, (long long)std::max(1, std::atoi(ov)) * e->num_cu));
    return (int)std::max(1LL, nt);
}

// Lane slots of the launched k_lloyd1: 8 on fine grids, else LSLOT.  D = 4
// (config 5: lists of ~8, up to 27) takes 8 slots since the slot map gives them
// to the candidates nearest each tile (k_lloyd1): 11.5 instead of 21.8 KB of
// LDS words per block, 5 instead of 3 waves per SIMD -- config-5 shard 404 ->
// 325 us per launch, 8-way slab 270 -> 220 us (round 4; PCM_D4_LS8=0 restores 16).
static int assign_ls(const pcm_engine *e) {
    static const bool d4_ls8 = [] { const char *v = std::getenv("PCM_D4_LS8"); return !v || std::atoi(v); }();
    return ((e->d <= 3 || d4_ls8) && lloyd_slots(e) == 8) ? 8 : LSLOT;
}

static LloydArgs lloyd_args(pcm_engine *e) {
    LloydArgs A{};
    A.xcd = ((xcd_mode() >> 1) & 1) && !e->tiles_lpt;   // an ordered tile list is dealt round-robin
    A.fast = e->fast_on ? 1 : 0;
    A.tilecost = e->tilecost_on ? 1 : 0;
    A.xs = e->xs;
    A.xz = e->use_xz ? e->xz : nullptr;
    A.tmeta = e->use_xz ? e->tmeta : nullptr;
    A.npad = e->npad;
    A.tiles = e->tiles;
    A.tsum = e->tsum;
    A.ntiles = e->ntiles_dev;
    A.fc_rec = e->fc_rec;
    A.fc_lab = e->fc_lab;
    A.C = e->C;
    A.fc_cnt = e->fc_cnt;
    A.K = e->k;
    for (int a = 0; a < MAXD; ++a) A.q[a] = e->qe.q[a];
    A.stats = e->stats;
    A.ctrl = e->ctrl;
    A.sub_start = e->sub_start;
    A.sub = e->sub;
    A.g = e->g;
    A.tl_cnt = e->zlev > 0 ? e->tl_cnt : nullptr;
    A.tl_rec = e->zlev > 0 ? e->tl_rec : nullptr;
    A.tl_lab = e->zlev > 0 ? e->tl_lab : nullptr;
    A.tbox = e->zlev > 0 ? e->tbox : nullptr;
    return A;
}

// E-step with the current centres: candidate lists, then labels (sorted
// order, e->lab) and, when inert is non-null, the exact inertia limbs added
// into inert[0..3].  Not gated.
static int launch_labels(pcm_engine *e, hipStream_t s, unsigned long long *inert) {
    if (int rc = launch_candidates(e, s, 0)) return rc;
    if (int rc = launch_tile_lists(e, s, 0)) return rc;
    LloydArgs A = lloyd_args(e);
    return dispatch_td(e->dtype, e->d, [&](auto T, auto DD) -> int {
        using TT = decltype(T);
        constexpr int D = decltype(DD)::value;
        if (e->n == 0) return 0;
        return dispatch_l(e, [&](auto L) -> int {
            using LT = decltype(L);
            // inertia limbs: per-block replica lines, folded into inert[] afterwards
            unsigned long long *rep = inert ? &e->ctrl->inert_rep[0][0] : nullptr;
            k_label<TT, D, LT><<<assign_grid(e), TPB, 0, s>>>(A, e->lab, rep, e->iscale);
            LAUNCHCHK();
            if (inert) {
                k_inert_fold<<<1, 64, 0, s>>>(rep, inert);
                LAUNCHCHK();
            }
            return 0;
        });
    });
}

// Fold completed event pairs into the sums (non-blocking unless the ring is full).
static int timing_drain(pcm_engine *e, bool block) {
    while (e->ev_pending > 0) {
        int slot = (e->ev_next - e->ev_pending + pcm_engine::TEV) % pcm_engine::TEV;
        if (block) HIPCHK(hipEventSynchronize(e->ev[slot][3]));
        else if (hipEventQuery(e->ev[slot][3]) != hipSuccess) return 0;
        float a = 0, b = 0, c = 0;
        HIPCHK(hipEventElapsedTime(&a, e->ev[slot][0], e->ev[slot][1]));
        HIPCHK(hipEventElapsedTime(&b, e->ev[slot][1], e->ev[slot][2]));
        HIPCHK(hipEventElapsedTime(&c, e->ev[slot][2], e->ev[slot][3]));
        e->t_sum[1] += a;   // candidates
        e->t_sum[0] += b;   // assign
        e->t_sum[2] += c;   // fold + global
        e->t_count++;
        e->ev_pending--;
    }
    return 0;
}

static int timing_mark(pcm_engine *e, int which, hipStream_t s) {
    if (!e->timing) return 0;
    if (which == 0) {
        if (e->ev_pending == pcm_engine::TEV)
            if (int rc = timing_drain(e, true)) return rc;
        if (!e->ev[e->ev_next][0])
            for (int j = 0; j < 4; ++j) HIPCHK(hipEventCreate(&e->ev[e->ev_next][j]));
    }
    HIPCHK(hipEventRecord(e->ev[e->ev_next][which], s));
    if (which == 3) {
        e->ev_next = (e->ev_next + 1) % pcm_engine::TEV;
        e->ev_pending++;
    }
    return 0;
}

// k_lloyd (its candidate lists were built by the previous k_lists, the resume
// path or pcm_fit_begin).  It accumulates into `target`: e->stats in every fit
// (the statistics buffer -- one GPU or the all-reduce / peer-exchange buffer
// of several -- zeroed by the previous update, k_resume or fit_begin), or the
// throw-away e->time_sink of the assign-timing calibration (pcm_time_assign).
static int iter_local_impl(pcm_engine *e, hipStream_t s, unsigned long long *target) {
    if (int rc = timing_mark(e, 0, s)) return rc;
    if (int rc = launch_tile_lists(e, s, 1)) return rc;   // crowded layouts only
    if (int rc = timing_mark(e, 1, s)) return rc;
    LloydArgs A = lloyd_args(e);
    A.stats = target;
    return dispatch_td(e->dtype, e->d, [&](auto T, auto DD) -> int {
        using TT = decltype(T);
        constexpr int D = decltype(DD)::value;
        if (e->n > 0) {
            // lane slots per thread: 8 on fine grids (>= 8 cells per centre: lists
            // of ~3 at config 3; 13.5 KB of LDS -> 5 waves/SIMD, 247 -> 237 us),
            // else 16 (12.5M-point shard: lists of ~6, 53 vs 57 us)
            auto launch = [&](auto LSc) {
                constexpr int LS = decltype(LSc)::value;
                // crowded layouts: + the long tile lists' int64 words (AccL::gwords)
                const size_t lds = e->zlev > 0 ? AccL<D, LS>::bytes_crowded
                                                : (size_t)AccL<D, LS>::words * sizeof(uint32_t);
                if (e->zlev > 0)   // crowded layout (sub-cell masks off: e->sub = 0)
                    k_lloyd1<TT, D, LS, false, true><<<lloyd_grid(e), TPB, lds, s>>>(
                        A, e->tiles, e->fc_rec, e->fc_lab, e->C, e->fc_cnt, e->tl_rec);
                else
                    k_lloyd1<TT, D, LS, (D <= 3 && LS == LSLOT)><<<lloyd_grid(e), TPB, lds, s>>>(
                        A, e->tiles, e->fc_rec, e->fc_lab, e->C, e->fc_cnt, e->C);
            };
            // coarse grids keep 16 slots with masks: 8 slots + LDS int64 words 42.0 -> 51.2 us,
            // 12 slots + global atomics 42.6 -> 65.7 us at 12.5M (tools/mls_sweep.sh)
            if (assign_ls(e) == 8) launch(std::integral_constant<int, 8>{});
            else launch(std::integral_constant<int, LSLOT>{});
            LAUNCHCHK();
        }
        return timing_mark(e, 2, s);
    });
}

int pcm_iter_local(pcm_engine *e, void *stream) {
    if (!e) return fail(PCM_E_ARG, "null engine");
    if (!e->fit_ready) return fail(PCM_E_STATE, "pcm_fit_begin must run first");
    return iter_local_impl(e, (hipStream_t)stream, e->stats);   // the caller all-reduces it
}

// Centre update + next candidate lists, reading `stats` (the summed statistics)
// in place.  D <= 3, K <= 1024: k_updlists does both in one launch.  Otherwise
// k_upd1 (K <= UPD1_MAX) or k_upd (the K new centres once, convergence,
// history), then k_lists (C := new centres, each block's lists rebuilt or
// refreshed; D = 4 pruned grids: k_coarse first, then one block per mid cell).
// The relocation resume takes k_resume + k_cand.
static int iter_global_impl(pcm_engine *e, hipStream_t s, bool resume_path) {
    int rc = dispatch_d(e->d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        if (resume_path) {
            k_resume<D><<<1, SHIFT_LANES, 0, s>>>(e->stats, e->k, e->qe, e->C, e->Cn, e->hist_changed, e->hist_shift,
                                                  e->ctrl);
            LAUNCHCHK();
            return launch_candidates(e, s, 1);
        }
        double wmin = 0.0;
        for (int a = 0; a < D; ++a)
            if (e->g.ext[a] > 0 && (wmin == 0.0 || e->g.w[a] < wmin)) wmin = e->g.w[a];
        const double dl_cap = e->drift_kappa * wmin;
        const int bpc = cand_bpc(e);
        const int nlist = (int)(e->g.ncoarse * bpc);
        if constexpr (D <= 3) {
            // (PCM_FUSED_UPD=0: k_upd1 + k_lists instead -- A/B and tests; read per
            // launch so tests can switch it between fits, captured graphs keep theirs)
            const char *fz = std::getenv("PCM_FUSED_UPD");
            if (!(fz && std::atoi(fz) == 0) && e->k <= 2 * CAND_TPB) {
                auto fused = [&](auto RR) {
                    constexpr int RV = decltype(RR)::value;
                    const size_t lds = (size_t)e->k * sizeof(float4);
                    // a dedicated publisher block when one more block still fits the residency
                    // (PCM_UPD_PUB=0: always the last arriver -- A/B only)
                    static const int pub_env = [] { const char *v = std::getenv("PCM_UPD_PUB"); return v ? std::atoi(v) : 1; }();
                    int per_cu = 0;
                    const bool pub = pub_env &&
                        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_updlists<D, RV, true>,
                                                                     CAND_TPB, lds) == hipSuccess &&
                        (long long)nlist + 1 <= (long long)per_cu * e->num_cu;
                    auto kern = pub ? k_updlists<D, RV, true> : k_updlists<D, RV, false>;
                    kern<<<nlist + (pub ? 1 : 0), CAND_TPB, lds, s>>>(
                        e->stats, e->k, e->qe, e->held, e->prev, e->C, e->cref, e->hist_changed, e->hist_shift, e->ctrl,
                        e->drift_alpha, dl_cap, e->g, e->fc_cnt, e->fc_rec, e->fc_lab, bpc, sole_args(e));
                };
                if (e->k <= CAND_TPB) fused(std::integral_constant<int, 1>{});
                else fused(std::integral_constant<int, 2>{});
                LAUNCHCHK();
                return 0;
            }
        }
        // one block (the shift tree in LDS, no hand-off between blocks) up to UPD1_MAX centres
        auto upd1 = [&](auto RR) {
            k_upd1<D, decltype(RR)::value><<<1, SHIFT_LANES, 0, s>>>(
                e->stats, e->k, e->qe, e->held, e->prev, e->C, e->Cn, e->cref, e->hist_changed, e->hist_shift, e->ctrl,
                e->drift_alpha, dl_cap);
        };
        if (e->k <= SHIFT_LANES)
            upd1(std::integral_constant<int, 1>{});
        else if (e->k <= UPD1_MAX)
            upd1(std::integral_constant<int, 2>{});
        else
            k_upd<D><<<blocks_for(e->k, UPD_TPB), UPD_TPB, 0, s>>>(
                e->stats, e->k, e->qe, e->held, e->prev, e->C, e->Cn, e->cref, e->shbuf, e->upart, e->hist_changed,
                e->hist_shift, e->ctrl, e->drift_alpha, dl_cap);
        LAUNCHCHK();
        auto lists = [&](auto kern, long long grid, int tpb, size_t lds, int blocks_per_cell, CoarseL cl) {
            kern<<<(int)grid, tpb, lds, s>>>(e->g, e->Cn, e->C, e->cref, e->k, e->ctrl, e->fc_cnt, e->fc_rec, e->fc_lab,
                                             blocks_per_cell, cl, sole_args(e));
        };
        if constexpr (D >= 4) {
            if (split_coarse(e)) {
                if (int rc = ensure_coarse(e)) return rc;
                k_coarse<D><<<(int)e->g.ncoarse, CAND_TPB, 0, s>>>(e->g, e->Cn, e->k, e->ctrl, 1, e->cl_cnt, e->cl_idx);
                LAUNCHCHK();
                CoarseL cl;
                cl.in_cnt = e->cl_cnt;
                cl.in_idx = e->cl_idx;
                lists(k_lists<D, 2, false, 256>, n_mid(e), 256, 0, 1, cl);   // mid-cell blocks of 256 threads
                LAUNCHCHK();
                return 0;
            }
        }
        if (e->k <= LISTS_STAGE_MAX)   // centres staged in LDS
            lists(k_lists<D, 4, true>, nlist, CAND_TPB, (size_t)e->k * sizeof(float4), bpc, CoarseL{});
        else
            lists(k_lists<D>, nlist, CAND_TPB, 0, bpc, CoarseL{});
        LAUNCHCHK();
        return 0;
    });
    if (rc) return rc;
    return timing_mark(e, 3, s);
}

int pcm_iter_global(pcm_engine *e, void *stream) {
    if (!e) return fail(PCM_E_ARG, "null engine");
    if (!e->fit_ready) return fail(PCM_E_STATE, "pcm_fit_begin must run first");
    return iter_global_impl(e, (hipStream_t)stream, false);
}

int pcm_timing(pcm_engine *e, int enable) {
    if (!e) return fail(PCM_E_ARG, "null engine");
    if (int rc = timing_drain(e, true)) return rc;
    e->timing = enable != 0;
    e->t_sum[0] = e->t_sum[1] = e->t_sum[2] = 0.0;
    e->t_count = 0;
    return 0;
}

int pcm_timing_read(pcm_engine *e, double *ms, int *count) {
    if (!e || !ms || !count) return fail(PCM_E_ARG, "bad argument");
    if (int rc = timing_drain(e, true)) return rc;
    for (int i = 0; i < 3; ++i) ms[i] = e->t_count ? e->t_sum[i] / (double)e->t_count : 0.0;
    *count = (int)e->t_count;
    return 0;
}

// Calibration of the assign kernel's launch duration: `reps` back-to-back
// launches on the current layout, lists and centres between ONE HIP event pair
// (no per-launch events, no k_step between them).  The statistics they add are
// discarded: the fit must restart with pcm_fit_begin.
int pcm_time_assign(pcm_engine *e, int reps, void *stream, double *ms) {
    if (!e || !ms || reps < 1) return fail(PCM_E_ARG, "bad argument");
    if (!e->fit_ready) return fail(PCM_E_STATE, "pcm_fit_begin must run first");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = timing_drain(e, true)) return rc;
    // a halted or finished fit gates k_lloyd1 off: its launches would time nothing
    uint32_t flags[2] = {0u, 0u};
    HIPCHK(hipMemcpyAsync(flags, e->ctrl, sizeof(flags), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flags[0] | flags[1]) return fail(PCM_E_STATE, "the fit has halted or finished: nothing to time");
    // events and the engine's timing flag are restored on every exit path
    struct Guard {
        pcm_engine *e;
        bool was;
        hipEvent_t a = nullptr, b = nullptr;
        ~Guard() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
            e->timing = was;
        }
    } g{e, e->timing};
    e->timing = false;
    HIPCHK(hipEventCreate(&g.a));
    HIPCHK(hipEventCreate(&g.b));
    HIPCHK(hipEventRecord(g.a, s));
    int rc = 0;
    for (int i = 0; i < reps && !rc; ++i) rc = iter_local_impl(e, s, e->time_sink);
    e->fit_ready = false;   // the contract: the fit restarts with pcm_fit_begin
    if (rc) return rc;
    HIPCHK(hipEventRecord(g.b, s));
    HIPCHK(hipEventSynchronize(g.b));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, g.a, g.b));
    *ms = (double)t / reps;
    return 0;
}

// Single-process iterations: the multi-GPU sequence without the all-reduce --
// k_lloyd1 into the statistics buffer, then the update reading it in place (its
// publisher zeroes it once every block has read it).
int pcm_iterate(pcm_engine *e, int n, void *stream) {
    if (!e || n < 0) return fail(PCM_E_ARG, "bad argument");
    if (!e->fit_ready) return fail(PCM_E_STATE, "pcm_fit_begin must run first");
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < n; ++i) {
        if (int rc = iter_local_impl(e, s, e->stats)) return rc;
        if (int rc = iter_global_impl(e, s, false)) return rc;
    }
    return 0;
}

// The cross-rank SUM of the statistics by peer-memory writes (pcm_xchg.hip),
// between pcm_iter_local and pcm_iter_global in place of the RCCL all-reduce;
// gated by the control block like both of them.
int pcm_iter_exchange(pcm_engine *e, pcm_xchg *x, int phase, void *stream) {
    if (!e || !x) return fail(PCM_E_ARG, "null engine or exchange");
    if (!e->fit_ready) return fail(PCM_E_STATE, "pcm_fit_begin must run first");
    return pcm_xchg_launch(x, e->stats, &e->ctrl->halt, phase, (hipStream_t)stream);
}

int pcm_stats_ptr(pcm_engine *e, void **ptr, int64_t *count) {
    if (!e || !ptr || !count) return fail(PCM_E_ARG, "bad argument");
    *ptr = e->stats;
    *count = (int64_t)e->k * (e->d + 1) + 1;
    return 0;
}

int pcm_bind_stats(pcm_engine *e, void *ptr) {
    if (!e) return fail(PCM_E_ARG, "null engine");
    e->stats = ptr ? (unsigned long long *)ptr : e->stats_own;
    return 0;
}

int pcm_reloc_candidates(pcm_engine *e, int m, void *records, void *stream) {
    if (!e || m < 1 || !records) return fail(PCM_E_ARG, "bad argument");
    if (!e->fit_ready) return fail(PCM_E_STATE, "no fit in progress");
    hipStream_t s = (hipStream_t)stream;
    const long long n = e->n;
    HIPCHK(hipMemsetAsync(records, 0, (size_t)m * sizeof(RelocRec), s));
    if (n == 0) return 0;
    // keys (8 B/pt) + selection state in the layout's scratch arena (>= 12 B/pt)
    const size_t need = align_up((size_t)n * 8) + sizeof(RselState);
    if (e->ws.ensure(need) != hipSuccess) return fail(PCM_E_NOMEM, "reloc scratch");
    unsigned long long *keys = (unsigned long long *)e->ws;
    RselState *st = (RselState *)((char *)e->ws + align_up((size_t)n * 8));
    RselState h{};
    h.prefix = 0ull;
    h.m_rem = (unsigned long long)std::min<long long>(m, n);
    HIPCHK(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, s));
    // labels of the halted iteration (the iterations keep no label array)
    if (int rc = launch_labels(e, s, nullptr)) return rc;
    if (int rc = host_reloc_select(e, m, keys, st, records, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int pcm_reloc_apply(pcm_engine *e, const void *records, int n_rec, void *stream) {
    if (!e || !records || n_rec < 1) return fail(PCM_E_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(e->rank_buf.ensure((size_t)n_rec * sizeof(int)));
    int rc = dispatch_d(e->d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        k_reloc_apply<D><<<1, 256, 0, s>>>((const RelocRec *)records, n_rec, e->held, e->k, e->rank_buf,
                                           e->empty_idx, e->ctrl);
        LAUNCHCHK();
        return 0;
    });
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(e->stats, e->held, ((size_t)e->k * (e->d + 1) + 1) * sizeof(unsigned long long),
                          hipMemcpyDeviceToDevice, s));
    return iter_global_impl(e, s, true);
}

int pcm_final(pcm_engine *e, void *stream) {
    if (!e) return fail(PCM_E_ARG, "null engine");
    if (!e->fit_ready) return fail(PCM_E_STATE, "pcm_fit_begin must run first");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(e->ctrl->inert, 0, sizeof(e->ctrl->inert), s));
    return launch_labels(e, s, e->ctrl->inert);
}

int pcm_labels(pcm_engine *e, int32_t *out, void *stream) {
    if (!e || (!out && e->n > 0)) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    if (e->n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    // uint16 labels (K <= 65535): scatter into a 2 B/pt scratch that stays in the
    // Infinity Cache while the random writes land, then one sequential widen to
    // int32 -- 100M points: 1.52 vs 2.11 ms for the direct int32 scatter
    // (tools/unperm_sweep.sh; windows of 64M/32M rows: 1.88/1.93 ms).
    // PCM_UNPERM / PCM_UNPERM_WIN: tuning sweeps only.
    static const int mode = [] { const char *v = std::getenv("PCM_UNPERM"); return v ? std::atoi(v) : 3; }();
    static const long long win = [] { const char *v = std::getenv("PCM_UNPERM_WIN"); return v ? std::atoll(v) : (1LL << 40); }();
    return dispatch_l(e, [&](auto L) -> int {
        using LT = decltype(L);
        const bool a16 = ((uintptr_t)out & 15u) == 0;
        if (mode == 3 && e->has_dmap) {
            // the sort's two position maps, inverted by two run-wise gathers:
            // sorted -> between the passes -> caller rows
            if (e->ws.ensure((size_t)e->n * sizeof(LT) + 64) != hipSuccess)
                return fail(PCM_E_NOMEM, "labels scratch");
            LT *mid = (LT *)e->ws;   // 256-B aligned scratch
            const uint32_t *m1 = e->dmap + e->n;   // the second pass's map: 16-B aligned iff n % 4 == 0
            const int g4 = (int)blocks_for((e->n + 3) / 4);
            const int xg = (xcd_mode() >> 2) & 1;
            if (((uintptr_t)m1 & 15u) == 0)
                k_lab_gather4<LT, LT, true, true><<<g4, 256, 0, s>>>(m1, (const LT *)e->lab, e->n, mid, xg);
            else
                k_lab_gather4<LT, LT, false, true><<<g4, 256, 0, s>>>(m1, (const LT *)e->lab, e->n, mid, xg);
            LAUNCHCHK();
            if (a16)
                k_lab_gather4<LT, int32_t, true, true><<<g4, 256, 0, s>>>(e->dmap, mid, e->n, out, xg);
            else
                k_lab_gather4<LT, int32_t, true, false><<<g4, 256, 0, s>>>(e->dmap, mid, e->n, out, xg);
            LAUNCHCHK();
            return 0;
        }
        if (mode >= 1 && std::is_same<LT, uint16_t>::value && a16) {
            // uint16 scatter into scratch (n * 2 B), in destination windows, then a sequential widen
            if (e->ws.ensure((size_t)e->n * 2 + 64) != hipSuccess) return fail(PCM_E_NOMEM, "labels scratch");
            uint16_t *t16 = (uint16_t *)e->ws;
            for (long long r0 = 0; r0 < e->n; r0 += win) {
                const long long r1 = std::min<long long>(e->n, r0 + win);
                k_unpermute_win<LT, uint16_t><<<blocks_for(e->n), 256, 0, s>>>((const LT *)e->lab, e->perm, e->n,
                                                                               (uint32_t)r0, (uint32_t)r1, t16);
                LAUNCHCHK();
            }
            k_widen_u16<<<blocks_for((e->n + 3) / 4), 256, 0, s>>>(t16, e->n, out);
            LAUNCHCHK();
            return 0;
        }
        if (mode == 2) {
            for (long long r0 = 0; r0 < e->n; r0 += win) {
                const long long r1 = std::min<long long>(e->n, r0 + win);
                k_unpermute_win<LT, int32_t><<<blocks_for(e->n), 256, 0, s>>>((const LT *)e->lab, e->perm, e->n,
                                                                              (uint32_t)r0, (uint32_t)r1, out);
                LAUNCHCHK();
            }
            return 0;
        }
        k_unpermute<LT><<<blocks_for(e->n), 256, 0, s>>>((const LT *)e->lab, e->perm, e->n, out);
        LAUNCHCHK();
        return 0;
    });
}

int pcm_get_centers(pcm_engine *e, float *out, void *stream) {
    if (!e || !out) return fail(PCM_E_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    return dispatch_d(e->d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        k_centers_out<D><<<blocks_for(e->k), 256, 0, s>>>(e->C, e->k, out);
        LAUNCHCHK();
        return 0;
    });
}

int pcm_history(pcm_engine *e, uint64_t *changed, double *shift, int cap, void *stream) {
    if (!e || !changed || !shift || cap < 0) return fail(PCM_E_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    int c = std::min(cap, e->max_iter_cap);
    HIPCHK(hipMemcpyAsync(changed, e->hist_changed, (size_t)c * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(shift, e->hist_shift, (size_t)c * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

static void status_fill(const pcm_engine *e, const Ctrl &h, pcm_status *out) {
    out->halt = h.halt;
    out->done = h.done;
    out->iter = h.iter;
    out->n_empty = h.n_empty;
    for (int q = 0; q < 3; ++q) out->inertia_limbs[q] = h.inert[q];
    out->inertia_scale = e->iscale;
    out->inertia_overflow = (uint32_t)h.inert[3];
    out->inertia = pcm_inertia_value(out->inertia_limbs, e->iscale, out->inertia_overflow);
    out->list_rebuilds = h.rebuilds;
    out->pad_ = 0;
    out->last_changed = h.last_changed;
    out->last_shift = h.last_shift;
}

int pcm_read_status(pcm_engine *e, pcm_status *out, void *stream) {
    if (!e || !out) return fail(PCM_E_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    Ctrl h{};
    HIPCHK(hipMemcpyAsync(&h, e->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    status_fill(e, h, out);
    return 0;
}

// Status without draining the stream: post = a snapshot of ctrl queued behind
// the work enqueued so far (pinned copy + event); wait = until that snapshot
// has landed.  Lets the host queue the next chunk of iterations before it
// reads the previous chunk's status (lloyd.run), so the GPU does not idle for
// the round trip.  One snapshot in flight per engine.
int pcm_status_post(pcm_engine *e, void *stream) {
    if (!e) return fail(PCM_E_ARG, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->ctrl_pin, e->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(e->st_ev, s));
    return 0;
}

int pcm_status_wait(pcm_engine *e, pcm_status *out) {
    if (!e || !out) return fail(PCM_E_ARG, "bad argument");
    HIPCHK(hipEventSynchronize(e->st_ev));
    status_fill(e, *e->ctrl_pin, out);
    return 0;
}

int pcm_assign_kernel_name(pcm_engine *e, char *buf, size_t n) {
    if (!e || !buf || n == 0) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    const int ls = assign_ls(e);
    const bool mask = e->d <= 3 && ls == LSLOT && e->zlev == 0;
    std::snprintf(buf, n, "k_lloyd1<%s,%d,%d,%s%s>", e->dtype == PCM_F16 ? "__half" : "float", e->d, ls,
                  mask ? "true" : "false", e->zlev > 0 ? ",crowded" : "");
    return 0;
}

// Debug (not in the public header): copy the sorted layout to device buffers
// (xs in the AoSoA-4 order of pcm_layout.hpp xs_index).  Here, beside pcm_labels, which
// instantiates the same k_unpermute.
int pcm_debug_layout(pcm_engine *e, void *xs_out, int32_t *lab_out, uint32_t *perm_out, void *stream) {
    if (!e || !e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(xs_out, e->xs, (size_t)e->d * e->npad * tsize(e->dtype), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(perm_out, e->perm, (size_t)e->n * 4, hipMemcpyDeviceToDevice, s));
    return dispatch_l(e, [&](auto L) -> int {
        using LT = decltype(L);
        k_unpermute<LT><<<blocks_for(e->n), 256, 0, s>>>((const LT *)e->lab, nullptr, e->n, lab_out);
        LAUNCHCHK();
        return 0;
    });
}

// Debug (not in the public header): the integers of the built layout, out[0 .. 20):
// sub, zlev, tile_cap, npad, ntiles, ntiles_cap, the sort plan's bits, npass, wb, nblk, nseg,
// has_dmap, use_xz, tiles_lpt, bytes per sorted-order label, ncells, n, d, prune, k.
// Reads host state only.
int pcm_debug_layout_facts(pcm_engine *e, int64_t *out, int cap) {
    if (!e || !out || cap < 20) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    const int64_t f[20] = {e->sub, e->zlev, (int64_t)e->tile_cap, e->npad, e->ntiles, e->ntiles_cap, e->rs_bits,
                           e->rs_npass, e->rs_wb, e->rs_nblk, e->rs_nseg, e->has_dmap, e->use_xz, e->tiles_lpt,
                           (int64_t)lsize(e), e->g.ncells, e->n, e->d, e->g.prune, e->k};
    std::copy(f, f + 20, out);
    return 0;
}

// Debug (not in the public header): one named buffer of the built layout copied to the caller's
// device buffer `out` of exactly `bytes` bytes; *need (optional) = the buffer's size, also when the
// copy is refused for its size (out null: the size query alone).  A buffer the layout does not have
// (no compressed stream, no position maps, ...) is PCM_E_STATE.  Copies only: the engine's state
// and its scratch stay as they are.
int pcm_debug_layout_buffer(pcm_engine *e, const char *name, void *out, size_t bytes, size_t *need, void *stream) {
    if (!e || !name) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    const std::string nm(name);
    const size_t nc = (size_t)e->g.ncells, n = (size_t)e->n, nt = (size_t)std::max(0LL, e->ntiles);
    const bool pts = n > 0;
    const void *src = nullptr;
    size_t sz = 0;
    bool known = true, have = true;
    if (nm == "cell_start") { src = e->cell_start; sz = (nc + 1) * 4; }
    else if (nm == "tile_off") { src = e->tile_off; sz = (nc + 1) * 4; }
    else if (nm == "fc_cnt") { src = e->fc_cnt; sz = nc * 4; }
    else if (nm == "sub_start") { src = e->sub_start; sz = ((nc << (e->sub ? e->d : 0)) + 1) * 4; have = pts && e->zlev == 0; }
    else if (nm == "tiles") { src = e->tiles; sz = nt * sizeof(uint4); have = pts; }
    else if (nm == "tsum") { src = e->tsum; sz = nt * e->d * sizeof(long long); have = pts; }
    else if (nm == "tmeta") { src = e->tmeta; sz = nt * sizeof(uint4); have = pts && e->use_xz; }
    else if (nm == "xz") { src = e->xz; sz = align_up((size_t)e->npad) * 8; have = pts && e->use_xz; }
    else if (nm == "zpts") { src = e->zpts; sz = 32 * 16 * sizeof(unsigned long long); have = pts; }
    else if (nm == "tbox") { src = e->tbox; sz = nt * 2 * sizeof(float4); have = pts && e->zlev > 0; }
    else if (nm == "dmap") { src = e->dmap; sz = 2 * n * 4; have = pts && e->has_dmap; }
    else if (nm == "torig") { src = e->torig; sz = nt * 4; have = pts && e->tiles_lpt; }
    else if (nm == "tpos") { src = e->tpos; sz = nt * 4; have = pts && e->tiles_lpt; }
    else known = false;
    if (!known) return fail(PCM_E_ARG, "pcm_debug_layout_buffer: unknown buffer " + nm);
    if (!have) return fail(PCM_E_STATE, "pcm_debug_layout_buffer: this layout has no " + nm);
    if (need) *need = sz;
    if (!out) return 0;
    if (bytes != sz) return fail(PCM_E_ARG, "pcm_debug_layout_buffer: " + nm + " holds " + std::to_string(sz) + " bytes");
    if (sz) HIPCHK(hipMemcpyAsync(out, src, sz, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

#ifdef PCM_DBG_TIMING
// This unit's copies of the stamp arrays (pcm_debug.hpp): the list and update kernels' and k_lloyd1's.
int pcm_debug_timing(unsigned long long *out, int nblocks) {
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_t), (size_t)nblocks * 16 * sizeof(unsigned long long)));
    return 0;
}
int pcm_debug_timing_lloyd(unsigned long long *out, int nblocks) {
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_l), (size_t)nblocks * 8 * sizeof(unsigned long long)));
    return 0;
}
#endif

}  // extern "C"
