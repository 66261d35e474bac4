// pcm_host.hpp — what the host units of the Lloyd engine share (pcm_engine.hip, pcm_layout.hip,
// pcm_inspect.hip, pcm_kpp.hip, pcm_predict.hip, pcm_cloud.hip): error macros, dispatch helpers, the
// engine's state and the host functions one unit defines for the others.  No kernels: every
// template kernel is instantiated by exactly one unit, the one whose function launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "pcm_common.hpp"
#include "pcm_kcommon.hpp"   // Grid, QExp, Ctrl, MAXD
#include "pcm_kmeans.h"

#define HIPCHK(expr)                                                                                 \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return pcm_fail(PCM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " @" +   \
                                           std::to_string(__LINE__));                               \
    } while (0)

#define LAUNCHCHK() HIPCHK(hipGetLastError())

namespace pcm {
struct UpdPart;   // pcm_update.hpp
struct SoleW;     // pcm_cand.hpp
struct RselState; // pcm_util.hpp

// One grow-only device allocation.  A DevBuf<T> is the typed member of an engine that holds one
// and enters it in the engine's list, so pcm_engine_destroy frees whatever the engine owns.
// Neither type has a destructor: an engine that has allocated is deleted through pcm_engine_destroy only.
struct DevMem {
    void *p = nullptr;
    size_t cap = 0;
    // At least `need` bytes: reallocates (after freeing the old block) only when they exceed the capacity.
    hipError_t ensure(size_t need) {
        if (p && need <= cap) return hipSuccess;
        if (hipError_t err = release()) return err;
        hipError_t err = hipMalloc(&p, std::max<size_t>(need, 256));
        if (err != hipSuccess) return err;
        cap = std::max<size_t>(need, 256);
        return hipSuccess;
    }
    hipError_t release() {
        hipError_t err = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        return err;
    }
};

template <typename T>
struct DevBuf {
    DevMem m;
    explicit DevBuf(std::vector<DevMem *> &owner) { owner.push_back(&m); }
    DevBuf(const DevBuf &) = delete;
    hipError_t ensure(size_t bytes) { return m.ensure(bytes); }
    size_t cap() const { return m.cap; }
    T *get() const { return static_cast<T *>(m.p); }
    operator T *() const { return get(); }
    template <typename U> explicit operator U *() const { return static_cast<U *>(get()); }   // (TT *)e->xs
    T *operator->() const { return get(); }
};
}  // namespace pcm

struct pcm_engine {
    int device = 0, d = 3, k = 1, dtype = PCM_F32, max_iter_cap = 300;
    long long n = 0, npad = 0, gidx0 = 0;
    long long n_global = 0;          // points over all ranks (pcm_layout_shard; = n for a single-process fit)
    bool has_rows = false;           // grows holds the global row of every local point (spatial shard); else gidx0 + i
    double lo[pcm::MAXD] = {0}, hi[pcm::MAXD] = {0}, maxabs[pcm::MAXD] = {0};
    bool have_bbox = false, layout_ready = false, fit_ready = false;
    pcm::Grid g{};
    pcm::QExp qe{};
    long long ntiles = 0;            // host copy: -1 = not read back yet (pcm_layout_info reads it)
    long long ntiles_cap = 0;        // upper bound on the tiles of the current layout (grid sizing)
    uint32_t tile_cap = pcm::TILE;   // points per tile
    uint32_t *ntiles_host = nullptr; // pinned: the layout's tile count, read back at the end of pcm_layout_build
    pcm::Ctrl *ctrl_pin = nullptr;   // pinned snapshot of ctrl (pcm_status_post / pcm_status_wait)
    hipEvent_t st_ev = nullptr;
    bool use_xz = false;             // the current layout has a compressed stream
    bool tiles_lpt = false;          // tiles ordered longest candidate list first (PCM_TILE_LPT, A/B)
    bool sole_on = true;             // PCM_SOLE=0 (A/B, read by pcm_fit_begin): every owner word stays 0
    bool fast_on = true;             // PCM_FAST=0 (A/B and tests, read by pcm_fit_begin): every tile takes k_lloyd1's generic body
    bool tilecost_on = true;         // PCM_TILECOST=0 (A/B and tests, read by pcm_fit_begin): a wave computes every round of its tile, in range or not
    int zlev = 0;                    // crowded layouts (tight clusters): Morton levels of the in-cell order and the tile lists
    bool has_dmap = false;           // the current layout kept its sort's position maps (2-pass sorts)
    int sub = 0;                     // the current layout is sorted by sub-cell
    int rs_bits = 0, rs_npass = 0, rs_wb = 0;   // the current layout's sort plan (RsPlan), kept for
    long long rs_nblk = 0, rs_nseg = 0;         // pcm_debug_layout_facts only
    int num_cu = 256;
    double drift_alpha = 2.0, drift_kappa = 0.05;  // candidate-list reuse policy (see k_upd)
    int iscale = 0;                  // exact-inertia weight exponent (from the global q)
    unsigned long long *stats = nullptr;   // stats_own, or a bound buffer the engine does not own (pcm_bind_stats)
    pcm::Ctrl ctrl_host{};

    // Device buffers: grown on demand, reused by later layouts, freed at destroy (every DevBuf
    // enters itself in `bufs`).  Those of the first group are allocated once by pcm_engine_create.
    std::vector<pcm::DevMem *> bufs;
    template <typename T> using Buf = pcm::DevBuf<T>;
    Buf<float4> C{bufs}, Cn{bufs};
    Buf<float4> cref{bufs};                    // [2][K] reference centres of the candidate lists (k_upd / k_lists)
    Buf<double> shbuf{bufs};                   // [K] squared centre shifts of one iteration (k_upd's shift tree)
    Buf<pcm::UpdPart> upart{bufs};             // [ceil(K / UPD_TPB)] k_upd's per-block records
    Buf<unsigned long long> prev{bufs};        // raw statistics of the previous iteration
    Buf<unsigned long long> time_sink{bufs};   // [K][D+1] throw-away target of pcm_time_assign's launches (never read)
    Buf<unsigned long long> stats_own{bufs};
    Buf<unsigned long long> held{bufs};        // statistics of a halted iteration
    Buf<unsigned long long> hist_changed{bufs};
    Buf<double> hist_shift{bufs};
    Buf<pcm::Ctrl> ctrl{bufs};
    Buf<float> bbox_part{bufs};
    Buf<unsigned> nonfinite{bufs};
    Buf<double> bbox_out{bufs};
    Buf<unsigned long long> cand_stats{bufs};
    Buf<int> empty_idx{bufs};                  // [K] scratch of the relocation kernel
    Buf<uint32_t> ntiles_dev{bufs};            // tile count of the current layout (written by k_tile_total)
    Buf<unsigned long long> zpts{bufs};        // points in compressed tiles (replicated device counter)
    Buf<int> rank_buf{bufs};                   // [records] scratch of pcm_reloc_apply
    Buf<uint32_t> grows{bufs};                 // global row of every local point (has_rows)
    Buf<void> xs{bufs};
    Buf<unsigned> xz{bufs};                    // compressed 8-B point records (fp32 D = 3, k_tile_compress)
    Buf<uint4> tmeta{bufs};                    // per-tile compression records
    // sole-owner tiles (SoleW, pcm_cand.hpp): a tile whose cell has a one-entry list adds tsum, unread
    Buf<long long> tsum{bufs};                 // [tile][d] fixed-point coordinate sums of the tile's points
    Buf<uint32_t> tpos{bufs}, torig{bufs};     // reordered tiles: layout tile index -> current position, and its inverse
    Buf<float4> tbox{bufs};                    // [tile][2] exact point box (crowded layouts)
    Buf<uint32_t> tl_cnt{bufs};                // [tile] list length (tiles of FULL cells) or FULL
    Buf<float4> tl_rec{bufs};                  // [tile][TLMAX]
    Buf<int32_t> tl_lab{bufs};                 // [tile][TLMAX]
    Buf<uint32_t> zcnt{bufs};                  // occupancy sample counts [ncells + 1]
    Buf<uint32_t> perm{bufs};
    Buf<uint32_t> dmap{bufs};                  // [2][n] the layout sort's per-pass position maps (labels back to row order)
    Buf<void> lab{bufs};                       // sorted-order labels: uint16 when k <= 65535, else int32
    Buf<uint32_t> cell_start{bufs};
    Buf<uint32_t> sub_start{bufs};             // [(ncells << d) + 1]: first sorted point of every sub-cell (half-cell per axis)
    Buf<uint32_t> tile_off{bufs};              // [ncells+1] first tile of each cell
    Buf<uint4> tiles{bufs};
    Buf<uint32_t> fc_cnt{bufs};
    Buf<float4> fc_rec{bufs};
    Buf<int32_t> fc_lab{bufs};
    Buf<uint32_t> cl_cnt{bufs};                // [ncoarse] coarse candidate lists (k_coarse; split layouts)
    Buf<int32_t> cl_idx{bufs};                 // [ncoarse][cand_capc]
    Buf<void> ws{bufs};                        // layout / relocation scratch arena

    // optional kernel timing: event pairs per iteration, summed on read
    static constexpr int TEV = 64;
    bool timing = false;
    hipEvent_t ev[TEV][4] = {};
    int ev_next = 0, ev_pending = 0;
    double t_sum[3] = {0, 0, 0};
    long long t_count = 0;
};

namespace pcm {

constexpr int BBOX_BLOCKS = 1024;

inline int fail(int code, const std::string &msg) { return pcm_fail(code, msg); }

inline size_t tsize(int dtype) { return dtype == PCM_F16 ? 2 : 4; }
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
inline int blocks_for(long long n, int bs = 256) { return (int)std::max(1LL, (n + bs - 1) / bs); }
inline unsigned cell_bits(long long nc) {
    unsigned b = 0;
    while ((1LL << b) < nc) ++b;
    return b;
}

// Internal sorted-order labels are uint16 when every label fits (saves 4 B/pt/iter of HBM).
inline bool small_labels(const pcm_engine *e) { return e->k <= 65535; }
inline size_t lsize(const pcm_engine *e) { return small_labels(e) ? 2 : 4; }

template <typename F>
int dispatch_d(int d, F &&f) {
    switch (d) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
    }
    return pcm_fail(PCM_E_ARG, "d must be 1..4");
}

template <typename F>
int dispatch_td(int dtype, int d, F &&f) {
    if (dtype == PCM_F16)
        return dispatch_d(d, [&](auto DD) { return f(__half{}, DD); });
    return dispatch_d(d, [&](auto DD) { return f(float{}, DD); });
}

template <typename F>
int dispatch_l(const pcm_engine *e, F &&f) {
    if (small_labels(e)) return f(uint16_t{});
    return f(int32_t{});
}

// XCD-aware block orders (xcd_block), a bit mask: 1 the sort scatters, 2 k_lloyd1's tiles, 4 the label
// gathers
inline int xcd_mode() {
    static const int m = [] { const char *v = std::getenv("PCM_XCD"); return v ? std::atoi(v) : 7; }();
    return m;
}

// LSD record sort (pcm_sort.hpp): passes, chunking and workspace offsets.
struct RsPlan {
    int npass = 1, wb = 8;
    long long nblk = 1, ent = 256;   // ent = RS_DIG * nblk
    long long nseg = 1;
    size_t o_ra = 0, o_rb = 0, o_hist = 0, o_goff = 0, o_segb = 0, total = 0;
};

// pcm_engine.hip
int check_device(pcm_engine *e);
int lloyd_slots(const pcm_engine *e);   // lane slots (8 or LSLOT) of the layout's grid
// Exact candidate lists of the centres C over the grid: `split` (D = 4 pruned grids) k_coarse, then
// k_cand<D, 2> on one block per mid cell; else k_cand<D> on bpc blocks per coarse cell.
int host_candidates(int d, const Grid &g, const float4 *C, int k, Ctrl *ctrl, int gate, bool split, int bpc,
                    uint32_t *fc_cnt, float4 *fc_rec, int32_t *fc_lab, float4 *cref, uint32_t *cl_cnt,
                    int32_t *cl_idx, const SoleW &sw, hipStream_t s);

// pcm_layout.hip
void make_grid(Grid &g, int d, const double *lo, const double *hi, double target);
// Halve the axis with the most cells until ncells <= ncells_max and ncoarse <= ncoarse_max (thin boxes).
void clamp_grid(Grid &g, long long ncells_max, long long ncoarse_max);
int inertia_scale(const int32_t *q, int d);
// Bounding box of the n > 0 rows of X into hb = {lo[d], hi[d]} (one stream synchronisation);
// PCM_E_NONFINITE when a coordinate is NaN or Inf.  part: BBOX_BLOCKS * 2 * MAXD floats, out: 2 * MAXD doubles.
int host_bbox(const void *X, int dtype, int d, long long n, float *part, unsigned *nonfinite, double *out,
              hipStream_t s, double hb[2 * MAXD]);
int rs_plan(int dtype, int d, long long n, unsigned bits, RsPlan &p);
// The cell sort of X by plan p in the workspace wb (xs: AoSoA-4, zero padded to npad; perm: sorted
// position -> row; dmaps: the per-pass position maps, or null), then the first sorted point of each
// of the nstart (sub-)cells, nstart + 1 entries.
int host_sort_cells(const void *X, int dtype, int d, long long n, long long npad, const Grid &g, int with_sub,
                    int zlev, unsigned bits, const RsPlan &p, char *wb, void *xs, uint32_t *perm, uint32_t *dmaps,
                    long long nstart, uint32_t *starts, hipStream_t s);
int tiles_order_lpt(pcm_engine *e, hipStream_t s);
// The relocation records of the (up to) m points farthest from their centres: keys of the engine's
// sorted points and labels, the radix select over them (state st), the gather into `records`.
int host_reloc_select(pcm_engine *e, int m, unsigned long long *keys, RselState *st, void *records, hipStream_t s);
// rocprim::exclusive_scan (plus) over n uint32 (tmp null: the size query), instantiated once for the layout and the cloud
hipError_t exscan_u32(void *tmp, size_t &bytes, uint32_t *in, uint32_t *out, size_t n, hipStream_t s);

}  // namespace pcm
