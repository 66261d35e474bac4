// pcm_layout.hip — the Lloyd engine's layout (pcm_layout_bbox / shard / build, pcm_engine_reserve):
// bounding box, pruning grid, the cell sort, tiles, compression and the tile order.  The bounding
// box, the grid and the sort also serve k-means++ seeding and predict (pcm_host.hpp).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "pcm_layout.hpp"
#include "pcm_sort.hpp"
#include "pcm_util.hpp"   // k_reloc_keys, k_rsel_*, k_reloc_gather
#include "pcm_host.hpp"

using namespace pcm;

namespace {

template <typename TT, int D>
void rs_plan_t(long long n, unsigned bits, RsPlan &p) {
    using R = PRec<TT, D>;
    constexpr int CH = RsCfg<TT, D>::CH;
    p.npass = std::max(1, (int)((bits + 7) / 8));
    p.wb = (int)((bits + p.npass - 1) / p.npass);
    p.nblk = std::max(1LL, (n + CH - 1) / CH);
    p.ent = (long long)RS_DIG * p.nblk;
    p.nseg = (p.nblk + RS_SEG - 1) / RS_SEG;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = (o + std::max<size_t>(bytes, 8) + 255) / 256 * 256; return at; };
    p.o_ra = take(p.npass >= 2 ? n * sizeof(R) : 0);
    p.o_rb = take(p.npass >= 3 ? n * sizeof(R) : 0);
    p.o_hist = take(p.ent * 4);
    p.o_goff = take(p.ent * 4);
    p.o_segb = take((size_t)p.nseg * RS_DIG * 4);
    p.total = o;
}

// 16-B row loads of the caller's X in the sort's first count pass (X 16-B aligned; PCM_SORT_VEC=0: the
// 4-B loads, A/B).  The same staged through LDS in the first scatter measured 899-901 -> 909-916 us
// (profiles/rd6_sort_count_vec.txt), so the scatter keeps its 4-B loads.
int sort_vec(const void *X) {
    static const int m = [] { const char *v = std::getenv("PCM_SORT_VEC"); return v ? std::atoi(v) : 1; }();
    return ((uintptr_t)X & 15u) == 0u ? m : 0;
}

// Sort the caller's rows X into cell order: AoSoA-4 xs (zero padded to npad)
// and perm (sorted position -> row).
template <typename TT, int D>
int rs_sort(const TT *X, long long n, long long npad, const Grid &g, int with_sub, int zlev, unsigned bits,
            const RsPlan &p, char *wb, TT *xs, uint32_t *perm, hipStream_t s, uint32_t *dmaps) {
    using R = PRec<TT, D>;
    R *ra = (R *)(wb + p.o_ra), *rb = (R *)(wb + p.o_rb);
    uint32_t *hist = (uint32_t *)(wb + p.o_hist), *goff = (uint32_t *)(wb + p.o_goff),
             *segb = (uint32_t *)(wb + p.o_segb);
    const int grid = (int)p.nblk;
    for (int q = 0; q < p.npass; ++q) {
        const int shift = q * p.wb, width = std::min(p.wb, (int)bits - shift);
        const bool from_x = q == 0, to_xs = q == p.npass - 1;
        const R *rin = from_x ? nullptr : (((q - 1) & 1) ? rb : ra);
        R *rout = to_xs ? nullptr : ((q & 1) ? rb : ra);
        if (from_x)
            k_rs_count<TT, D, true><<<grid, RS_CTPB, 0, s>>>(X, rin, n, g, with_sub, zlev, shift, width, hist,
                                                             sort_vec(X) & 1);
        else
            k_rs_count<TT, D, false><<<grid, RS_CTPB, 0, s>>>(X, rin, n, g, with_sub, zlev, shift, width, hist, 0);
        LAUNCHCHK();
        k_rs_colscan<<<(int)p.nseg, RS_DIG, 0, s>>>(hist, p.nblk, goff, segb);
        LAUNCHCHK();
        k_rs_segscan<<<1, RS_DIG, 0, s>>>(segb, p.nseg);
        LAUNCHCHK();
#define PCM_RS_SCATTER(FX, TX)                                                                                      \
    k_rs_scatter<TT, D, FX, TX><<<grid, RS_TPB, 0, s>>>(X, rin, n, g, with_sub, zlev, shift, width, goff, segb, rout, \
                                                        xs, perm, dmaps ? dmaps + (size_t)q * n : nullptr, xcd_mode() & 1)
        if (from_x && to_xs) PCM_RS_SCATTER(true, true);
        else if (from_x) PCM_RS_SCATTER(true, false);
        else if (to_xs) PCM_RS_SCATTER(false, true);
        else PCM_RS_SCATTER(false, false);
#undef PCM_RS_SCATTER
        LAUNCHCHK();
    }
    if (npad > n) {
        k_xs_pad<TT, D><<<1, 64, 0, s>>>(n, npad, xs);
        LAUNCHCHK();
    }
    return 0;
}

// The layout's buffers persist across layouts (a later cloud reuses them when
// they are large enough); invalidating a layout frees nothing.
void free_layout(pcm_engine *e) {
    e->layout_ready = false;
    e->fit_ready = false;
    e->has_dmap = false;
}

}  // namespace

int pcm::rs_plan(int dtype, int d, long long n, unsigned bits, RsPlan &p) {
    return dispatch_td(dtype, d, [&](auto T, auto DD) -> int {
        rs_plan_t<decltype(T), decltype(DD)::value>(n, bits, p);
        return 0;
    });
}

int pcm::host_sort_cells(const void *X, int dtype, int d, long long n, long long npad, const Grid &g, int with_sub,
                         int zlev, unsigned bits, const RsPlan &p, char *wb, void *xs, uint32_t *perm,
                         uint32_t *dmaps, long long nstart, uint32_t *starts, hipStream_t s) {
    return dispatch_td(dtype, d, [&](auto T, auto DD) -> int {
        using TT = decltype(T);
        constexpr int D = decltype(DD)::value;
        if (int rc = rs_sort<TT, D>((const TT *)X, n, npad, g, with_sub, zlev, bits, p, wb, (TT *)xs, perm, s, dmaps))
            return rc;
        // (sub-)cell starts by binary search over the sorted points (Morton-ordered cells: the keys' cell bits)
        k_cell_starts_xs<TT, D><<<blocks_for(nstart + 1), 256, 0, s>>>((const TT *)xs, n, g, with_sub, zlev, nstart,
                                                                      starts, d * zlev);
        LAUNCHCHK();
        return 0;
    });
}

// In this unit, not beside pcm_reloc_candidates: k_reloc_keys and k_reloc_gather index the sorted
// points through xs_index<D>, as the sort's kernels do, and the compiler specialises such a shared
// inline function by the callers a unit holds (argument ranges); compiled apart from k_xs_pad and
// k_cell_starts_xs the two kernels get other, shorter address arithmetic (profiles/engine_split.txt).
int pcm::host_reloc_select(pcm_engine *e, int m, unsigned long long *keys, RselState *st, void *records,
                           hipStream_t s) {
    const long long n = e->n;
    const int hblk = (int)std::min<long long>((n + 255) / 256, (long long)e->num_cu * 4);
    return dispatch_td(e->dtype, e->d, [&](auto T, auto DD) -> int {
        using TT = decltype(T);
        constexpr int D = decltype(DD)::value;
        return dispatch_l(e, [&](auto L) -> int {
            using LT = decltype(L);
            k_reloc_keys<TT, D, LT><<<blocks_for(n), 256, 0, s>>>((const TT *)e->xs, n, (const LT *)e->lab, e->perm,
                                                                 e->C, e->gidx0, e->has_rows ? e->grows : nullptr,
                                                                 keys);
            LAUNCHCHK();
            if (m < n)   // exactly the top m; m >= n takes every point (T = 0)
                for (int pass = 0; pass < 8; ++pass) {
                    k_rsel_hist<<<hblk, 256, 0, s>>>(keys, n, st, pass);
                    LAUNCHCHK();
                    k_rsel_pick<<<1, 64, 0, s>>>(st, pass);
                    LAUNCHCHK();
                }
            k_reloc_gather<TT, D, LT><<<blocks_for(n), 256, 0, s>>>(keys, n, (const TT *)e->xs, (const LT *)e->lab,
                                                                   e->qe, st, m, (RelocRec *)records);
            LAUNCHCHK();
            return 0;
        });
    });
}

hipError_t pcm::exscan_u32(void *tmp, size_t &bytes, uint32_t *in, uint32_t *out, size_t n, hipStream_t s) {
    return rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), s);
}

// Roughly cubic grid of about `target` cells over the box [lo, hi]
// (degenerate axes get one cell); F = 4 fine cells per coarse cell per axis.
void pcm::make_grid(Grid &g, int d, const double *lo, const double *hi, double target) {
    g = Grid{};
    g.d = d;
    g.F = 4;   // fixed: k_cand assumes 4 fine cells per coarse cell per axis
    target = std::max(1.0, std::min(target, (double)(1 << 18)));
    double vol = 1.0;
    int nondeg = 0;
    double maxext = 0.0;
    for (int a = 0; a < MAXD; ++a) {
        g.G[a] = 1;
        g.GC[a] = 1;
    }
    for (int a = 0; a < d; ++a) {
        double ex = hi[a] - lo[a];
        g.ext[a] = ex;
        g.lo[a] = lo[a];
        maxext = std::max(maxext, ex);
        if (ex > 0) {
            vol *= ex;
            nondeg++;
        }
    }
    if (nondeg > 0) {
        double sz = std::pow(vol / target, 1.0 / nondeg);
        for (int a = 0; a < d; ++a) {
            if (g.ext[a] > 0) {
                long long G = std::llround(g.ext[a] / sz);
                g.G[a] = (int)std::max(1LL, std::min(G, 4096LL));
            }
        }
    }
    long long nc = 1;
    for (int a = 0; a < d; ++a) nc *= g.G[a];
    while (nc > (1LL << 20)) {   // keep keys and candidate tables bounded
        int amax = 0;
        for (int a = 1; a < d; ++a)
            if (g.G[a] > g.G[amax]) amax = a;
        g.G[amax] = std::max(1, g.G[amax] / 2);
        nc = 1;
        for (int a = 0; a < d; ++a) nc *= g.G[a];
    }
    long long ncc = 1;
    for (int a = 0; a < d; ++a) {
        g.w[a] = g.ext[a] / g.G[a];
        g.inv[a] = g.ext[a] > 0 ? (double)g.G[a] / g.ext[a] : 0.0;
        g.mg[a] = 1e-7 * g.ext[a];
        g.GC[a] = (g.G[a] + g.F - 1) / g.F;
        ncc *= g.GC[a];
    }
    g.ncells = nc;
    g.ncoarse = ncc;
    // fp32 distances overflow beyond ~1.8e19: no pruning then (brute force is exact)
    g.prune = (maxext < 1e18) ? 1 : 0;
}

// make_grid's cell counts clamped to a caller's table bounds.  make_grid sizes
// the cells from the box's volume and gives every axis at least one cell, so a
// thin box (one axis far shorter than the others, yet not constant) gets far
// more cells than the target along its long axes, whatever the target.  The
// axis with the most cells is halved until the grid fits; that ends at the
// latest with one cell per axis (1 cell, 1 coarse cell).  A grid that fits is
// left as make_grid made it.  The cell count affects speed only.
void pcm::clamp_grid(Grid &g, long long ncells_max, long long ncoarse_max) {
    const int d = g.d;
    while (g.ncells > ncells_max || g.ncoarse > ncoarse_max) {
        int amax = 0;
        for (int a = 1; a < d; ++a)
            if (g.G[a] > g.G[amax]) amax = a;
        if (g.G[amax] <= 1) break;   // one cell: bounds below 1 are the caller's error
        g.G[amax] = std::max(1, g.G[amax] / 2);
        long long nc = 1, ncc = 1;
        for (int a = 0; a < d; ++a) {   // the derived fields, as make_grid sets them
            g.w[a] = g.ext[a] / g.G[a];
            g.inv[a] = g.ext[a] > 0 ? (double)g.G[a] / g.ext[a] : 0.0;
            g.GC[a] = (g.G[a] + g.F - 1) / g.F;
            nc *= g.G[a];
            ncc *= g.GC[a];
        }
        g.ncells = nc;
        g.ncoarse = ncc;
    }
}

// The Lloyd engine's pruning grid: about min(32 K, n / 2800) cells -- ~2.8k
// points per cell: fewer, fuller tiles (a tile round is 512 points) outweigh
// the slightly longer candidate lists (swept on 12.5M / 100M clouds).
static void choose_grid(pcm_engine *e) {
    // D = 4: smaller cells (~1k points) shorten the lists more than the tiles
    // cost (config-5 shape: 20736 -> 65536 cells, 913 -> 846 us per iteration)
    // (a spatial shard holds about n / n_global of the centres: the cap scales with it)
    // D = 4 slabs: 48 cells per centre (config-5 8-way slab, 13718 -> 27783 cells,
    // lists 7.1 -> 5.3, one tile per cell: 280 -> 250 us per rank; 36501 cells 265,
    // profiles/rd4_c5_slab_grid.txt); D <= 3: 32 (the config-4 slab sweep)
    const double share = e->n_global > 0 ? std::min(1.0, (double)e->n / (double)e->n_global) : 1.0;
    const double per_centre = e->d >= 4 ? 48.0 : 32.0;
    double target = std::min(per_centre * e->k * share, (double)e->n / (e->d >= 4 ? 1000.0 : 2800.0));
    if (const char *ov = std::getenv("PCM_CELL_TARGET")) target = std::atof(ov);   // tuning sweeps only
    make_grid(e->g, e->d, e->lo, e->hi, target);
    if (e->k <= 1) e->g.prune = 0;
}

// Exact-inertia exponent s (oracle/lloyd_ref.py inertia_scale): the global
// exponents give |x_a|, |c_a| < 2^(QBITS - q_a), so every canonical distance
// is below bound = sum_a 4^(QBITS + 1 - q_a) (times 1 + 2^-20 for rounding);
// s = 64 - e with bound' < 2^e keeps trunc(d * 2^s) < 2^64.
int pcm::inertia_scale(const int32_t *q, int d) {
    double bound = 0.0;
    for (int a = 0; a < d; ++a) bound += std::ldexp(1.0, 2 * (QBITS + 1 - q[a]));
    int e = 0;
    (void)std::frexp(bound * (1.0 + std::ldexp(1.0, -20)), &e);
    return 64 - e;
}

int pcm::host_bbox(const void *X, int dtype, int d, long long n, float *part, unsigned *nonfinite, double *out,
                   hipStream_t s, double hb[2 * MAXD]) {
    HIPCHK(hipMemsetAsync(nonfinite, 0, sizeof(unsigned), s));
    const int nblk = (int)std::min<long long>(BBOX_BLOCKS, (n + 255) / 256);
    int rc = dispatch_td(dtype, d, [&](auto T, auto DD) -> int {
        using TT = decltype(T);
        constexpr int D = decltype(DD)::value;
        k_bbox_partial<TT, D><<<nblk, 256, 0, s>>>((const TT *)X, n, part, nonfinite);
        LAUNCHCHK();
        k_bbox_final<D><<<1, 256, 0, s>>>(part, nblk, out);
        LAUNCHCHK();
        return 0;
    });
    if (rc) return rc;
    unsigned nf = 0;
    HIPCHK(hipMemcpyAsync(hb, out, 2 * d * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nf, nonfinite, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nf) return fail(PCM_E_NONFINITE, "input points contain NaN or Inf");
    return 0;
}

extern "C" {

// Debug (not in the public header): make_grid alone, for the tests' restatement of it.  Host
// arithmetic only, no HIP call: it runs on a machine without a GPU.
int pcm_debug_make_grid(int d, const double *lo, const double *hi, double target, int *G, int64_t *ncells,
                        int *prune) {
    if (d < 1 || d > MAXD || !lo || !hi || !G || !ncells || !prune) return fail(PCM_E_ARG, "bad argument");
    Grid g;
    make_grid(g, d, lo, hi, target);
    for (int a = 0; a < MAXD; ++a) G[a] = g.G[a];
    *ncells = g.ncells;
    *prune = g.prune;
    return 0;
}

int pcm_layout_bbox(pcm_engine *e, const void *X, int64_t n, void *stream, double *lo, double *hi, double *maxabs) {
    if (!e || (!X && n > 0) || n < 0 || !lo || !hi || !maxabs) return fail(PCM_E_ARG, "bad argument");
    if (n >= (1LL << 32) - 8) return fail(PCM_E_ARG, "n must be < 2^32 per engine");
    if (int rc = check_device(e)) return rc;
    hipStream_t s = (hipStream_t)stream;
    e->n = n;
    e->n_global = n;
    e->has_rows = false;
    e->have_bbox = false;
    free_layout(e);
    if (n == 0) {
        for (int a = 0; a < e->d; ++a) lo[a] = hi[a] = maxabs[a] = e->lo[a] = e->hi[a] = e->maxabs[a] = 0.0;
        e->have_bbox = true;
        return 0;
    }
    double hb[2 * MAXD];
    if (int rc = host_bbox(X, e->dtype, e->d, n, e->bbox_part, e->nonfinite, e->bbox_out, s, hb)) return rc;
    for (int a = 0; a < e->d; ++a) {
        e->lo[a] = lo[a] = hb[a];
        e->hi[a] = hi[a] = hb[e->d + a];
        e->maxabs[a] = maxabs[a] = std::max(std::fabs(hb[a]), std::fabs(hb[e->d + a]));
    }
    e->have_bbox = true;
    return 0;
}

int pcm_layout_shard(pcm_engine *e, const uint32_t *rows, int64_t n_global, void *stream) {
    if (!e || (!rows && e->n > 0)) return fail(PCM_E_ARG, "bad argument");
    if (!e->have_bbox) return fail(PCM_E_STATE, "pcm_layout_bbox must run first");
    if (n_global < e->n || n_global >= (1LL << 32)) return fail(PCM_E_ARG, "n_global must be in [n, 2^32)");
    if (int rc = check_device(e)) return rc;
    free_layout(e);
    e->n_global = n_global;
    e->has_rows = true;
    if (e->n == 0) return 0;
    HIPCHK(e->grows.ensure((size_t)e->n * sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(e->grows, rows, (size_t)e->n * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return 0;
}

// Crowded-cell detection (tile lists, k_tile_cand): the cell counts of a strided
// sample of up to 2^20 points, scaled to n.  A cell expected to hold more than
// ZCROWD tiles' worth of points gets its points ordered by zlev Morton levels,
// enough that a level-zlev box of the fullest cell holds ~1/8 tile (the lists
// are only needed when K exceeds CAPF).  One host read-back of 4 bytes.
// PCM_ZLEV forces the level count (tests: crowded order on small clouds).
static int choose_zlev(pcm_engine *e, const void *X, hipStream_t s) {
    e->zlev = 0;
    const long long n = e->n, nc = e->g.ncells;
    const int d = e->d;
    const unsigned cb = cell_bits(nc);
    const int zmax = std::min(6, (int)((32 - (int)cb) / d));
    if (const char *v = std::getenv("PCM_ZLEV")) {
        e->zlev = std::max(0, std::min(zmax, std::atoi(v)));
        return 0;
    }
    constexpr double ZCROWD = 4.0;
    if (!e->g.prune || e->k <= CAPF || n < (long long)(ZCROWD * e->tile_cap) || zmax < 1) return 0;
    const long long m = std::min(n, 1LL << 20), stride = n / m;
    HIPCHK(e->zcnt.ensure((size_t)(nc + 1) * sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(e->zcnt, 0, (size_t)(nc + 1) * sizeof(uint32_t), s));
    int rc = dispatch_td(e->dtype, d, [&](auto T, auto DD) -> int {
        using TT = decltype(T);
        constexpr int D = decltype(DD)::value;
        k_zsample<TT, D><<<blocks_for(m), 256, 0, s>>>((const TT *)X, m, stride, e->g, e->zcnt);
        LAUNCHCHK();
        return 0;
    });
    if (rc) return rc;
    k_umax<<<(int)std::min<long long>(1024, std::max(1LL, (nc + 255) / 256)), 256, 0, s>>>(e->zcnt, nc, e->zcnt + nc);
    LAUNCHCHK();
    uint32_t mx = 0;
    HIPCHK(hipMemcpyAsync(&mx, e->zcnt + nc, sizeof(mx), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double est = (double)mx * (double)n / (double)m;
    if (est <= ZCROWD * e->tile_cap) return 0;
    int z = 1;
    while (z < zmax && std::ldexp(1.0, d * z) < 8.0 * est / e->tile_cap) ++z;
    e->zlev = z;
    return 0;
}

// Grow the point-sized persistent buffers for a cloud of up to n points and
// touch them, so that the first layout of a process allocates nothing large.
// The first allocations of a fresh process map and clear new VRAM (~17 ms for
// config 3's ~5 GB); the buffers are the ones pcm_layout_build
// grows: points (xs), labels, perm, the sort's records (ws, sized for the
// worst-case 4-pass plan plus the per-cell arrays of the largest grid), its
// position maps (dmap) and the compressed stream (xz, fp32 D = 3).  Crowded
// layouts' tile-list storage is sized by the tiles and stays lazy.
int pcm_engine_reserve(pcm_engine *e, int64_t n, void *stream) {
    if (!e || n < 0) return fail(PCM_E_ARG, "bad argument");
    if (n >= (1LL << 28) - 32) return fail(PCM_E_ARG, "at most 2^28 - 32 points per engine");
    if (int rc = check_device(e)) return rc;
    // ... and the layout kernels loaded: the runtime loads a unit's code object when one of its
    // kernels is first needed (~9 ms for this unit's), which would land in the first layout too
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_tile_counts)));
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long npad = ((n + 3) / 4) * 4 + 4;
    const size_t ts = tsize(e->dtype);
    size_t scan_bytes = 0;
    if (exscan_u32(nullptr, scan_bytes, nullptr, nullptr, (size_t)1 << 20, s) != hipSuccess)
        return fail(PCM_E_HIP, "reserve: rocprim size query failed");
    RsPlan p;
    if (int rc = rs_plan(e->dtype, e->d, n, 32, p)) return rc;
    const size_t ws_need = align_up(p.total) + align_up(((size_t)1 << 20) * 4) + scan_bytes;
    free_layout(e);   // a grown buffer no longer holds the old layout
    auto grow = [&](DevMem &m, size_t need) -> int {
        if (need == 0) return 0;
        HIPCHK(m.ensure(need));
        HIPCHK(hipMemsetAsync(m.p, 0, m.cap, s));
        return 0;
    };
    if (int rc = grow(e->xs.m, (size_t)e->d * npad * ts)) return rc;
    if (int rc = grow(e->lab.m, (size_t)npad * lsize(e))) return rc;
    if (int rc = grow(e->perm.m, (size_t)n * sizeof(uint32_t))) return rc;
    if (int rc = grow(e->ws.m, ws_need)) return rc;
    if (int rc = grow(e->dmap.m, (size_t)2 * n * sizeof(uint32_t))) return rc;
    return grow(e->xz.m, (e->dtype == PCM_F32 && e->d == 3) ? (size_t)align_up(npad) * 8 : 0);
}

int pcm_layout_build(pcm_engine *e, const void *X, const int32_t *q, int64_t gidx0, void *stream) {
    if (!e || !q) return fail(PCM_E_ARG, "bad argument");
    if (!e->have_bbox) return fail(PCM_E_STATE, "pcm_layout_bbox must run first");
    if (int rc = check_device(e)) return rc;
    hipStream_t s = (hipStream_t)stream;
    free_layout(e);
    for (int a = 0; a < MAXD; ++a) e->qe.q[a] = a < e->d ? q[a] : 0;
    e->iscale = inertia_scale(q, e->d);
    e->gidx0 = gidx0;
    const long long n = e->n;
    e->npad = ((n + 3) / 4) * 4 + 4;
    // the assign kernel addresses points with 32-bit offsets and uses offset
    // 0x0ffffff0 (points) as its always-out-of-range prefetch
    if (e->npad >= 0x0ffffff0LL) return fail(PCM_E_ARG, "at most 2^28 - 32 points per engine (shard larger clouds)");
    choose_grid(e);
    const long long nc = e->g.ncells;
    const size_t ts = tsize(e->dtype);
    // points per tile (<= TILE): PCM_TILE_CAP for tuning sweeps and tests only (read at every layout)
    {
        const char *v = std::getenv("PCM_TILE_CAP");
        const int c = v ? std::atoi(v) : TILE;
        e->tile_cap = (uint32_t)std::min(TILE, std::max(4 * TPB, c));
    }
    // every cell holds ceil(count / cap) <= count / cap + 1 tiles
    e->ntiles_cap = nc + n / e->tile_cap + 1;
    e->ntiles = -1;
    e->rs_bits = e->rs_npass = e->rs_wb = 0;   // no sort yet (an empty cloud has none)
    e->rs_nblk = e->rs_nseg = 0;

    // persistent layout buffers (no allocation when an earlier layout was as large)
    HIPCHK(e->xs.ensure((size_t)e->d * e->npad * ts));
    HIPCHK(e->lab.ensure((size_t)e->npad * lsize(e)));
    HIPCHK(e->perm.ensure((size_t)std::max(1LL, n) * sizeof(uint32_t)));
    HIPCHK(e->cell_start.ensure((size_t)(nc + 1) * sizeof(uint32_t)));
    HIPCHK(e->tile_off.ensure((size_t)(nc + 1) * sizeof(uint32_t)));
    HIPCHK(e->fc_cnt.ensure((size_t)(nc + 1) * sizeof(uint32_t)));
    HIPCHK(e->sub_start.ensure((size_t)((nc << e->d) + 1) * sizeof(uint32_t)));
    HIPCHK(e->fc_rec.ensure((size_t)nc * CAPF * sizeof(float4)));
    HIPCHK(e->fc_lab.ensure((size_t)nc * CAPF * sizeof(int32_t)));
    HIPCHK(e->tiles.ensure((size_t)e->ntiles_cap * sizeof(uint4)));
    HIPCHK(e->tsum.ensure((size_t)std::max(1LL, e->ntiles_cap) * e->d * sizeof(long long)));
    HIPCHK(hipMemsetAsync(e->fc_rec, 0, (size_t)nc * CAPF * sizeof(float4), s));
    HIPCHK(hipMemsetAsync(e->fc_lab, 0, (size_t)nc * CAPF * sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(e->fc_cnt, 0, (size_t)nc * sizeof(uint32_t), s));

    if (n == 0) {
        HIPCHK(hipMemsetAsync(e->tile_off, 0, (size_t)(nc + 1) * sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(e->cell_start, 0, (size_t)(nc + 1) * sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(e->lab, 0xff, (size_t)e->npad * lsize(e), s));
        HIPCHK(hipMemsetAsync(e->xs, 0, (size_t)e->d * e->npad * ts, s));
        HIPCHK(hipMemsetAsync(e->ntiles_dev, 0, sizeof(uint32_t), s));
        e->ntiles = 0;
        e->ntiles_cap = 0;
        e->layout_ready = true;
        return 0;
    }

    // sort key: cell id << d | sub-cell (which half of the cell per axis) on the
    // coarse grids whose k_lloyd1 variant uses sub-cell masks (the 16-slot D <= 3
    // one, see lloyd_slots); else the cell id
    e->sub = (e->d <= 3 && lloyd_slots(e) == LSLOT) ? 1 : 0;
    if (int rc = choose_zlev(e, X, s)) return rc;
    if (e->zlev > 0) e->sub = 0;
    const int sh = e->sub ? e->d : 0;
    const long long nsub = nc << sh;
    // Key order: the LSD record sort of pcm_sort.hpp (no random row gather, no
    // key array).  Measured at config 3: (key, row) pairs sort +
    // 12-B row gather 1.4 + 2.9 ms; rocprim pairs sort with 16-B point records
    // as values 3.4 ms in all; counting sorts slower still (global-atomic
    // counters 3.65 + 7.35 ms, LDS-privatised 0.39 + 7.55 ms: single-point
    // writes into 32768 key ranges do not merge).
    unsigned bits = 1;
    while ((1LL << bits) < nsub) ++bits;
    if (e->zlev > 0) bits = cell_bits(nc) + (unsigned)(e->d * e->zlev);   // <= 32 (choose_zlev)
    size_t scan_bytes = 0;
    if (exscan_u32(nullptr, scan_bytes, nullptr, nullptr, (size_t)nc, s) != hipSuccess)
        return fail(PCM_E_HIP, "layout: rocprim size query failed");
    RsPlan p;
    if (int rc = rs_plan(e->dtype, e->d, n, bits, p)) return rc;
    e->rs_bits = (int)bits;
    e->rs_npass = p.npass;
    e->rs_wb = p.wb;
    e->rs_nblk = p.nblk;
    e->rs_nseg = p.nseg;
    const size_t o_tcnt = align_up(p.total), o_tmp = align_up(o_tcnt + nc * 4), ws_need = o_tmp + scan_bytes;
    if (e->ws.ensure(ws_need) != hipSuccess) return fail(PCM_E_NOMEM, "layout scratch");
    char *wb = (char *)e->ws;
    uint32_t *tcnt = (uint32_t *)(wb + o_tcnt);
    void *tmp = wb + o_tmp;
    // 2-pass sorts keep their position maps for pcm_labels
    e->has_dmap = p.npass == 2 && e->dmap.ensure((size_t)2 * n * sizeof(uint32_t)) == hipSuccess;
    // sorted points, then the starts of the cells (Morton-ordered cells) or of the sub-cells
    int rc = host_sort_cells(X, e->dtype, e->d, n, e->npad, e->g, e->sub, e->zlev, bits, p, wb, e->xs, e->perm,
                             e->has_dmap ? e->dmap.get() : nullptr, e->zlev > 0 ? nc : nsub,
                             e->zlev > 0 ? e->cell_start : e->sub_start, s);
    if (rc) return rc;
    if (e->zlev == 0) {
        k_cell_from_sub<<<blocks_for(nc + 1), 256, 0, s>>>(e->sub_start, nc, sh, e->cell_start);
        LAUNCHCHK();
    }
    k_tile_counts<<<blocks_for(nc), 256, 0, s>>>(e->cell_start, nc, tcnt, e->tile_cap);
    LAUNCHCHK();
    size_t sb = scan_bytes;
    if (exscan_u32(tmp, sb, tcnt, e->tile_off, (size_t)nc, s) != hipSuccess)
        return fail(PCM_E_HIP, "layout: tile scan");
    k_tile_total<<<1, 64, 0, s>>>(e->tile_off, tcnt, nc, e->ntiles_dev);
    LAUNCHCHK();
    k_tile_write<<<blocks_for(nc), 256, 0, s>>>(e->cell_start, e->tile_off, nc, e->tiles, e->tile_cap);
    LAUNCHCHK();
    e->tiles_lpt = false;
    // the exact tile count for the grids of the per-tile kernels (the bound
    // ntiles_cap launched ~1.7x as many blocks at config 3, the excess exiting
    // after one memory latency: a drain tail on every assign launch)
    HIPCHK(hipMemcpyAsync(e->ntiles_host, e->ntiles_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    // compressed point stream for k_lloyd1 (fp32, D = 3; PCM_XZ=0 disables it: A/B measurement only)
    static const bool xz_on = [] { const char *v = std::getenv("PCM_XZ"); return !(v && std::atoi(v) == 0); }();
    e->use_xz = xz_on && e->dtype == PCM_F32 && e->d == 3;
    HIPCHK(hipMemsetAsync(e->zpts, 0, 32 * 16 * sizeof(unsigned long long), s));
    if (e->use_xz) {
        HIPCHK(e->xz.ensure((size_t)align_up(e->npad) * 8));   // whole 256-point blocks (zword)
        HIPCHK(e->tmeta.ensure((size_t)e->ntiles_cap * sizeof(uint4)));
        k_tile_compress<<<(int)std::max(1LL, e->ntiles_cap), 256, 0, s>>>((const float *)e->xs, e->tiles, e->ntiles_dev, e->tmeta,
                                                           e->xz, e->zpts, e->qe, e->tsum);
        LAUNCHCHK();
    } else {   // the tiles' fixed-point sums (k_tile_compress writes them on its way)
        rc = dispatch_td(e->dtype, e->d, [&](auto T, auto DD) -> int {
            using TT = decltype(T);
            constexpr int D = decltype(DD)::value;
            k_tile_sums<TT, D><<<(int)std::max(1LL, e->ntiles_cap), 256, 0, s>>>((const TT *)e->xs, e->tiles, e->ntiles_dev,
                                                                                 e->qe, e->tsum);
            LAUNCHCHK();
            return 0;
        });
        if (rc) return rc;
    }
    if (e->zlev > 0) {   // crowded layout: exact tile boxes and tile-list storage
        HIPCHK(e->tbox.ensure((size_t)e->ntiles_cap * 2 * sizeof(float4)));
        HIPCHK(e->tl_cnt.ensure((size_t)e->ntiles_cap * sizeof(uint32_t)));
        HIPCHK(e->tl_rec.ensure((size_t)e->ntiles_cap * TLMAX * sizeof(float4)));
        HIPCHK(e->tl_lab.ensure((size_t)e->ntiles_cap * TLMAX * sizeof(int32_t)));
        rc = dispatch_td(e->dtype, e->d, [&](auto T, auto DD) -> int {
            using TT = decltype(T);
            constexpr int D = decltype(DD)::value;
            k_tile_box<TT, D><<<(int)e->ntiles_cap, 256, 0, s>>>((const TT *)e->xs, e->tiles, e->ntiles_dev, e->tbox);
            LAUNCHCHK();
            return 0;
        });
        if (rc) return rc;
    }
    // one host synchronisation at the end (the tile count; and choose_zlev's
    // occupancy read-back): X must not be modified by other streams meanwhile
    HIPCHK(hipStreamSynchronize(s));
    e->ntiles = (long long)*e->ntiles_host;
    if (e->ntiles > e->ntiles_cap) return fail(PCM_E_HIP, "layout: tile count exceeds its bound");
    e->layout_ready = true;
    return 0;
}

}  // extern "C"

// Longest-list-first tile order: the tile records (and their compression
// records) sorted by descending candidate-list length of their cell at the
// first lists, so k_lloyd1 dispatches its longest-lived blocks first and the
// short ones fill the tail (a block's lifetime follows its list length,
// DESIGN.md §4).  Where the tiles are few generations of resident blocks (the
// 8-way slab: 4096 tiles, 37.1 vs 39.1 us per assign) or D = 4 (config-5 shard,
// 299 vs 307 us) it pays; config 3's 32768 D = 3 tiles keep their spatial order
// and the XCD ranges (profiles/rd6_tile_lpt_ab.txt).  The statistics are exact
// integers, so the order changes no result.  PCM_TILE_LPT = 0 / 1 forces it.
int pcm::tiles_order_lpt(pcm_engine *e, hipStream_t s) {
    const char *lv = std::getenv("PCM_TILE_LPT");   // read at every fit start (A/B runs, tests)
    const int mode = lv ? std::atoi(lv) : -1;
    const bool want = mode == 1 || (mode < 0 && (e->d >= 4 || e->ntiles <= 16LL * e->num_cu));
    if (!want || e->zlev > 0 || e->ntiles < 2) return 0;   // crowded layouts: tile boxes and lists are per tile
    const unsigned nt = (unsigned)e->ntiles;
    size_t sort_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                  (uint32_t *)nullptr, (size_t)nt, 0u, 16u, s) != hipSuccess)
        return fail(PCM_E_HIP, "tile order: sort size");
    const size_t o_k1 = align_up((size_t)nt * 4), o_v0 = o_k1 + align_up((size_t)nt * 4), o_v1 = o_v0 + align_up((size_t)nt * 4),
                 o_t2 = o_v1 + align_up((size_t)nt * 4), o_m2 = o_t2 + align_up((size_t)nt * 16),
                 o_s2 = o_m2 + align_up((size_t)nt * 16), o_o2 = o_s2 + align_up((size_t)nt * e->d * 8),
                 o_tmp = o_o2 + align_up((size_t)nt * 4), need = o_tmp + sort_bytes;
    if (e->ws.ensure(need) != hipSuccess) return fail(PCM_E_NOMEM, "tile order scratch");
    HIPCHK(e->tpos.ensure((size_t)nt * sizeof(uint32_t)));
    HIPCHK(e->torig.ensure((size_t)nt * sizeof(uint32_t)));
    char *wb = (char *)e->ws;
    uint32_t *k0 = (uint32_t *)wb, *k1 = (uint32_t *)(wb + o_k1), *v0 = (uint32_t *)(wb + o_v0), *v1 = (uint32_t *)(wb + o_v1);
    uint4 *t2 = (uint4 *)(wb + o_t2), *m2 = (uint4 *)(wb + o_m2);
    long long *s2 = (long long *)(wb + o_s2);
    uint32_t *o2 = (uint32_t *)(wb + o_o2);
    k_tile_lpt_keys<<<blocks_for(nt), 256, 0, s>>>(e->tiles, e->fc_cnt, nt, k0, v0);
    LAUNCHCHK();
    size_t sb = sort_bytes;
    if (rocprim::radix_sort_pairs((void *)(wb + o_tmp), sb, k0, k1, v0, v1, (size_t)nt, 0u, 16u, s) != hipSuccess)
        return fail(PCM_E_HIP, "tile order: sort");
    // (a layout's first reorder starts from the layout order: torig = identity)
    k_tile_gather<<<blocks_for(nt), 256, 0, s>>>(e->tiles, e->use_xz ? e->tmeta : nullptr, v1, nt, t2, m2, e->tsum, s2, e->d,
                                                 e->tiles_lpt ? e->torig : nullptr, o2, e->tpos);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(e->tiles, t2, (size_t)nt * sizeof(uint4), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(e->tsum, s2, (size_t)nt * e->d * sizeof(long long), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(e->torig, o2, (size_t)nt * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (e->use_xz) HIPCHK(hipMemcpyAsync(e->tmeta, m2, (size_t)nt * sizeof(uint4), hipMemcpyDeviceToDevice, s));
    e->tiles_lpt = true;
    return 0;
}
