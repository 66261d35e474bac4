// pcm_kpp.hip — k-means++ seeding (oracle/kpp_ref.py; sklearn/cluster/_kmeans.py:174-272):
// cell layout of X (pcm_layout.hip's bounding box, grid and sort), then 3 launches per centre
// (csrc/pcm_kpp.hpp).  All device memory comes from the caller's workspace (pcm_kmeanspp_workspace).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#include "pcm_kpp.hpp"
#include "pcm_host.hpp"

using namespace pcm;

namespace {
struct KppWs {   // byte offsets into the workspace
    size_t bbox_part, bbox_out, nonfinite, sort, perm, crow, xs, closest, cell_start, cmax, bsum, ctl, um, total;
    long long nc_max;
    RsPlan plan;   // the cell sort's plan at the largest grid (kpp_cells_max)
};

long long kpp_cells_max(long long n, int d) {
    const double target = std::max(1.0, (double)n / KPP_CELL_PTS);
    return std::min<long long>(1LL << 20, (long long)std::ceil(std::pow(1.5, d) * target) + 2);
}

int kpp_layout(long long n, int d, int k, int L, KppWs &w) {
    const long long npad = ((n + 3) / 4) * 4 + 4;
    const long long nb = (n + KPP_OB - 1) / KPP_OB;
    w.nc_max = kpp_cells_max(n, d);
    if (int rc = rs_plan(PCM_F32, d, n, cell_bits(w.nc_max), w.plan)) return rc;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + std::max<size_t>(bytes, 8)); return at; };
    w.bbox_part = take((size_t)BBOX_BLOCKS * 2 * MAXD * sizeof(float));
    w.bbox_out = take(2 * MAXD * sizeof(double));
    w.nonfinite = take(sizeof(unsigned));
    w.sort = take(w.plan.total);
    w.perm = take(n * 4);
    w.crow = take(n * 4);
    w.xs = take((size_t)npad * d * sizeof(float));
    w.closest = take(n * 4);
    w.cell_start = take((w.nc_max + 1) * 4);
    w.cmax = take(w.nc_max * 4);
    w.bsum = take(nb * 8);
    w.ctl = take(sizeof(KppCtl));
    w.um = take((size_t)std::max(1, (k - 1) * L) * 8);
    w.total = o;
    return 0;
}

// oracle/kpp_ref.py kpp_scale: n * 2^s * maxd * (1 + 2^-20) < 2^62
int kpp_scale(long long n, double maxd) {
    if (!(maxd > 0.0) || n <= 0) return 0;
    int e = 0;
    (void)std::frexp(maxd * (1.0 + std::ldexp(1.0, -20)), &e);
    int nb = 0;
    for (unsigned long long v = (unsigned long long)(n - 1); v; v >>= 1) ++nb;
    return 62 - std::max(1, nb) - e;
}
}  // namespace

extern "C" {

int pcm_kmeanspp_workspace(int64_t n, int d, int k, int n_local_trials, size_t *bytes) {
    if (!bytes || n < 1 || d < 1 || d > MAXD || k < 1 || n_local_trials < 1) return fail(PCM_E_ARG, "bad argument");
    KppWs w;
    if (int rc = kpp_layout(n, d, k, n_local_trials, w)) return rc;
    *bytes = w.total;
    return 0;
}

int pcm_kmeanspp(const float *X, int64_t n, int d, int k, int n_local_trials, int64_t first_index,
                 const uint64_t *umant, int64_t *indices, void *workspace, size_t workspace_bytes, void *stream) {
    if (!X || !indices || n < 1 || k < 1 || k > n || d < 1 || d > MAXD) return fail(PCM_E_ARG, "bad argument");
    if (n_local_trials < 1 || n_local_trials > KPP_LMAX) return fail(PCM_E_ARG, "n_local_trials must be 1..16");
    if (first_index < 0 || first_index >= n) return fail(PCM_E_ARG, "first_index out of range");
    if (k > 1 && !umant) return fail(PCM_E_ARG, "umant is null");
    if (n >= (1LL << 32) - 8) return fail(PCM_E_ARG, "n must be < 2^32");
    const int L = n_local_trials;
    KppWs w;
    if (int rc = kpp_layout(n, d, k, L, w)) return rc;
    if (!workspace || workspace_bytes < w.total) return fail(PCM_E_ARG, "workspace too small (pcm_kmeanspp_workspace)");
    hipStream_t s = (hipStream_t)stream;
    char *wb = (char *)workspace;
    float *bbox_part = (float *)(wb + w.bbox_part), *xs = (float *)(wb + w.xs), *closest = (float *)(wb + w.closest),
          *cmax = (float *)(wb + w.cmax);
    double *bbox_out = (double *)(wb + w.bbox_out);
    unsigned *nonfinite = (unsigned *)(wb + w.nonfinite);
    uint32_t *perm = (uint32_t *)(wb + w.perm), *cell_start = (uint32_t *)(wb + w.cell_start);
    float *crow = (float *)(wb + w.crow);
    unsigned long long *bsum = (unsigned long long *)(wb + w.bsum), *um = (unsigned long long *)(wb + w.um);
    KppCtl *ctl = (KppCtl *)(wb + w.ctl);
    const long long npad = ((n + 3) / 4) * 4 + 4;
    const long long nb = (n + KPP_OB - 1) / KPP_OB;
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
        ncu = 256;
    // bounding box (+ non-finite check) -> pruning grid of ~n / KPP_CELL_PTS cells, weight scale
    double hb[2 * MAXD];
    if (int rc = host_bbox(X, PCM_F32, d, n, bbox_part, nonfinite, bbox_out, s, hb)) return rc;
    double maxd = 0.0;
    for (int a = 0; a < d; ++a) maxd += (hb[d + a] - hb[a]) * (hb[d + a] - hb[a]);
    const int scale = kpp_scale(n, maxd);
    Grid g;
    make_grid(g, d, hb, hb + d, std::max(1.0, (double)n / KPP_CELL_PTS));
    // a thin box (a few pixels of relief over a whole image) gets far more cells than kpp_cells_max
    // along its long axes: clamp_grid halves them until the cell arrays fit; a grid that fits stays
    clamp_grid(g, w.nc_max, std::numeric_limits<long long>::max());
    const long long nc = g.ncells;
    if (nc > w.nc_max) return fail(PCM_E_STATE, "kmeanspp: grid exceeds the workspace bound");
    unsigned bits = 1;
    while ((1LL << bits) < nc) ++bits;
    if (k > 1) HIPCHK(hipMemcpy(um, umant, (size_t)(k - 1) * L * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(bsum, 0, nb * 8, s));
    HIPCHK(hipMemsetAsync(ctl, 0, sizeof(KppCtl), s));
    // cell layout (the Lloyd engine's record sort, pcm_sort.hpp), cell starts
    RsPlan p;
    if (int rc = rs_plan(PCM_F32, d, n, bits, p)) return rc;
    if (p.total > w.plan.total) return fail(PCM_E_STATE, "kmeanspp: sort plan exceeds the workspace bound");
    if (int rc = host_sort_cells(X, PCM_F32, d, n, npad, g, 0, 0, bits, p, wb + w.sort, xs, perm, nullptr, nc,
                                 cell_start, s))
        return rc;
    return dispatch_d(d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        const int pgrid = ncu * 8;
        k_kpp_init<D><<<pgrid, 256, 0, s>>>(xs, cell_start, nc, X, first_index, closest, cmax, (long long *)indices);
        LAUNCHCHK();
        k_kpp_init_rows<D><<<(int)std::min<long long>(nb, pgrid), 256, 0, s>>>(X, n, first_index, scale, crow, bsum, ctl);
        LAUNCHCHK();
        // from centre 64 on a step touches a neighbourhood: a quarter of the grid
        // (2048 -> 512 blocks) for eval/apply, 163.3 -> 159.1 ms at config 3
        // (tools/kpp_grid_sweep.sh; 1/8: 162.6 ms); re-swept after the round-3
        // atomics fix: 1/4 109.3-110.2, 1/2 113.3, 1/8 123.4 ms (tools/r4j.sh).
        // PCM_KPP_LATE_*: tuning only
        // round 5 (eval at 86 VGPRs, 5 waves/SIMD): eval keeps the whole grid, apply
        // 1/4 -- 94.5 ms vs 95.1 (1/2, 1/4), 94.9 (1/2, 1/2), 95.9 (1/1, 1/8)
        // (tools/rd5q.sh, profiles/rd5_kpp_steps.txt)
        static const int late_div = [] { const char *v = std::getenv("PCM_KPP_LATE_DIV"); return v ? std::max(1, std::atoi(v)) : 1; }();
        static const int apply_div = [] { const char *v = std::getenv("PCM_KPP_APPLY_DIV"); return v ? std::max(1, std::atoi(v)) : 4; }();
        static const int late_c = [] { const char *v = std::getenv("PCM_KPP_LATE_C"); return v ? std::atoi(v) : 64; }();
        for (int c = 1; c < k; ++c) {
            const int eg = c >= late_c ? std::max(ncu, pgrid / late_div) : pgrid;
            const int ag = c >= late_c ? std::max(ncu, pgrid / apply_div) : pgrid;
            k_kpp_search<D><<<L + KPP_RED_BLOCKS, KPP_STPB, 0, s>>>(bsum, nb, crow, X, n,
                                                                    um + (size_t)(c - 1) * L, L, scale, c, cmax, nc,
                                                                    ctl);
            LAUNCHCHK();
            if (L <= 8) k_kpp_eval<D, 8><<<eg, 256, 0, s>>>(xs, cell_start, g, closest, cmax, L, scale, c, ctl);
            else k_kpp_eval<D><<<eg, 256, 0, s>>>(xs, cell_start, g, closest, cmax, L, scale, c, ctl);
            LAUNCHCHK();
            k_kpp_apply<D><<<ag, 256, 0, s>>>(xs, perm, cell_start, g, closest, crow, cmax, bsum, X, n, L, scale, c,
                                              c + 1 < k ? 1 : 0, (long long *)indices, ctl);
            LAUNCHCHK();
        }
        return 0;
    });
}

#ifdef PCM_DBG_TIMING
// This unit's copies of the stamp arrays (pcm_debug.hpp), written by the k_kpp_* kernels.
int pcm_debug_timing_kpp(unsigned long long *out, int nblocks) {
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_t), (size_t)nblocks * 16 * sizeof(unsigned long long)));
    return 0;
}
int pcm_debug_timing_eval(unsigned long long *out, int nblocks) {
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_e), (size_t)nblocks * 8 * sizeof(unsigned long long)));
    return 0;
}
int pcm_debug_kpp_counts(unsigned long long *out, int ncentres) {
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_kpp), (size_t)ncentres * 4 * sizeof(unsigned long long)));
    return 0;
}
#endif

}  // extern "C"
