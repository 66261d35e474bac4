// pcm_predict.hip — predict (sklearn KMeans.predict / _labels_inertia, sklearn/cluster/_kmeans.py:
// 1083-1108, on given centres): bounding box of X -> pruning grid -> exact
// candidate lists of the centres (the fit's builders at drift budget 0) ->
// k_predict.  All device memory comes from the caller's workspace.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <new>

#include "pcm_cand.hpp"   // cand_capc, SoleW
#include "pcm_util.hpp"   // k_predict_pack, k_predict, k_cand_stats; k_inert_fold (pcm_assign.hpp)
#include "pcm_host.hpp"

using namespace pcm;

namespace {
struct PredWs {   // byte offsets into the workspace
    size_t bbox_part, bbox_out, nonfinite, c4, cref, ctrl, cand_stats, inert, rep, fc_cnt, fc_rec, fc_lab, cl_cnt, cl_idx,
        total;
    long long nc_max, ncoarse_max;
};

// Grid rule: the fit's per-centre policy (32 K cells, D = 4: 48 K), at most one
// cell per 8 points (building a cell's list costs about as much as scanning a
// few tens of points) and make_grid's 2^18 cap.
double pred_target(long long n, int d, int k) {
    const double per_centre = d >= 4 ? 48.0 : 32.0;
    return std::max(1.0, std::min({per_centre * (double)k, (double)n / 8.0, (double)(1 << 18)}));
}

void pred_layout(long long n, int d, int k, PredWs &w) {
    const double target = pred_target(n, d, k);
    // make_grid rounds every axis to a whole number of cells; pcm_predict shrinks
    // the target until the grid fits these bounds (the cell count affects speed only)
    w.nc_max = (long long)std::ceil(1.5 * target) + 16;
    w.ncoarse_max = d >= 4 ? w.nc_max / 64 + 16 : 0;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + std::max<size_t>(bytes, 8)); return at; };
    w.bbox_part = take((size_t)BBOX_BLOCKS * 2 * MAXD * sizeof(float));
    w.bbox_out = take(2 * MAXD * sizeof(double));
    w.nonfinite = take(sizeof(unsigned));
    w.c4 = take((size_t)k * sizeof(float4));
    w.cref = take((size_t)k * sizeof(float4));
    w.ctrl = take(sizeof(Ctrl));
    w.cand_stats = take(3 * sizeof(unsigned long long));
    w.inert = take(4 * sizeof(unsigned long long));
    w.rep = take((size_t)INERT_REP * 16 * sizeof(unsigned long long));
    w.fc_cnt = take((size_t)w.nc_max * sizeof(uint32_t));
    w.fc_rec = take((size_t)w.nc_max * CAPF * sizeof(float4));
    w.fc_lab = take((size_t)w.nc_max * CAPF * sizeof(int32_t));
    w.cl_cnt = take((size_t)w.ncoarse_max * sizeof(uint32_t));
    w.cl_idx = take((size_t)w.ncoarse_max * cand_capc<4>() * sizeof(int32_t));
    w.total = o;
}

// make_grid over the box, then the cell counts clamped to the workspace bounds
// (clamp_grid, pcm_layout.hip: thin boxes; 1 cell and 1 coarse cell are inside
// every bound pred_layout gives).  The coarse tables exist at D = 4 only.
void pred_grid(Grid &g, int d, const double *lo, const double *hi, double target, const PredWs &w) {
    make_grid(g, d, lo, hi, target);
    clamp_grid(g, w.nc_max, d >= 4 ? w.ncoarse_max : std::numeric_limits<long long>::max());
}

int pred_args(int64_t n, int d, int k) {
    if (d < 1 || d > MAXD) return fail(PCM_E_ARG, "d must be 1..4");
    if (k < 1 || k > (1 << 24)) return fail(PCM_E_ARG, "k must be in [1, 2^24]");
    if (n < 0) return fail(PCM_E_ARG, "n must be >= 0");
    return 0;
}
}  // namespace

extern "C" {

int pcm_predict_workspace(int64_t n, int d, int k, size_t *bytes) {
    if (!bytes) return fail(PCM_E_ARG, "bytes is null");
    if (int rc = pred_args(n, d, k)) return rc;
    PredWs w;
    pred_layout(n, d, k, w);
    *bytes = w.total;
    return 0;
}

int pcm_predict(const void *X, int dtype, int64_t n, int d, const float *C, int k, const int32_t *q, int32_t *labels,
                float *dist, pcm_inertia *limbs, int64_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = pred_args(n, d, k)) return rc;
    if (dtype != PCM_F32 && dtype != PCM_F16) return fail(PCM_E_ARG, "dtype must be PCM_F32 or PCM_F16");
    if ((!X || !labels) && n > 0) return fail(PCM_E_ARG, "X or labels is null");
    if (!C) return fail(PCM_E_ARG, "C is null");
    if (limbs && !q) return fail(PCM_E_ARG, "inertia limbs need the fixed-point exponents q");
    if (info) info[0] = info[1] = info[2] = 0;
    if (limbs) {
        std::memset(limbs, 0, sizeof(*limbs));
        limbs->scale = inertia_scale(q, d);
    }
    if (n == 0) return 0;   // nothing to label: no device call
    hipStream_t s = (hipStream_t)stream;
    // centres: finite (checked on the host), and how far they reach (k is bounded; nothing throws)
    const size_t nce = (size_t)k * d;
    std::unique_ptr<float[]> hc(new (std::nothrow) float[nce]);
    if (!hc) return fail(PCM_E_NOMEM, "predict: host copy of the centres");
    HIPCHK(hipMemcpyAsync(hc.get(), C, nce * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double cabs = 0.0;
    for (size_t i = 0; i < nce; ++i) {
        if (!std::isfinite(hc[i])) return fail(PCM_E_ARG, "centres contain NaN or Inf");
        cabs = std::max(cabs, (double)std::fabs(hc[i]));
    }
    PredWs w;
    pred_layout(n, d, k, w);
    if (!workspace || workspace_bytes < w.total) return fail(PCM_E_ARG, "workspace too small (pcm_predict_workspace)");
    char *wb = (char *)workspace;
    float *bbox_part = (float *)(wb + w.bbox_part);
    double *bbox_out = (double *)(wb + w.bbox_out);
    unsigned *nonfinite = (unsigned *)(wb + w.nonfinite);
    float4 *c4 = (float4 *)(wb + w.c4), *cref = (float4 *)(wb + w.cref), *fc_rec = (float4 *)(wb + w.fc_rec);
    Ctrl *ctrl = (Ctrl *)(wb + w.ctrl);
    unsigned long long *cand_stats = (unsigned long long *)(wb + w.cand_stats), *inert = (unsigned long long *)(wb + w.inert),
                       *rep = (unsigned long long *)(wb + w.rep);
    uint32_t *fc_cnt = (uint32_t *)(wb + w.fc_cnt), *cl_cnt = (uint32_t *)(wb + w.cl_cnt);
    int32_t *fc_lab = (int32_t *)(wb + w.fc_lab), *cl_idx = (int32_t *)(wb + w.cl_idx);
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
        ncu = 256;
    // bounding box of X (+ non-finite check): the one host synchronisation on the data
    double hb[2 * MAXD];
    if (int rc = host_bbox(X, dtype, d, n, bbox_part, nonfinite, bbox_out, s, hb)) return rc;
    // The grid covers the box of X alone: the list builders' test (prunable) is
    // geometric over a cell's box and holds for centres anywhere, inside or
    // outside the grid; only the points must lie in their cells' boxes.
    Grid g;
    pred_grid(g, d, hb, hb + d, pred_target(n, d, k), w);
    if (g.ncells > w.nc_max || (d >= 4 && g.ncoarse > w.ncoarse_max))
        return fail(PCM_E_STATE, "predict: grid exceeds the workspace bound");
    double xabs = 0.0;
    for (int a = 0; a < d; ++a) xabs = std::max({xabs, std::fabs(hb[a]), std::fabs(hb[d + a])});
    // no pruning for one centre, and none where an fp32 distance can overflow (make_grid checks
    // the extent of X; centres may lie far outside it)
    if (k <= 1 || xabs + cabs >= 1e18) g.prune = 0;
    k_predict_pack<<<blocks_for(k), 256, 0, s>>>(C, k, d, c4);
    LAUNCHCHK();
    if (limbs) {
        HIPCHK(hipMemsetAsync(inert, 0, 4 * sizeof(unsigned long long), s));
        HIPCHK(hipMemsetAsync(rep, 0, (size_t)INERT_REP * 16 * sizeof(unsigned long long), s));
    }
    if (g.prune) {
        // k_cand also records the centres its lists were built at and clears the drift
        // budget: a private control block and reference buffer take those stores
        HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(Ctrl), s));
        const long long bpc = std::max(1LL, std::min(8LL, (2LL * ncu + g.ncoarse - 1) / g.ncoarse));
        if (int rc = host_candidates(d, g, c4, k, ctrl, 0, d >= 4, (int)bpc, fc_cnt, fc_rec, fc_lab, cref, cl_cnt,
                                     cl_idx, SoleW{}, s))
            return rc;
    }
    int rc = dispatch_td(dtype, d, [&](auto TT, auto DD) -> int {
        using T = decltype(TT);
        constexpr int D = decltype(DD)::value;
        const int pg = (int)std::min<long long>((n + TPB - 1) / TPB, (long long)ncu * 32);
        k_predict<T, D><<<pg, TPB, 0, s>>>((const T *)X, n, g, c4, k, fc_cnt, fc_rec, fc_lab, labels, dist,
                                           limbs ? rep : nullptr, limbs ? limbs->scale : 0);
        LAUNCHCHK();
        return 0;
    });
    if (rc) return rc;
    unsigned long long hi[4] = {0, 0, 0, 0}, hs[3] = {0, 0, 0};
    if (limbs) {
        k_inert_fold<<<1, 64, 0, s>>>(rep, inert);
        LAUNCHCHK();
        HIPCHK(hipMemcpyAsync(hi, inert, sizeof(hi), hipMemcpyDeviceToHost, s));
    }
    if (info && g.prune) {
        HIPCHK(hipMemsetAsync(cand_stats, 0, 3 * sizeof(unsigned long long), s));
        k_cand_stats<<<blocks_for(g.ncells), 256, 0, s>>>(fc_cnt, g.ncells, cand_stats);
        LAUNCHCHK();
        HIPCHK(hipMemcpyAsync(hs, cand_stats, sizeof(hs), hipMemcpyDeviceToHost, s));
    }
    if (limbs || (info && g.prune)) HIPCHK(hipStreamSynchronize(s));
    if (limbs) {
        for (int t = 0; t < 3; ++t) limbs->limbs[t] = hi[t];
        limbs->overflow = (uint32_t)std::min<unsigned long long>(hi[3], 0xFFFFFFFFull);
    }
    if (info && g.prune) {
        info[0] = (int64_t)g.ncells;
        info[1] = (int64_t)hs[2];
        info[2] = (int64_t)hs[0];
    }
    return 0;
}

}  // extern "C"
