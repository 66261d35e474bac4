// pcm_align.hip — co-registration statistics of labelled days against fixed centres (DESIGN.md §4,
// "Registration: k_align").
//
// pcm_align_prepare builds, once per registration, the exact candidate lists of the centres over
// a pruning grid laid over the box of the CENTRES (the fit's builders at drift budget 0, as
// pcm_predict).  pcm_align_stats is then one launch per iteration: every row is transformed by its
// group's rigid motion in float32, finds its canonical nearest centre, and adds the fixed-point
// sums a Kabsch solve needs to its group's PCM_ALIGN_WORDS words:
//
//   word 0, 1        inliers (d2 <= max_d2), outliers (valid rows, trimmed)
//   words 2..4       sum pq_a          pq_a = trunc(ldexp(p_a, q_a)), cq_a = trunc(ldexp(c_ja, q_a))
//   words 5..7       sum cq_a
//   words 8..25      sum pq_a cq_b     nine pairs, row-major, lo = p & 0xffffffff, hi = p >> 32
//   words 26..31     sum pq_a^2        lo / hi
//   words 32..37     sum cq_a^2        lo / hi
//
// All adds are integer adds: the words do not depend on the order of the rows, on the grid or on
// how the rows are split over calls, chunks and ranks.
//
// Paths of a row (none changes a bit of the result):
//   * inside the grid's box on every axis (tested before any clamping): the row bins with the
//     layout's arithmetic and scans its cell's exact list (a FULL cell scans all K);
//   * outside on some axis: all K centres -- the lists are exact only for points inside their
//     cell's box;
//   * provable outlier (finite max_d2 only): on some axis fl(clo_a - p_a) >= r or
//     fl(p_a - chi_a) >= r, [clo, chi] the box of the centres and r the smallest float with
//     fl(r * r) > max_d2.  Rounding is monotone, so for every centre c the first difference of
//     dist_canon is at least r in magnitude, its square at least fl(r * r), and the rounded adds of
//     non-negative squares never go below that: d2 > max_d2 without a scan.
//
// Accumulation: k_cluster_stats' scheme with key = group.  A wave takes a contiguous run of rounds
// (64 rows each) and carries per-lane sums of ONE group across them; when the carried group is
// absent from a round they are summed over the wave (reduce_scatter) and flushed with one
// no-return atomic wave-instruction per 32 words.  Lanes of another group than the carried one
// (the round at a day boundary, a randomly ordered cloud) add their words with per-lane atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>

#include "pcm_cand.hpp"   // SoleW
#include "pcm_util.hpp"   // k_predict_pack, k_cand_stats
#include "pcm_host.hpp"
#include "pcm_reduce.hpp"

using namespace pcm;
using pcm_stats::reduce_scatter;
using pcm_stats::u64;

namespace {

constexpr int A_TPB = 256;
constexpr int A_WAVES = A_TPB / 64;
constexpr int A_MIN_ROUNDS = 16;   // rounds per wave before the grid shrinks (a flush costs about one round)
constexpr int W = PCM_ALIGN_WORDS;

struct AlignWs {   // byte offsets into the workspace
    size_t c4, cref, ctrl, cand_stats, fc_cnt, fc_rec, fc_lab, total;
    long long nc_max;
};

// The host side of a prepared workspace (the bytes of pcm_align_plan).
struct AlignPlan {
    uint32_t magic;
    int k;
    Grid g;
    AlignWs w;
    float clo[3], chi[3];   // box of the centres
    double cabs[3];         // max |c_a|
    int ncu;
};
static_assert(sizeof(AlignPlan) <= sizeof(pcm_align_plan), "pcm_align_plan is too small");
constexpr uint32_t PLAN_MAGIC = 0x414c4731u;

// predict's grid rule: 32 cells per centre, one cell per 8 rows, 2^18 at most
double align_target(long long n, int k) {
    return std::max(1.0, std::min({32.0 * (double)k, (double)std::max<long long>(n, 8) / 8.0, (double)(1 << 18)}));
}

void align_layout(long long n, int k, AlignWs &w) {
    w.nc_max = (long long)std::ceil(1.5 * align_target(n, k)) + 16;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + std::max<size_t>(bytes, 8)); return at; };
    w.c4 = take((size_t)k * sizeof(float4));
    w.cref = take((size_t)k * sizeof(float4));
    w.ctrl = take(sizeof(Ctrl));
    w.cand_stats = take(3 * sizeof(unsigned long long));
    w.fc_cnt = take((size_t)w.nc_max * sizeof(uint32_t));
    w.fc_rec = take((size_t)w.nc_max * CAPF * sizeof(float4));
    w.fc_lab = take((size_t)w.nc_max * CAPF * sizeof(int32_t));
    w.total = o;
}

int align_args(int64_t n, int k) {
    if (k < 1 || k > (1 << 24)) return fail(PCM_E_ARG, "k must be in [1, 2^24]");
    if (n < 0) return fail(PCM_E_ARG, "n must be >= 0");
    return 0;
}

struct AlignQ {
    int q[3];
};
struct AlignGrid {   // what the binning reads of the plan's Grid
    double lo[3], inv[3];
    int G[3];
    int prune;
};
struct AlignBox {
    float clo[3], chi[3];
    float r;   // smallest float with fl(r * r) > max_d2; unused when skip == 0
    int skip;
};

// p_a = ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a, every operation rounded (-ffp-contract=off)
__device__ __forceinline__ void rigid(const float *__restrict__ T, int g, const float (&x)[3], float (&p)[3]) {
    const float *t = T + (size_t)g * 12;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float m0 = t[3 * a] * x[0], m1 = t[3 * a + 1] * x[1], m2 = t[3 * a + 2] * x[2];
        const float s01 = m0 + m1;
        const float s = s01 + m2;
        p[a] = s + t[9 + a];
    }
}

template <bool GROUPS, bool XFORM>
__global__ __launch_bounds__(A_TPB) void k_align(const float *__restrict__ X, long long n,
                                                 const uint8_t *__restrict__ groups, int n_groups,
                                                 const float *__restrict__ T, float max_d2, AlignQ qe, AlignBox bx,
                                                 AlignGrid g, const float4 *__restrict__ C, int K,
                                                 const uint32_t *__restrict__ fc_cnt,
                                                 const float4 *__restrict__ fc_rec,
                                                 const int32_t *__restrict__ fc_lab, u64 *__restrict__ out,
                                                 long long rounds, long long rpw) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * A_WAVES + (threadIdx.x >> 6);
    const long long r0 = wave * rpw, r1 = r0 + rpw < rounds ? r0 + rpw : rounds;
    if (r0 >= r1) return;
    int ckey = -1;   // the carried group (wave-uniform), -1: none
    u64 acc[W];      // this lane's share of the carried group's words
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0;
    unsigned skipped = 0;   // wave-uniform
    auto flush = [&]() {
        if (ckey < 0) return;
        u64 *row = out + (long long)ckey * W;
        {   // words 0..31: lane l ends with word l >> 1
            u64 v[32];
#pragma unroll
            for (int w = 0; w < 32; ++w) v[w] = acc[w];
            const u64 tot = reduce_scatter<32>(v, lane);
            if ((lane & 1) == 0) atomicAdd(row + (lane >> 1), tot);
        }
        {   // words 32..37 (padded to 8): lane l ends with word 32 + (l >> 3)
            u64 v[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) v[w] = 32 + w < W ? acc[32 + w < W ? 32 + w : 0] : 0ull;
            const u64 tot = reduce_scatter<8>(v, lane);
            if ((lane & 7) == 0 && 32 + (lane >> 3) < W) atomicAdd(row + 32 + (lane >> 3), tot);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = 0;
    };
    // the loads of round r + 1 are issued before round r is worked (k_cluster_stats): the row index
    // is clamped to n - 1 and what a lane past the end loads is never used
    float nx[3];
    int ng = 0;
    auto fetch = [&](long long r) {
        long long i = r * 64 + lane;
        i = i < n ? i : n - 1;
        if (GROUPS) ng = (int)groups[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) nx[a] = X[i * 3 + a];
    };
    fetch(r0);
    for (long long r = r0; r < r1; ++r) {
        const long long i = r * 64 + lane;
        const int grp = ng;
        float x[3], p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] = nx[a];
        fetch(r + 1);
        // ---- the row's point and whether it counts at all
        bool valid = i < n && grp < n_groups && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
        if (valid) {
            if (XFORM) rigid(T, grp, x, p);
            else {
#pragma unroll
                for (int a = 0; a < 3; ++a) p[a] = x[a];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
                valid = valid && isfinite(p[a]) && fabsf(__builtin_ldexpf(p[a], qe.q[a])) < (float)(1 << QBITS);
        }
        skipped += (unsigned)__popcll(__ballot(i < n && !valid));
        // ---- which lanes add to the carried registers: those of the carried group, or, when it is
        // absent from the round, of the first valid lane's group (after a flush)
        const u64 vm = __ballot(valid);
        if (!vm) continue;
        u64 m = ckey >= 0 ? __ballot(valid && grp == ckey) : 0ull;
        if (!m) {
            flush();
            ckey = __builtin_amdgcn_readfirstlane(__shfl(grp, __ffsll((long long)vm) - 1));
            m = __ballot(valid && grp == ckey);
        }
        if (!valid) continue;
        const bool carried = (m >> lane) & 1ull;
        u64 *row = out + (long long)grp * W;
        // ---- provable outliers need no scan
        bool far = false;
        if (bx.skip) {
#pragma unroll
            for (int a = 0; a < 3; ++a) far = far || (bx.clo[a] - p[a] >= bx.r) || (p[a] - bx.chi[a] >= bx.r);
        }
        float bd = 0.f;
        int bj = 0;
        if (!far) {
            uint32_t mlist = FULL;
            long long cell = 0;
            if (g.prune) {
                // inside the box iff the unclamped index is a cell on every axis (tested in fp64, before any cast)
                bool in = true;
                int idx[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double v = floor(((double)p[a] - g.lo[a]) * g.inv[a]);
                    in = in && v >= 0.0 && v < (double)g.G[a];
                    idx[a] = in ? (int)v : 0;
                }
                if (in) {
                    cell = encode(idx, g.G, 3);   // row-major over the axes, as the list builders index their cells
                    mlist = fc_cnt[cell];
                }
            }
            if (mlist - 1u < (uint32_t)CAPF) {   // a list of 1..CAPF candidates, ids ascending
                const float4 *rec = fc_rec + (size_t)cell * CAPF;
                int bp = 0;
                bd = dist_canon<3>(p, rec[0]);
                for (uint32_t c = 1; c < mlist; ++c) {
                    const float dd = dist_canon<3>(p, rec[c]);
                    if (dd < bd) { bd = dd; bp = (int)c; }
                }
                bj = fc_lab[(size_t)cell * CAPF + bp];
            } else {
                bd = dist_canon<3>(p, C[0]);
                for (int j = 1; j < K; ++j) {
                    const float dd = dist_canon<3>(p, C[j]);
                    if (dd < bd) { bd = dd; bj = j; }
                }
            }
        }
        if (far || !(bd <= max_d2)) {   // trimmed
            if (carried) acc[1] += 1;
            else atomicAdd(row + 1, 1ull);
            continue;
        }
        // ---- the inlier's words
        const float4 c = C[bj];
        long long pq[3], cq[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pq[a] = (long long)fixed_i(p[a], qe.q[a]);
            cq[a] = (long long)fixed_i(comp(c, a), qe.q[a]);
        }
        u64 val[W];
        val[0] = 1;
        val[1] = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            val[2 + a] = (u64)pq[a];
            val[5 + a] = (u64)cq[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const long long pr = pq[a] * cq[b];
                val[8 + 2 * (3 * a + b)] = (u64)pr & 0xffffffffull;
                val[9 + 2 * (3 * a + b)] = (u64)(pr >> 32);
            }
            const long long pp = pq[a] * pq[a], cc = cq[a] * cq[a];
            val[26 + 2 * a] = (u64)pp & 0xffffffffull;
            val[27 + 2 * a] = (u64)(pp >> 32);
            val[32 + 2 * a] = (u64)cc & 0xffffffffull;
            val[33 + 2 * a] = (u64)(cc >> 32);
        }
        if (carried) {
#pragma unroll
            for (int w = 0; w < W; ++w) acc[w] += val[w];
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w != 1) atomicAdd(row + w, val[w]);
        }
    }
    flush();
    if (lane == 0 && skipped) atomicAdd(out + (long long)n_groups * W, (u64)skipped);
}

template <bool GROUPS>
__global__ __launch_bounds__(256) void k_align_apply(const float *__restrict__ X, long long n,
                                                     const uint8_t *__restrict__ groups, int n_groups,
                                                     const float *__restrict__ T, float *__restrict__ out) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const int grp = GROUPS ? (int)groups[i] : 0;
    float x[3], p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = X[i * 3 + a];
    if (grp < n_groups) rigid(T, grp, x, p);
    else {   // no transform for the row: NaN, so that pcm_align_stats skips it as it skips the group
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = __builtin_nanf("");
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out[i * 3 + a] = p[a];
}

}  // namespace

extern "C" {

int pcm_align_workspace(int64_t n_hint, int k, size_t *bytes) {
    if (!bytes) return fail(PCM_E_ARG, "bytes is null");
    if (int rc = align_args(n_hint, k)) return rc;
    AlignWs w;
    align_layout(n_hint, k, w);
    *bytes = w.total;
    return 0;
}

int pcm_align_prepare(const float *C, int k, int64_t n_hint, float max_d2, void *workspace, size_t workspace_bytes,
                      pcm_align_plan *plan, int64_t *info, void *stream) {
    if (int rc = align_args(n_hint, k)) return rc;
    if (!C || !plan) return fail(PCM_E_ARG, "pcm_align_prepare: C or plan is null");
    if (!(max_d2 >= 0.f)) return fail(PCM_E_ARG, "pcm_align_prepare: max_d2 must be >= 0 (+inf: no trimming)");
    if (info) info[0] = info[1] = info[2] = 0;
    hipStream_t s = (hipStream_t)stream;
    AlignPlan P;
    std::memset(&P, 0, sizeof(P));
    align_layout(n_hint, k, P.w);
    if (!workspace || workspace_bytes < P.w.total)
        return fail(PCM_E_ARG, "pcm_align_prepare: workspace too small (pcm_align_workspace)");
    // centres: finite (checked on the host), their box and how far they reach
    const size_t nce = (size_t)k * 3;
    std::unique_ptr<float[]> hc(new (std::nothrow) float[nce]);
    if (!hc) return fail(PCM_E_NOMEM, "pcm_align_prepare: host copy of the centres");
    HIPCHK(hipMemcpyAsync(hc.get(), C, nce * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) {
        P.clo[a] = std::numeric_limits<float>::infinity();
        P.chi[a] = -std::numeric_limits<float>::infinity();
    }
    for (size_t i = 0; i < nce; ++i) {
        if (!std::isfinite(hc[i])) return fail(PCM_E_ARG, "centres contain NaN or Inf");
        const int a = (int)(i % 3);
        P.clo[a] = std::min(P.clo[a], hc[i]);
        P.chi[a] = std::max(P.chi[a], hc[i]);
        P.cabs[a] = std::max(P.cabs[a], (double)std::fabs(hc[i]));
    }
    // The grid's box: the box of the centres, inflated on every axis by the trimming radius when
    // there is one (rows farther out are outliers), else by an eighth of its longest side (days
    // arrive displaced by a fraction of the scene).  The inflation never falls below 2^-10 of the
    // scene's reach, so that coplanar or identical centres still get cells of a usable extent;
    // the box decides which path a row takes, never its result.
    double maxext = 0.0, cabs = 0.0;
    for (int a = 0; a < 3; ++a) {
        maxext = std::max(maxext, (double)P.chi[a] - (double)P.clo[a]);
        cabs = std::max(cabs, P.cabs[a]);
    }
    double pad = std::isfinite(max_d2) ? std::sqrt((double)max_d2) * (1.0 + 1e-6) : 0.125 * maxext;
    pad = std::max({pad, std::ldexp(std::max(maxext, cabs), -10), 1e-30});
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)P.clo[a] - pad;
        hi[a] = (double)P.chi[a] + pad;
    }
    make_grid(P.g, 3, lo, hi, align_target(n_hint, k));
    clamp_grid(P.g, P.w.nc_max, std::numeric_limits<long long>::max());
    if (P.g.ncells > P.w.nc_max) return fail(PCM_E_STATE, "pcm_align_prepare: grid exceeds the workspace bound");
    // no pruning for one centre, and none where an fp32 distance inside the box can overflow
    if (k <= 1 || cabs + pad >= 1e18) P.g.prune = 0;
    int dev = 0;
    P.ncu = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&P.ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || P.ncu < 1)
        P.ncu = 256;
    char *wb = (char *)workspace;
    float4 *c4 = (float4 *)(wb + P.w.c4), *cref = (float4 *)(wb + P.w.cref), *fc_rec = (float4 *)(wb + P.w.fc_rec);
    Ctrl *ctrl = (Ctrl *)(wb + P.w.ctrl);
    uint32_t *fc_cnt = (uint32_t *)(wb + P.w.fc_cnt);
    int32_t *fc_lab = (int32_t *)(wb + P.w.fc_lab);
    unsigned long long *cand_stats = (unsigned long long *)(wb + P.w.cand_stats);
    k_predict_pack<<<blocks_for(k), 256, 0, s>>>(C, k, 3, c4);
    LAUNCHCHK();
    if (P.g.prune) {
        // k_cand records the centres its lists were built at and clears the drift budget: a private
        // control block and reference buffer take those stores (pcm_predict)
        HIPCHK(hipMemsetAsync(ctrl, 0, sizeof(Ctrl), s));
        const long long bpc = std::max(1LL, std::min(8LL, (2LL * P.ncu + P.g.ncoarse - 1) / P.g.ncoarse));
        if (int rc = host_candidates(3, P.g, c4, k, ctrl, 0, false, (int)bpc, fc_cnt, fc_rec, fc_lab, cref, nullptr,
                                     nullptr, SoleW{}, s))
            return rc;
        if (info) {
            unsigned long long hs[3] = {0, 0, 0};
            HIPCHK(hipMemsetAsync(cand_stats, 0, sizeof(hs), s));
            k_cand_stats<<<blocks_for(P.g.ncells), 256, 0, s>>>(fc_cnt, P.g.ncells, cand_stats);
            LAUNCHCHK();
            HIPCHK(hipMemcpyAsync(hs, cand_stats, sizeof(hs), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            info[0] = (int64_t)P.g.ncells;
            info[1] = (int64_t)hs[2];
            info[2] = (int64_t)hs[0];
        }
    }
    P.k = k;
    P.magic = PLAN_MAGIC;
    std::memset(plan, 0, sizeof(*plan));
    std::memcpy(plan, &P, sizeof(P));
    return 0;
}

int pcm_align_stats(const float *X, int64_t n, const uint8_t *groups, int n_groups, const float *T, float max_d2,
                    const int32_t *q, uint64_t *out, int64_t *info, const void *workspace, const pcm_align_plan *plan,
                    void *stream) {
    if (n < 0) return fail(PCM_E_ARG, "pcm_align_stats: n must be >= 0");
    if (n >= (int64_t)1 << 31) return fail(PCM_E_ARG, "pcm_align_stats: n must be below 2^31 (exactness of the limb sums)");
    if (n_groups < 1 || n_groups > PCM_ALIGN_MAXG)
        return fail(PCM_E_ARG, "pcm_align_stats: n_groups must be 1.." + std::to_string(PCM_ALIGN_MAXG));
    if (!(max_d2 >= 0.f)) return fail(PCM_E_ARG, "pcm_align_stats: max_d2 must be >= 0 (+inf: no trimming)");
    if (!plan || !workspace || !q) return fail(PCM_E_ARG, "pcm_align_stats: plan, workspace or q is null");
    AlignPlan P;
    std::memcpy(&P, plan, sizeof(P));
    if (P.magic != PLAN_MAGIC) return fail(PCM_E_STATE, "pcm_align_stats: the plan was not prepared (pcm_align_prepare)");
    if (info) info[0] = info[1] = info[2] = 0;
    if (n > 0 && (!X || !out)) return fail(PCM_E_ARG, "pcm_align_stats: X or out is null");
    AlignQ qe;
    for (int a = 0; a < 3; ++a) {
        qe.q[a] = q[a];
        if (q[a] < -126 || q[a] > 126) return fail(PCM_E_ARG, "pcm_align_stats: q out of range");
        // cq = trunc(ldexp(c, q)) must stay an int whose products with pq (|pq| < 2^QBITS) and with itself fit the limbs
        if (std::ldexp(P.cabs[a], q[a]) >= (double)(1 << 30))
            return fail(PCM_E_ARG, "pcm_align_stats: q does not cover the centres (|ldexp(c, q)| must be below 2^30)");
    }
    if (n == 0) return 0;   // nothing to add: no device call
    hipStream_t s = (hipStream_t)stream;
    AlignBox bx;
    for (int a = 0; a < 3; ++a) {
        bx.clo[a] = P.clo[a];
        bx.chi[a] = P.chi[a];
    }
    bx.skip = 0;
    bx.r = 0.f;
    if (std::isfinite(max_d2)) {
        // the smallest float r with fl(r * r) > max_d2 (see the head of this file); none when r * r never exceeds it
        volatile float r = std::sqrt(max_d2);
        for (int it = 0; it < 8; ++it) {
            volatile float rr = r * r;
            if (rr > max_d2) break;
            r = std::nextafter((float)r, std::numeric_limits<float>::infinity());
        }
        volatile float rr = r * r;
        if (rr > max_d2 && std::isfinite((float)r)) {
            bx.r = r;
            bx.skip = 1;
        }
    }
    const long long rounds = (n + 63) / 64;
    long long nblk = std::min<long long>((long long)P.ncu * 8, (rounds + A_WAVES * A_MIN_ROUNDS - 1) / (A_WAVES * A_MIN_ROUNDS));
    if (const char *e = std::getenv("PCM_ALIGN_BLOCKS")) {   // tests: the words must not depend on the grid
        const long long v = std::atoll(e);
        if (v >= 1) nblk = std::min<long long>(v, 1 << 20);
    }
    nblk = std::max<long long>(1, std::min(nblk, (rounds + A_WAVES - 1) / A_WAVES));
    const long long rpw = (rounds + nblk * A_WAVES - 1) / (nblk * A_WAVES);
    const char *wb = (const char *)workspace;
    const float4 *c4 = (const float4 *)(wb + P.w.c4), *fc_rec = (const float4 *)(wb + P.w.fc_rec);
    const uint32_t *fc_cnt = (const uint32_t *)(wb + P.w.fc_cnt);
    const int32_t *fc_lab = (const int32_t *)(wb + P.w.fc_lab);
    AlignGrid ag;
    for (int a = 0; a < 3; ++a) {
        ag.lo[a] = P.g.lo[a];
        ag.inv[a] = P.g.inv[a];
        ag.G[a] = P.g.G[a];
    }
    ag.prune = P.g.prune;
    auto launch = [&](auto GG, auto XX) {
        k_align<decltype(GG)::value, decltype(XX)::value><<<(unsigned)nblk, A_TPB, 0, s>>>(
            X, n, groups, n_groups, T, max_d2, qe, bx, ag, c4, P.k, fc_cnt, fc_rec, fc_lab, (u64 *)out, rounds, rpw);
    };
    using Yes = std::true_type;
    using No = std::false_type;
    if (groups && T) launch(Yes{}, Yes{});
    else if (groups) launch(Yes{}, No{});
    else if (T) launch(No{}, Yes{});
    else launch(No{}, No{});
    LAUNCHCHK();
    if (info) {
        info[0] = P.g.prune ? (int64_t)P.g.ncells : 0;
        info[1] = (int64_t)nblk;
        info[2] = (int64_t)rpw;
    }
    return 0;
}

int pcm_align_apply(const float *X, int64_t n, const uint8_t *groups, int n_groups, const float *T, float *out,
                    void *stream) {
    if (n < 0) return fail(PCM_E_ARG, "pcm_align_apply: n must be >= 0");
    if (n_groups < 1 || n_groups > PCM_ALIGN_MAXG)
        return fail(PCM_E_ARG, "pcm_align_apply: n_groups must be 1.." + std::to_string(PCM_ALIGN_MAXG));
    if (!T) return fail(PCM_E_ARG, "pcm_align_apply: T is null");
    if (n > 0 && (!X || !out)) return fail(PCM_E_ARG, "pcm_align_apply: X or out is null");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (groups) k_align_apply<true><<<blocks_for(n), 256, 0, s>>>(X, n, groups, n_groups, T, out);
    else k_align_apply<false><<<blocks_for(n), 256, 0, s>>>(X, n, groups, n_groups, T, out);
    LAUNCHCHK();
    return 0;
}

}  // extern "C"
