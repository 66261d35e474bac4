// pcm_inspect.hip — introspection of an engine's layout and lists, the synthetic clouds and the
// brute-force assign the tests and benchmarks compare against.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pcm_layout.hpp"   // k_tile_list_stats
#include "pcm_util.hpp"     // k_cand_stats, k_sole_stats, k_synth*, k_bruteforce
#include "pcm_host.hpp"

using namespace pcm;

extern "C" {

int pcm_layout_info(pcm_engine *e, int64_t *ncells, int64_t *ntiles, int *grid) {
    if (!e || !ncells || !ntiles || !grid) return fail(PCM_E_ARG, "bad argument");
    *ncells = e->g.ncells;
    if (e->layout_ready && e->ntiles < 0) {   // read back lazily (synchronises the device)
        uint32_t nt = 0;
        HIPCHK(hipMemcpy(&nt, e->ntiles_dev, sizeof(uint32_t), hipMemcpyDeviceToHost));
        e->ntiles = nt;
    }
    *ntiles = e->ntiles;
    for (int a = 0; a < MAXD; ++a) grid[a] = e->g.G[a];
    return 0;
}

int pcm_layout_stream_bytes(pcm_engine *e, double *bytes, int64_t *compressed_points) {
    if (!e || !bytes || !compressed_points) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    unsigned long long zr[32 * 16], z = 0;   // replica lines of k_tile_compress
    HIPCHK(hipMemcpy(zr, e->zpts, sizeof(zr), hipMemcpyDeviceToHost));
    for (int r = 0; r < 32; ++r) z += zr[r * 16];
    const double raw = (double)e->d * (double)tsize(e->dtype);
    *compressed_points = (int64_t)z;
    *bytes = (double)z * 8.0 + (double)(e->n - (long long)z) * raw;
    return 0;
}

int pcm_candidate_stats(pcm_engine *e, double *mean, int *mx, int64_t *full_cells, void *stream) {
    if (!e || !mean || !mx || !full_cells) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(e->cand_stats, 0, 3 * sizeof(unsigned long long), s));
    k_cand_stats<<<blocks_for(e->g.ncells), 256, 0, s>>>(e->fc_cnt, e->g.ncells, e->cand_stats);
    LAUNCHCHK();
    unsigned long long h[3];
    HIPCHK(hipMemcpyAsync(h, e->cand_stats, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    long long nonfull = e->g.ncells - (long long)h[2];
    *mean = nonfull > 0 ? (double)h[0] / (double)nonfull : 0.0;
    *mx = (int)h[1];
    *full_cells = (int64_t)h[2];
    return 0;
}

int pcm_sole_tiles(pcm_engine *e, int64_t *tiles, int64_t *points, void *stream) {
    if (!e || !tiles || !points) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    *tiles = *points = 0;
    if (e->n == 0 || e->ntiles_cap <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(e->cand_stats, 0, 2 * sizeof(unsigned long long), s));
    k_sole_stats<<<blocks_for(e->ntiles_cap), 256, 0, s>>>(e->tiles, e->ntiles_dev, e->cand_stats);
    LAUNCHCHK();
    unsigned long long h[2];
    HIPCHK(hipMemcpyAsync(h, e->cand_stats, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *tiles = (int64_t)h[0];
    *points = (int64_t)h[1];
    return 0;
}

int pcm_tile_list_stats(pcm_engine *e, int *zlev, int64_t *crowded_tiles, int64_t *listed_tiles, int64_t *listed_len,
                        void *stream) {
    if (!e || !zlev || !crowded_tiles || !listed_tiles || !listed_len) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    *zlev = e->zlev;
    *crowded_tiles = *listed_tiles = *listed_len = 0;
    if (e->zlev <= 0 || e->n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(e->cand_stats, 0, 6 * sizeof(unsigned long long), s));
    k_tile_list_stats<<<blocks_for(e->ntiles_cap), 256, 0, s>>>(e->tiles, e->ntiles_dev, e->fc_cnt, e->tl_cnt,
                                                                 e->cand_stats);
    LAUNCHCHK();
    unsigned long long h[3];
    HIPCHK(hipMemcpyAsync(h, e->cand_stats, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *crowded_tiles = (int64_t)h[0];
    *listed_tiles = (int64_t)h[1];
    *listed_len = (int64_t)h[2];
    return 0;
}

int pcm_tile_list_detail(pcm_engine *e, int64_t *long_lists, int64_t *allk_tiles, int64_t *max_len, void *stream) {
    if (!e || !long_lists || !allk_tiles || !max_len) return fail(PCM_E_ARG, "bad argument");
    if (!e->layout_ready) return fail(PCM_E_STATE, "layout not built");
    *long_lists = *allk_tiles = *max_len = 0;
    if (e->zlev <= 0 || e->n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(e->cand_stats, 0, 6 * sizeof(unsigned long long), s));
    k_tile_list_stats<<<blocks_for(e->ntiles_cap), 256, 0, s>>>(e->tiles, e->ntiles_dev, e->fc_cnt, e->tl_cnt,
                                                                 e->cand_stats);
    LAUNCHCHK();
    unsigned long long h[6];
    HIPCHK(hipMemcpyAsync(h, e->cand_stats, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *long_lists = (int64_t)h[3];
    *allk_tiles = (int64_t)h[4];
    *max_len = (int64_t)h[5];
    return 0;
}

int pcm_synth_uniform(float *out, int64_t n, int d, uint64_t seed, int64_t start, void *stream) {
    if ((!out && n > 0) || n < 0 || d < 1) return fail(PCM_E_ARG, "bad argument");
    if (n == 0) return 0;
    k_synth<<<blocks_for(n * d), 256, 0, (hipStream_t)stream>>>(out, n, d, seed, start);
    LAUNCHCHK();
    return 0;
}

int pcm_synth_rows(float *out, const int64_t *rows, int64_t m, int d, uint64_t seed, void *stream) {
    if ((!out || !rows) && m > 0) return fail(PCM_E_ARG, "bad argument");
    if (m == 0) return 0;
    k_synth_rows<<<blocks_for(m * d), 256, 0, (hipStream_t)stream>>>(out, (const long long *)rows, m, d, seed);
    LAUNCHCHK();
    return 0;
}

int pcm_assign_bruteforce(const float *X, int64_t n, int d, const float *C, int k, const int32_t *q, int32_t *labels,
                          uint64_t *stats, void *stream) {
    if ((!X && n > 0) || !C || !q || (!labels && n > 0) || k < 1 || n < 0) return fail(PCM_E_ARG, "bad argument");
    if ((size_t)k * sizeof(float4) > 160 * 1024) return fail(PCM_E_ARG, "k too large for LDS staging");
    if (n == 0) return 0;
    QExp qe{};
    for (int a = 0; a < MAXD; ++a) qe.q[a] = a < d ? q[a] : 0;
    hipStream_t s = (hipStream_t)stream;
    int nblk = (int)std::min<long long>((n + 255) / 256, 2048);
    return dispatch_d(d, [&](auto DD) -> int {
        constexpr int D = decltype(DD)::value;
        k_bruteforce<D><<<nblk, 256, (size_t)k * sizeof(float4), s>>>(X, n, C, k, qe, labels,
                                                                       (unsigned long long *)stats);
        LAUNCHCHK();
        return 0;
    });
}

}  // extern "C"
