/* pcm_kmeans.h — C ABI of the MI355X multi-day point-cloud K-means (Lloyd) engine.
 *
 * Drop-in boundary for the "Multi-day 3D Point Cloud" K-means step
 * (SURVEY.md §8b).  The reference has no K-means of its own: the step slots in
 * after the per-pair cloud assembly of members/rafael/disparity/plugin.py:147-192,
 * and its arithmetic follows scikit-learn's Lloyd, the only K-means the reference
 * executes (members/jasraj/land_use_classification/core.py:227-228):
 *
 *   pcm_fit_begin / pcm_iter_* / pcm_iterate   replace one call of
 *       sklearn/cluster/_kmeans.py:623-752 _kmeans_single_lloyd (its loop body is
 *       _k_means_lloyd.pyx:23-165 lloyd_iter_chunked_dense: E-step :168-213,
 *       accumulation :215-218 + :118-152, relocation _k_means_common.pyx:167-211,
 *       averaging :274-295, shift :298-311, convergence _kmeans.py:717-732);
 *   pcm_final                                 replaces the final E-step and
 *       inertia of _kmeans.py:736-750;
 *   pcm_labels / pcm_get_centers              return the fit outputs (labels in
 *       the caller's original row order, centres (K, D) float32).
 *
 * Conventions (modelled on lloyd_iter_chunked_dense's in-place contract,
 * _k_means_lloyd.pyx:23-32): caller-owned device buffers (torch tensors),
 * outputs written in place, no allocation and no host synchronisation in the
 * per-iteration entry points (pcm_iter_*, pcm_iterate, pcm_final), all work
 * ordered on the hipStream_t passed as `stream` (NULL = default stream).
 * Every function returns 0 on success or a negative PCM_E* code; the message of
 * the last failure on the calling thread is available from pcm_last_error.
 * Nothing throws across this ABI.  One engine must not be used from two
 * threads at once; distinct engines are independent.
 * Load this library after the process has loaded libamdhip64.so.7 (e.g. after
 * `import torch`) so that one HIP runtime serves both.
 */
#ifndef PCM_KMEANS_H
#define PCM_KMEANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCM_ABI_VERSION 8

enum pcm_dtype { PCM_F32 = 0, PCM_F16 = 1, PCM_F64 = 2 /* dense path only */ };

#define PCM_DENSE_DMAX 64   /* features of the generic-D (dense) path */

enum pcm_err {
    PCM_OK = 0,
    PCM_E_ARG = -1,      /* invalid argument / shape */
    PCM_E_HIP = -2,      /* HIP runtime or kernel launch failure */
    PCM_E_STATE = -3,    /* call out of order (e.g. iterate before layout) */
    PCM_E_NONFINITE = -4,/* input points contain NaN or Inf */
    PCM_E_NOMEM = -5
};

/* Device-side iteration status, copied to the host by pcm_read_status. */
typedef struct pcm_status {
    uint32_t halt;       /* 1: empty clusters need relocation (pcm_reloc_*) */
    uint32_t done;       /* 0 running, 1 strict label convergence, 2 shift<=tol, 3 max_iter,
                            4 a peer exchange timed out (pcm_iter_exchange; the fit is void),
                            5 the update's publisher block timed out waiting for its list blocks (void) */
    uint32_t iter;       /* completed Lloyd iterations */
    uint32_t n_empty;    /* empty clusters seen by the halted iteration */
    double inertia;      /* local inertia of the last pcm_final (= pcm_inertia_value of the fields below) */
    uint64_t last_changed;   /* statistic words (of K*(D+1)) that differ from the previous iteration's:
                                NOT a count of changed labels -- 0 exactly when no label changed */
    double last_shift;
    /* Exact, order-independent inertia: sum over points of trunc(d * 2^scale)
     * (d = canonical fp32 distance to the final centre) as 32-bit limbs
     * inertia_limbs[0] + 2^32 [1] + 2^64 [2].  Sum-all-reduce the limbs over
     * ranks, then pcm_inertia_value gives the global inertia; the result is
     * bit-identical for any world size. */
    uint64_t inertia_limbs[3];
    int32_t inertia_scale;
    uint32_t inertia_overflow;   /* > 0: a distance exceeded the bound (inertia = +inf) */
    uint32_t list_rebuilds;      /* candidate-list rebuilds so far in this fit (the other iterations
                                    only refreshed the lists' centre records) */
    uint32_t pad_;
} pcm_status;

typedef struct pcm_engine pcm_engine;

int pcm_abi_version(void);
/* Inertia from (all-reduced) limbs: ldexp((double)(l0 + l1 2^32 + l2 2^64), -scale),
 * one correctly rounded conversion; +inf when overflow > 0. */
double pcm_inertia_value(const uint64_t *limbs, int scale, uint32_t overflow);
int pcm_last_error(char *buf, size_t n);

/* Create an engine for D-dimensional points (1..4), K clusters, on HIP device
 * `device`.  `max_iter` sizes the per-iteration history. */
int pcm_engine_create(int device, int d, int k, int dtype, int max_iter, pcm_engine **out);
int pcm_engine_destroy(pcm_engine *e);

/* Layout, step 1 (host-synchronising, once per point cloud): local bounding box
 * of X (n rows, row-major, dtype given at create) on device.  Writes lo[d],
 * hi[d], maxabs[d] (host arrays).  Returns PCM_E_NONFINITE for NaN/Inf input. */
int pcm_layout_bbox(pcm_engine *e, const void *X, int64_t n, void *stream,
                    double *lo, double *hi, double *maxabs);

/* Layout, step 2 (host-synchronising, once): bin rows into the pruning grid,
 * sort them into cell order (AoSoA-4: groups of 4 points stored coordinate-major)
 * and build the tile list.  `q` are the
 * GLOBAL fixed-point exponents (identical on every rank), `gidx0` the global row
 * index of local row 0 (relocation tie-break).  X must stay unchanged until
 * this call returns. */
int pcm_layout_build(pcm_engine *e, const void *X, const int32_t *q, int64_t gidx0, void *stream);

/* Optional, at engine setup: grow (and zero) the point-sized device buffers a
 * layout of up to `n` points needs, so that the first pcm_layout_build of a
 * process allocates nothing large (a fresh process's first allocations map
 * and clear new VRAM).  Buffers only grow; invalidates the current layout.
 * No reference counterpart (the reference allocates per call). */
int pcm_engine_reserve(pcm_engine *e, int64_t n, void *stream);

/* Layout, optional step between pcm_layout_bbox and pcm_layout_build: the
 * engine's cloud is a SPATIAL shard of a fit over `n_global` points on all
 * ranks (pcm_shard_* below).  `rows` (device uint32[n], copied) is each local
 * point's global row index -- the relocation tie-break (distance desc, global
 * row asc, _k_means_common.pyx:185-187) -- and n_global scales the pruning-grid
 * policy (cells per centre) to the whole cloud.  Reset by pcm_layout_bbox. */
int pcm_layout_shard(pcm_engine *e, const uint32_t *rows, int64_t n_global, void *stream);

/* Start a fit from centres C0 (device, K*D float32): labels := -1, history
 * cleared, absolute shift tolerance `tol`, iteration cap `max_iter`. */
int pcm_fit_begin(pcm_engine *e, const float *C0, double tol, int max_iter, void *stream);

/* One Lloyd iteration split at the all-reduce:
 *   pcm_iter_local   assign + exact accumulation of the local integer
 *                    statistics straight into the buffer of pcm_stats_ptr;
 *   (caller all-reduces that buffer with SUM over ranks when world size > 1)
 *   pcm_iter_global  empty-cluster check (may set halt), averaging, shift,
 *                    convergence flags, the next iteration's candidate lists;
 *                    zeroes the statistics buffer for the next iteration.
 * Both are gated on the device: after convergence or halt they are no-ops. */
int pcm_iter_local(pcm_engine *e, void *stream);
int pcm_iter_global(pcm_engine *e, void *stream);
/* n x (local, global) on one device without any host synchronisation. */
int pcm_iterate(pcm_engine *e, int n, void *stream);

/* Device pointer + element count (int64) of the per-iteration statistics
 * buffer: K*(D+1) offset-encoded fixed-point sums and counts, then 1 change
 * count.  Sum-all-reduce it between pcm_iter_local and pcm_iter_global. */
int pcm_stats_ptr(pcm_engine *e, void **ptr, int64_t *count);
/* Use a caller-owned device buffer of pcm_stats_ptr's count int64 elements
 * (e.g. a torch tensor handed to torch.distributed.all_reduce) instead of the
 * engine's own; NULL reverts to the engine buffer. */
int pcm_bind_stats(pcm_engine *e, void *ptr);

/* Empty-cluster relocation (run only after pcm_read_status reports halt):
 * write this rank's `m` farthest-from-centre points as 32-byte records to
 * `records` (device, m*32 bytes); the caller concatenates every rank's records
 * (all-gather) and passes all `n_rec` of them to pcm_reloc_apply, which picks
 * the global farthest, moves them into the empty clusters, clears halt and
 * completes the iteration. */
int pcm_reloc_candidates(pcm_engine *e, int m, void *records, void *stream);
int pcm_reloc_apply(pcm_engine *e, const void *records, int n_rec, void *stream);

/* Final E-step with the final centres (labels + local inertia). */
int pcm_final(pcm_engine *e, void *stream);
/* Labels in the caller's original row order (device int32[n]). */
int pcm_labels(pcm_engine *e, int32_t *out, void *stream);
/* Current centres (device float32[K*D]). */
int pcm_get_centers(pcm_engine *e, float *out, void *stream);
/* Per-iteration history (host arrays of length >= iter): changed statistic words
 * (as pcm_status.last_changed; 0 exactly when no label changed), shifts. */
int pcm_history(pcm_engine *e, uint64_t *changed, double *shift, int cap, void *stream);
/* Synchronise `stream` and copy the device status. */
int pcm_read_status(pcm_engine *e, pcm_status *out, void *stream);
/* The same without draining the stream (round 6): pcm_status_post queues a
 * snapshot of the status behind the work enqueued so far; pcm_status_wait
 * blocks until that snapshot has landed and decodes it.  One snapshot in flight
 * per engine (a post overwrites the previous one). */
int pcm_status_post(pcm_engine *e, void *stream);
int pcm_status_wait(pcm_engine *e, pcm_status *out);

/* Layout facts for diagnostics: cells, tiles, grid dims (host ints). */
int pcm_layout_info(pcm_engine *e, int64_t *ncells, int64_t *ntiles, int *grid /*[4]*/);
/* Bytes the assign kernel streams per iteration for the current layout (points
 * in compressed tiles at 8 B, the others at d * sizeof(dtype)) and the number
 * of compressed points (synchronising; see DESIGN.md §3, compressed stream). */
int pcm_layout_stream_bytes(pcm_engine *e, double *bytes, int64_t *compressed_points);
/* Name of the assign-kernel variant the current layout launches per iteration
 * (e.g. "k_lloyd1<float,3,8,false>"), for measurement records. */
int pcm_assign_kernel_name(pcm_engine *e, char *buf, size_t n);
/* Mean/max fine candidate-list length of the last iteration (synchronising). */
int pcm_candidate_stats(pcm_engine *e, double *mean, int *max, int64_t *full_cells, void *stream);
/* Sole-owner tiles of the current candidate lists: tiles whose cell has a
 * one-entry list, which the assign kernel credits to that centroid from the
 * tile's layout-time sums without reading its points, and the points they hold
 * (synchronising; 0 / 0 with PCM_SOLE=0). */
int pcm_sole_tiles(pcm_engine *e, int64_t *tiles, int64_t *points, void *stream);
/* Crowded layouts (cells holding many tiles' worth of points, e.g. tight
 * clusters): the Morton levels of the in-cell point order (0: not crowded),
 * the tiles of cells whose list is FULL or longer than 16 at the last
 * iteration, how many of them got a shorter tile list and those lists' summed
 * length (synchronising). */
int pcm_tile_list_stats(pcm_engine *e, int *zlev, int64_t *crowded_tiles, int64_t *listed_tiles, int64_t *listed_len,
                        void *stream);
/* Crowded layouts, the long-list paths of the assign kernel: tile lists longer
 * than 256 (scanned through LDS chunks), all-K tiles (a FULL cell's tile with no
 * list of at most 1024) and the longest tile list (synchronising; 0 when not
 * crowded). */
int pcm_tile_list_detail(pcm_engine *e, int64_t *long_lists, int64_t *allk_tiles, int64_t *max_len, void *stream);

/* Kernel timing on the engine's launch stream (HIP events around every launch
 * of the assign kernel and of the candidate and tail kernels).  enable=1 starts
 * recording (resets the sums), pcm_timing_read synchronises and returns mean
 * milliseconds per iteration for: [0] assign, [1] candidates, [2] fold+global,
 * and the number of iterations timed. */
int pcm_timing(pcm_engine *e, int enable);
int pcm_timing_read(pcm_engine *e, double *ms /*[3]*/, int *count);

/* Calibration: mean milliseconds of `reps` back-to-back assign launches on the
 * current layout and centres, between one HIP event pair.  The statistics they
 * add are discarded; the engine needs pcm_fit_begin before iterating again. */
int pcm_time_assign(pcm_engine *e, int reps, void *stream, double *ms);

/* Rows `rows[0..m)` (device int64) of the synthetic cloud, device float32[m*d]. */
int pcm_synth_rows(float *out, const int64_t *rows, int64_t m, int d, uint64_t seed, void *stream);

/* Counter-based U[0,1) synthetic cloud (identical to oracle.splitmix_uniform):
 * out[(i)*d + a] for rows [start, start+n), device float32. */
int pcm_synth_uniform(float *out, int64_t n, int d, uint64_t seed, int64_t start, void *stream);

/* Stateless operator (sklearn lloyd_iter_chunked_dense shape, unit weights,
 * brute force over all K, LDS-staged centres): labels (device int32[n]) and
 * integer statistics (device uint64[K*(D+1)], accumulated, caller zeroes)
 * for centres C (device float32[K*D]).  q = fixed-point exponents. */
int pcm_assign_bruteforce(const float *X, int64_t n, int d, const float *C, int k,
                          const int32_t *q, int32_t *labels, uint64_t *stats, void *stream);

/* ---------------------------------------------------------------- predict
 * Labels (and distances, inertia) of a cloud against GIVEN centres: the E-step
 * of sklearn's KMeans.predict / score (_labels_inertia, sklearn/cluster/
 * _kmeans.py:1083-1108) in the canonical arithmetic of pcm_final, without the
 * layout sort -- the rows keep the caller's order.  X: device n*d rows
 * (PCM_F32 or PCM_F16, d = 1..4); C: device float32[k*d], anywhere relative to
 * X (finite; checked on the host).  labels: device int32[n]; dist (nullable):
 * device float32[n], the canonical squared distance to the assigned centre.
 * inertia (nullable, host): the exact limbs of sum trunc(dist * 2^scale) and
 * the overflow count, scale derived from `q` (host int32[d], the fixed-point
 * exponents of X AND C together, identical on every rank; used only for the
 * inertia -- labels and distances never depend on it).  Multi-rank callers sum
 * limbs and overflow over the ranks, then pcm_inertia_value.  info (nullable,
 * host int64[3]): cells of the pruning grid, cells whose list is FULL (their
 * points scan all k centres), summed length of the other lists; all 0 when no
 * lists were built (k = 1, or coordinates near the fp32 range).
 * Synchronises `stream` (centres, bounding box, and the host outputs);
 * PCM_E_NONFINITE for NaN/Inf in X, PCM_E_ARG for NaN/Inf in C (k <= 2^24);
 * n = 0 succeeds without any device call (the centres are then not checked).  workspace: caller-owned device memory of
 * pcm_predict_workspace bytes. */
typedef struct pcm_inertia {
    uint64_t limbs[3];
    uint32_t overflow;
    int32_t scale;
} pcm_inertia;
int pcm_predict_workspace(int64_t n, int d, int k, size_t *bytes);
int pcm_predict(const void *X, int dtype, int64_t n, int d, const float *C, int k, const int32_t *q, int32_t *labels,
                float *dist, pcm_inertia *inertia, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- cluster statistics
 * Exact per-(group, cluster) zeroth, first and second moments of a labelled
 * cloud, in one pass over the rows in the caller's order (no reference
 * counterpart: the reference never fuses days; DESIGN.md §4 "Cluster
 * statistics").  X: device n*d rows (PCM_F32 or PCM_F16, d = 1..4); labels:
 * device int32[n] (e.g. of pcm_labels / pcm_predict); groups (nullable: every
 * row in group 0): device uint8[n], the day / cloud of each row; q: host
 * int32[d], the fixed-point exponents of the fit (fixed.fixed_q).
 * With xq_a = trunc(ldexp(x_a, q_a)) (the engine's fixed point), the row of
 * (g, j) at out + (g*k + j)*W, W = PCM_STATS_WORDS(d), holds
 *   word 0         the number of rows;
 *   words 1..d     sum xq_a (int64 two's complement);
 *   then for each pair a <= b (upper triangle, row-major) two words: with the
 *   int64 product p = xq_a*xq_b (|p| < 2^50)
 *       lo += (uint64)p & 0xffffffff,  hi += (uint64)(p >> 32)  (arithmetic
 *   shift, wrapping add); the pair's value is lo + 2^32 * (int64)hi.
 * The sums are EXACT while fewer than 2^31 rows in total have been accumulated
 * into one `out` (over all calls and ranks that were added into it): lo then
 * stays below 2^63 and |hi| below 2^49.  Every add is an integer add, so the
 * words are the same bit pattern for any order of the rows, any grid, and any
 * split of the rows over calls or ranks (sum the words).
 * A row whose label is outside [0, k), whose group is >= n_groups or which has
 * a non-finite coordinate is skipped: it adds nothing to any row and 1 to the
 * trailing word out[n_groups*k*W].
 * out: device uint64[n_groups*k*W + 1], ACCUMULATED -- the caller zeroes it.
 * Stream-ordered: no host synchronisation, no allocation.  The arguments are
 * checked before any device call (PCM_E_ARG: d, dtype, n < 0, n >= 2^31,
 * k < 1, n_groups outside 1..PCM_STATS_MAXG, n_groups*k >= 2^31, a null out,
 * labels, X or q with n > 0); n = 0 succeeds without any device call. */
#define PCM_STATS_WORDS(d) (1 + (d) + (d) * ((d) + 1))      /* D=3: 16 words = 128 B */
#define PCM_STATS_MAXG 256
int pcm_cluster_stats(const void *X, int dtype, int64_t n, int d,
                      const int32_t *labels, const uint8_t *groups /* nullable: all group 0 */,
                      int n_groups, int k, const int32_t *q /* host int32[d] */,
                      uint64_t *out /* device, n_groups*k*W + 1 words, ACCUMULATED: caller zeroes */,
                      void *stream);

/* ---------------------------------------------------------------- height grid
 * Exact height-map raster of a (labelled, multi-day) cloud, in one pass over
 * the rows in the caller's order (no reference counterpart: the reference
 * rasters one pair and never fuses days; DESIGN.md §4 "Height grid").
 * X: device float32 n*3 rows (z, y, x), the plugin's column order; labels
 * (nullable: every row label 0): device int32[n], valid in [0, k); groups
 * (nullable: every row in group 0): device uint8[n], the day / cloud of each
 * row; H, W: the raster; (oy, ox): its origin; cell_log2 = s: a cell is 2^s
 * units on a side, -8 <= s <= 16; q: the fixed-point exponent of z
 * (fixed.fixed_q of max |z|).
 * In float32 (one rounded subtraction, an exact scaling, a floor)
 *   fy = floorf(ldexpf(y - oy, -s)),  fx = floorf(ldexpf(x - ox, -s)),
 * the row is inside iff 0 <= fy < H and 0 <= fx < W (compared as floats), and
 *   zq = trunc(ldexp(z, q))           (the engine's fixed point).
 * Word w of group g is the H x W plane at out + (g*4 + w)*H*W, the pixel at
 * fy*W + fx inside it.  An inside row updates the four words of its (g, pixel):
 *   word 0   += 1                                            (count)
 *   word 1   += zq                    (int64 two's complement, wrapping add)
 *   word 2   = max(word 2, ((uint64)(zq + 2^25) << 32) | (0xffffffff - label))   (top)
 *   word 3   = max(word 3, ((uint64)(2^25 - zq) << 32) | (0xffffffff - label))   (bottom)
 * (unsigned 64-bit maxima).  A zero word 2 / 3 means no row: a zeroed buffer
 * is the empty grid.  Among rows of equal height the smaller label wins.
 * After the planes come two words: out[n_groups*4*H*W] counts the valid rows
 * outside the raster, out[n_groups*4*H*W + 1] the skipped rows -- a row with a
 * non-finite coordinate, a label outside [0, k), a group >= n_groups or
 * |zq| >= 2^25 updates nothing else.
 * The sums are EXACT while fewer than 2^31 rows in total have been accumulated
 * into one `out`.  Adds and maxima of integers commute, so the words are the
 * same bit pattern for any order of the rows, any grid, and any split of the
 * rows over calls or ranks (add words 0-1, take the maximum of words 2-3).
 * out: device uint64[n_groups*4*H*W + 2], ACCUMULATED -- the caller zeroes it.
 * Stream-ordered: no host synchronisation, no allocation.  The arguments are
 * checked before any device call (PCM_E_ARG: n < 0, n >= 2^31, H or W outside
 * 1..2^24, n_groups outside 1..PCM_GRID_MAXG, n_groups*H*W >= 2^31, k < 1,
 * cell_log2 outside -8..16, a null X or out with n > 0); n = 0 succeeds
 * without any device call. */
#define PCM_GRID_WORDS 4
#define PCM_GRID_MAXG 256
int pcm_height_grid(const float *X, int64_t n,
                    const int32_t *labels /* nullable: all label 0 */, int k,
                    const uint8_t *groups /* nullable: all group 0 */, int n_groups,
                    int H, int W, float oy, float ox, int cell_log2, int q,
                    uint64_t *out /* device, n_groups*4*H*W + 2 words, ACCUMULATED: caller zeroes */,
                    void *stream);

/* ---------------------------------------------------------------- registration
 * Exact statistics for co-registering labelled days (groups) onto fixed centres
 * (no reference counterpart: the reference builds every pair's cloud in that
 * pair's own frame and never registers them; DESIGN.md §4 "Registration:
 * k_align").  X: device float32 n*3 rows (z, y, x); C: device float32 k*3.
 *
 * pcm_align_prepare, once per set of centres: copies and checks the centres on
 * the host (PCM_E_ARG for NaN/Inf; synchronises `stream`), lays the pruning grid
 * over the box of the CENTRES -- inflated by sqrt(max_d2) when that is finite,
 * else by an eighth of its longest side, and never by less than 2^-10 of the
 * centres' reach (coplanar, identical or single centres) -- and builds the exact
 * candidate lists.  n_hint (the rows a pcm_align_stats call will see) sizes the
 * grid only.  workspace: caller-owned device memory of pcm_align_workspace(n_hint,
 * k) bytes, read by every later pcm_align_stats; plan: host, filled here, passed
 * on unchanged.  info (nullable, host int64[3]): cells, FULL cells, summed
 * length of the other lists (all 0 without lists: k = 1).
 *
 * pcm_align_stats: one launch, no host synchronisation, no allocation.  For
 * each row i of group g (groups nullable: all group 0), in float32 with every
 * operation rounded,
 *   p_a = ((R_a0*x_0 + R_a1*x_1) + R_a2*x_2) + t_a,
 * T: device float32[n_groups*12], per group R row-major then t (NULL: p = x);
 * j = the canonical nearest centre of p (the fit's fp32 distance, strict <,
 * lowest index on ties), d2 that distance; the row is an inlier iff
 * d2 <= max_d2 (float32 compare; +inf admits every row).  With
 * pq_a = trunc(ldexp(p_a, q_a)), cq_a = trunc(ldexp(c_ja, q_a)) (q: host
 * int32[3]) the group's row out + g*PCM_ALIGN_WORDS holds
 *   word 0        inliers            word 1        outliers (valid rows, trimmed)
 *   words 2..4    sum pq_a           words 5..7    sum cq_a       (inliers)
 *   words 8..25   sum pq_a*cq_b, the nine (a, b) row-major, two words each:
 *                 lo += (uint64)p & 0xffffffff, hi += (uint64)(p >> 32)
 *   words 26..31  sum pq_a^2 (lo, hi)    words 32..37  sum cq_a^2 (lo, hi)
 * A row with a non-finite x or p, a group >= n_groups or some
 * |ldexp(p_a, q_a)| >= 2^25 is skipped: it adds 1 to out[n_groups*38] and
 * nothing else.  EXACT while fewer than 2^31 rows in all went into one `out`;
 * every add is an integer add, so the words are the same bits for any row
 * order, any grid (PCM_ALIGN_BLOCKS overrides it) and any split of the rows over
 * calls, chunks and ranks.  out: device uint64[n_groups*38 + 1], ACCUMULATED.
 * PCM_E_ARG when |ldexp(c, q)| >= 2^30 for some centre.  info (nullable, host
 * int64[3]): cells of the grid, blocks launched, rounds of 64 rows per wave.
 *
 * pcm_align_apply writes p (same arithmetic) for every row; a row whose group
 * is >= n_groups gets NaN. */
#define PCM_ALIGN_WORDS 38
#define PCM_ALIGN_MAXG 256
typedef struct pcm_align_plan {
    uint64_t opaque[64];
} pcm_align_plan;
int pcm_align_workspace(int64_t n_hint, int k, size_t *bytes);
int pcm_align_prepare(const float *C, int k, int64_t n_hint, float max_d2, void *workspace, size_t workspace_bytes,
                      pcm_align_plan *plan, int64_t *info, void *stream);
int pcm_align_stats(const float *X, int64_t n, const uint8_t *groups /* nullable */, int n_groups,
                    const float *T /* device, nullable */, float max_d2, const int32_t *q /* host int32[3] */,
                    uint64_t *out /* device, n_groups*38 + 1 words, ACCUMULATED: caller zeroes */,
                    int64_t *info, const void *workspace, const pcm_align_plan *plan, void *stream);
int pcm_align_apply(const float *X, int64_t n, const uint8_t *groups /* nullable */, int n_groups,
                    const float *T /* device */, float *out, void *stream);

/* ---------------------------------------------------------------- support
 * Exact fixed-radius neighbour counts and day support of a cloud, the basis of
 * the radius outlier filter (no reference counterpart: the reference never
 * removes the speckle of its disparity maps; DESIGN.md §4 "Support").
 * X: device float32 n*3 rows (z, y, x).  With r2 = radius * radius (float32),
 * row j is a neighbour of row i (j != i) iff, in float32, every operation
 * rounded, no contraction,
 *   dz = z_i - z_j, dy = y_i - y_j, dx = x_i - x_j,  (dz*dz + dy*dy) + dx*dx <= r2.
 * Duplicates of a row are its neighbours; a row with a NaN or Inf coordinate
 * has no neighbours, is nobody's neighbour and gets counts = days = 0.
 *   counts[i] = min(neighbours of i, max_count)      (max_count < 0: no limit)
 *   days[i]   = distinct groups among row i and its neighbours (exact whatever
 *               max_count is; groups NULL: every row in group 0)
 * Three steps, all stream-ordered, no host synchronisation, no allocation:
 *   pcm_support_keys   fills info (device int64[PCM_SUPPORT_INFO_WORDS]) and
 *                      keys (device int64[n]): the row's cell, 21 bits per axis,
 *                      x fastest; 2^63 - 1 for a non-finite row;
 *   (the caller sorts: sorted_keys ascending and perm, sorted_keys[i] =
 *    keys[perm[i]] -- any sort, ties in any order)
 *   pcm_support_count  gathers the cell-sorted copy into the workspace
 *                      (pcm_support_workspace bytes) and counts; writes counts
 *                      (device int32[n]) and, when days is not NULL, days
 *                      (device int32[n]) in the caller's row order.
 * info: [0] the cell exponent s (a cell is 2^s units on a side: the smallest s
 * with 2^s >= radius (1 + 2^-20), at least -32, raised until |x| 2^-s <= 2^40
 * and every axis spans at most 2^21 cells); [1..3] the cell of the box's low
 * corner (z, y, x); [4..6] the bits each axis needs; [7] the rows skipped as
 * non-finite; [8..14] internal; [15] set when perm held a value outside [0, n)
 * (that row is left unwritten).  groups: device uint8[n] with values below
 * n_groups (the caller checks; the kernel uses the low 6 bits).
 * The results are integers decided by the predicate alone -- the cells only
 * prune -- so they are the same bits for any row order, sort and launch shape.
 * Cost: a row is tested against every row of the cells around it, so the count
 * grows with the SQUARE of a cell's population (many duplicates, or a radius
 * far above the point spacing).  A cell run longer than PCM_SUPPORT_CHUNK rows
 * is staged in several chunks.  PCM_SUPPORT_PHASE=1 / 2 in the environment runs
 * only the gather / only the count (measurement).
 * The arguments are checked before any device call (PCM_E_ARG: n < 0,
 * n >= 2^31, radius not finite or <= 0, n_groups outside 1..PCM_SUPPORT_MAXG,
 * a null pointer with n > 0, a workspace too small); n = 0 succeeds without
 * counting. */
#define PCM_SUPPORT_CHUNK 128
#define PCM_SUPPORT_TPB 256
#define PCM_SUPPORT_MAXG 64
#define PCM_SUPPORT_INFO_WORDS 16
int pcm_support_workspace(int64_t n, size_t *bytes);
int pcm_support_keys(const float *X, int64_t n, float radius, int64_t *keys, int64_t *info, void *stream);
int pcm_support_count(const float *X, int64_t n, const uint8_t *groups /* nullable */, int n_groups, float radius,
                      int max_count, const int64_t *sorted_keys, const int64_t *perm, int32_t *counts,
                      int32_t *days /* nullable */, int64_t *info, void *workspace, size_t workspace_bytes,
                      void *stream);

/* ---------------------------------------------------------------- voxels
 * Exact voxel-grid reduction of a cloud: one entry per occupied voxel with its
 * count, fixed-point coordinate sums, lowest row and the groups (days) that saw
 * it (no reference counterpart; DESIGN.md §4 "Voxels").  X: device float32 n*3
 * rows (z, y, x).  voxel, origin: HOST float32[3] (z, y, x): sizes finite and
 * > 0, origin finite.  On axis a the cell of a finite row is, in float32, every
 * operation rounded, no contraction,
 *   c_a = floorf((x_a - origin_a) * inv_a),  inv_a = (float)(1.0 / (double)voxel_a)
 * (inv_a must be a finite normal float32).  A row with a NaN or Inf coordinate
 * belongs to no voxel.  Four steps, all stream-ordered, no allocation:
 *   pcm_voxel_keys    fills info (device int64[PCM_VOXEL_INFO_WORDS]) and keys
 *                     (device int64[n]): the row's cell relative to the cell of
 *                     the box's low corner, 21 bits per axis, x fastest; 2^63 - 1
 *                     for a non-finite row (and for every row when info[0] != 0);
 *   (the caller sorts: sorted_keys ascending and perm, sorted_keys[i] =
 *    keys[perm[i]] -- any sort, ties in any order)
 *   pcm_voxel_count   counts the segment heads of the sorted keys per wave of 64
 *                     rows into the workspace (pcm_voxel_workspace bytes), scans
 *                     them and writes the number of voxels M to info[8];
 *   (the caller reads info once: the error word, M, the skipped rows, the box)
 *   pcm_voxel_reduce  with m = M: for voxel v in ascending (cz, cy, cx) order
 *                     cells[v*3 + a] (int64) the absolute cell, counts[v] (int32),
 *                     sums[v*3 + a] (int64) = sum of trunc(ldexp(x_a, q_a)) taken
 *                     as int32 (q: HOST int32[3]), first[v] (int32) the lowest
 *                     row, day_mask[v] (int64, with groups) bit g set iff a row of
 *                     group g is in v; inverse[i] (int32[n]) the voxel of row i,
 *                     -1 for a non-finite row.  It initialises the outputs itself.
 * info: [0] 0 or PCM_VOXEL_E_* bits over the finite rows' box: a non-finite
 * cell, |cell| > 2^40, an axis spanning more than 2^21 cells (or all three
 * spanning exactly 2^21: the last key would be the skip key); [1..3] the cell of
 * the box's low corner; [4..6] the cells each axis spans; [7] the rows skipped
 * as non-finite; [8] M; [9..14] the box of the finite rows, low then high corner,
 * as order-preserving uint32 (u = bits ^ 0xffffffff for a negative float, bits |
 * 0x80000000 otherwise); [15] set when perm held a value outside [0, n) or the
 * keys changed between count and reduce (such rows are left unwritten).
 * groups: device uint8[n] with values below n_groups (the caller checks; the
 * kernel uses the low 6 bits).  Only a wave's first and last segment, when they
 * continue in a neighbouring wave, are written with integer atomics; integer
 * adds, ors and minima commute, so the outputs are the same bits for any row
 * order, sort and launch shape.  Exact while |ldexp(x_a, q_a)| < 2^31.
 * The arguments are checked before any device call (PCM_E_ARG: n < 0,
 * n >= 2^31, a null pointer, a bad size or origin, m outside [0, n], n_groups
 * outside 1..PCM_VOXEL_MAXG, a workspace too small); n = 0 makes no device call
 * beyond initialising info. */
#define PCM_VOXEL_TPB 256
#define PCM_VOXEL_MAXG 64
#define PCM_VOXEL_INFO_WORDS 16
#define PCM_VOXEL_E_NONFINITE 1
#define PCM_VOXEL_E_MAGNITUDE 2
#define PCM_VOXEL_E_SPAN 4
int pcm_voxel_workspace(int64_t n, size_t *bytes);
int pcm_voxel_keys(const float *X, int64_t n, const float *voxel /* host float[3] */,
                   const float *origin /* host float[3] */, int64_t *keys, int64_t *info, void *stream);
int pcm_voxel_count(const int64_t *sorted_keys, int64_t n, int64_t *info, void *workspace, size_t workspace_bytes,
                    void *stream);
int pcm_voxel_reduce(const float *X, int64_t n, const uint8_t *groups /* nullable */, int n_groups,
                     const int32_t *q /* host int32[3] */, const int64_t *sorted_keys, const int64_t *perm, int64_t m,
                     int64_t *cells, int32_t *counts, int64_t *sums, int32_t *first, int64_t *day_mask /* nullable */,
                     int32_t *inverse, int64_t *info, const void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- nearest
 * Exact nearest row of another cloud within a radius: the cloud-to-cloud
 * distance (no reference counterpart; DESIGN.md §4 "Nearest").  Queries X
 * (n rows) and targets Y (m rows): device float32 rows (z, y, x); X and Y may be
 * the same array.  With r2 = radius * radius (float32; both must be finite and
 * > 0), target j is a candidate of query i iff both rows are finite, groups[i]
 * != target_groups[j] (when the two are given; device int32, any values,
 * compared for equality only) and, in float32, every operation rounded, no
 * contraction,
 *   dz = X_i.z - Y_j.z, dy = X_i.y - Y_j.y, dx = X_i.x - Y_j.x,
 *   d2 = (dz*dz + dy*dy) + dx*dx <= r2.
 *   index[i]  = the candidate j that minimises (d2, j) lexicographically -- a tie
 *               in distance goes to the LOWEST target row --, -1 when there is none
 *   sqdist[i] = that d2, +inf when index[i] = -1
 * A query with a NaN or Inf coordinate gets -1 / +inf; such a target is never a
 * candidate.  Three steps, all stream-ordered, no host synchronisation, no
 * allocation:
 *   pcm_nearest_keys  fills info (device int64[PCM_NEAREST_INFO_WORDS]) from the
 *                     box over the finite rows of BOTH clouds and writes xkeys
 *                     (device int64[n]) and ykeys (device int64[m]) against the
 *                     same cells: 21 bits per axis, x fastest; 2^63 - 1 for a
 *                     non-finite row;
 *   (the caller sorts each key array: sorted ascending and its permutation,
 *    sorted[i] = keys[perm[i]] -- any sort, ties in any order)
 *   pcm_nearest_find  gathers the cell-sorted copy of Y (planes z, y, x, the row
 *                     numbers, the int32 groups) into the workspace
 *                     (pcm_nearest_workspace(m) bytes) and scans: a wave takes 64
 *                     consecutive sorted queries, read as X[xperm[i]]; writes
 *                     index (device int32[n]) and sqdist (device float32[n]) in
 *                     the caller's row order.
 * info: [0] the cell exponent s (support's rule: the smallest s with 2^s >=
 * radius (1 + 2^-20), at least -32, raised until |x| 2^-s <= 2^40 and every axis
 * spans at most 2^21 cells); [1..3] the cell of the box's low corner (z, y, x);
 * [4..6] the bits each axis needs; [7] the queries skipped as non-finite; [8] the
 * targets skipped as non-finite; [9..15] internal; [16] set when xperm or yperm
 * held a value outside its range (that query is left unwritten, that target is
 * never a candidate).
 * The results are decided by the predicate and the tie rule alone -- the cells
 * only prune -- so they are the same bits for any row order, sort and launch
 * shape.  Cost: a query is tested against every target of the cells around it,
 * so the work grows with the PRODUCT of the cells' populations.  A cell run
 * longer than PCM_NEAREST_CHUNK rows is staged in several chunks.
 * PCM_NEAREST_PHASE=1 / 2 in the environment runs only the gather / only the
 * scan (measurement).
 * The arguments are checked before any device call (PCM_E_ARG: n or m < 0 or
 * >= 2^31, a radius or radius squared not finite or <= 0, one of groups /
 * target_groups without the other, a null pointer with n or m > 0, a workspace
 * too small).  n = 0 makes no device call in pcm_nearest_find; m = 0 writes
 * -1 / +inf for every query without a scan. */
#define PCM_NEAREST_CHUNK 128
#define PCM_NEAREST_TPB 256
#define PCM_NEAREST_INFO_WORDS 20
int pcm_nearest_workspace(int64_t m, size_t *bytes);
int pcm_nearest_keys(const float *X, int64_t n, const float *Y, int64_t m, float radius, int64_t *xkeys, int64_t *ykeys,
                     int64_t *info, void *stream);
int pcm_nearest_find(const float *X, int64_t n, const float *Y, int64_t m, const int32_t *groups /* nullable */,
                     const int32_t *target_groups /* nullable */, float radius, const int64_t *xkeys_sorted,
                     const int64_t *xperm, const int64_t *ykeys_sorted, const int64_t *yperm, int32_t *index,
                     float *sqdist, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- local moments
 * Exact per-point neighbourhood moments and the plane through a point's
 * neighbours (no reference counterpart; DESIGN.md §4 "Local moments").  Queries
 * X (n rows) and targets Y (m rows): device float32 rows (z, y, x).  Target j is
 * in the neighbourhood of query i iff both rows are finite and the predicate of
 * the nearest section holds (d2 <= r2, float32, no contraction): no groups, no
 * self-exclusion.  With q (host int32[3], each in [-126, 62]),
 *   yq_a = trunc(ldexp(Y_j.a, q_a)), xq_a = trunc(ldexp(X_i.a, q_a)), dq_a = yq_a - xq_a
 * and words (device int64[n * PCM_MOMENTS_WORDS], row-major) receives per query
 *   [0] the count   [1..3] sum dq_z, dq_y, dq_x
 *   [4..9] sum dq_a dq_b for (zz, zy, zx, yy, yx, xx).
 * Integer sums: the same bits for any row order, sort and launch shape.  A
 * non-finite query gets ten zeros; a non-finite target is in no neighbourhood.
 * The kernel checks nothing per pair: the CALLER chooses q so that, with
 * B_a = floor((double)radius (1 + 2^-20) 2^q_a) + 1 (>= |dq_a| of every pair the
 * predicate admits), B_a < 2^31, max(m, 1) B_a B_b <= 2^62 and |coordinate_a|
 * 2^q_a < 2^31 over the finite rows of both clouds.  Steps, all stream-ordered,
 * no host synchronisation, no allocation:
 *   pcm_nearest_keys  (above) fills info and the keys of both clouds;
 *   (the caller sorts each key array, as for pcm_nearest_find)
 *   pcm_moments_scan  gathers the cell-sorted copy of Y (three float planes and
 *                     the three int32 fixed-point planes) into the workspace
 *                     (pcm_moments_workspace(m) bytes) and scans as
 *                     pcm_nearest_find does: a wave takes 64 consecutive sorted
 *                     queries, read as X[xperm[i]], and stages the candidates
 *                     through LDS in chunks of PCM_MOMENTS_CHUNK rows.  info is
 *                     the block pcm_nearest_keys filled (layout above); a value
 *                     of xperm or yperm outside its range sets info[16].
 *                     Y == NULL: the targets are the queries -- m, ykeys_sorted
 *                     and yperm are ignored (the queries' arrays serve), the
 *                     workspace is pcm_moments_workspace(n) bytes, and info comes
 *                     from pcm_nearest_keys(X, n, NULL, 0, ...): the targets
 *                     skipped are the queries skipped.
 *   pcm_moments_planes  one lane per row, float64: c = words[0],
 *                     mu_a = S_a 2^-q_a / c, C_ab = M_ab 2^-(q_a + q_b) / c - mu_a mu_b,
 *                     eigen-decomposition by cyclic Jacobi (until the
 *                     off-diagonals are zero, at most 8 sweeps);
 *                     normal (device float32[n * 3]) the unit eigenvector of the
 *                     smallest eigenvalue, signed z >= 0, ties by y then x (a
 *                     component within 2^-30 of 0 is set to 0 first, so that the
 *                     rounding noise of a vertical plane's z picks no sign);
 *                     roughness = sqrt(max(l0, 0)); planarity = (l1 - l0) / l2,
 *                     0 where l2 <= 0; distance = -normal . mu, the signed
 *                     distance of the query to the plane through the
 *                     neighbourhood's mean (device float32[n] each).  Rows with
 *                     count < max(min_count, 1) get NaN.
 * PCM_MOMENTS_PHASE=1 / 2 in the environment runs only the gather / only the
 * scan (measurement).  Cost: as for nearest, the work grows with the PRODUCT of
 * the cells' populations.
 * The arguments are checked before any device call (PCM_E_ARG: n or m < 0 or
 * >= 2^31, a radius or radius squared not finite or <= 0, q null or outside
 * [-126, 62], min_count < 0, a null pointer, a workspace too small).  n = 0
 * makes no device call; m = 0 (Y not NULL) zeroes words without a scan. */
#define PCM_MOMENTS_CHUNK 128
#define PCM_MOMENTS_TPB 256
#define PCM_MOMENTS_WORDS 10
int pcm_moments_workspace(int64_t m, size_t *bytes);
int pcm_moments_scan(const float *X, int64_t n, const float *Y /* nullable: the queries */, int64_t m, float radius,
                     const int32_t *q /* host int32[3] */, const int64_t *xkeys_sorted, const int64_t *xperm,
                     const int64_t *ykeys_sorted, const int64_t *yperm, int64_t *words, int64_t *info, void *workspace,
                     size_t workspace_bytes, void *stream);
int pcm_moments_planes(const int64_t *words, int64_t n, const int32_t *q /* host int32[3] */, int64_t min_count,
                       float *normal, float *distance, float *roughness, float *planarity, void *stream);

/* ---------------------------------------------------------------- slab sharding
 * Multi-GPU layout (no reference counterpart -- the reference is
 * single-process): the row shards the ranks receive are regrouped into slabs
 * of the longest axis so that each rank's pruning grid covers only its slab.
 * X: device n*d rows (dtype PCM_F32/PCM_F16) whose global row index is gidx0 + i.
 * bin(x) = clamp(floor((x[axis] - lo) * inv), 0, nbins - 1), computed in fp64.
 *   pcm_shard_hist       hist[nbins] (device uint64, overwritten), nbins <= 16384;
 *   pcm_shard_partition  stable partition by owner[bin] (device uint8[nbins],
 *                        values < P): X_out (device n*d) holds the rows grouped
 *                        by destination rank in original order, rows_out
 *                        (device uint32[n]) their global indices, counts (host
 *                        int64[P]) the group sizes; synchronises `stream`;
 *   pcm_shard_scatter_labels  out[rows[i] - gidx0] = labels[i] (device int32):
 *                        labels returned in the partition's order -> row order. */
#define PCM_SHARD_MAXP 16
int pcm_shard_hist(const void *X, int dtype, int64_t n, int d, int axis, double lo, double inv, int nbins,
                   uint64_t *hist, void *stream);
int pcm_shard_partition_workspace(int64_t n, int P, size_t *bytes);
int pcm_shard_partition(const void *X, int dtype, int64_t n, int d, int axis, double lo, double inv, int nbins,
                        const uint8_t *owner, int P, int64_t gidx0, void *X_out, uint32_t *rows_out, int64_t *counts,
                        void *workspace, size_t workspace_bytes, void *stream);
int pcm_shard_scatter_labels(const int32_t *labels, const uint32_t *rows, int64_t n, int64_t gidx0, int32_t *out,
                             void *stream);

/* ---------------------------------------------------------------- peer exchange
 * One-sided SUM of the per-iteration statistics over the ranks (SURVEY.md §8e;
 * no reference counterpart -- the reference is single-process): it replaces the
 * RCCL all-reduce between pcm_iter_local and pcm_iter_global by writes into the
 * peers' memory.  Each rank creates one exchange of `words` int64 (pcm_stats_ptr's
 * count); its receive buffer (2 x P slots + flags, uncached device memory) is made
 * reachable to the other ranks by pcm_xchg_handle -> pcm_xchg_open (another
 * process: IPC) or pcm_xchg_link (an exchange of the same process).  Every rank
 * must run the same sequence of exchanges.
 *   pcm_xchg_allreduce  buf (device uint64[words]) := SUM over ranks, in place,
 *                       stream-ordered, no host synchronisation (graph-capturable);
 *                       phase 1 = push only, 2 = wait + sum only, 3 = both;
 *   pcm_iter_exchange   the same on the engine's statistics buffer, gated by the
 *                       engine's device control block like pcm_iter_*; a wait
 *                       longer than timeout_s sets status done = 4 (exchange
 *                       failed) and gates the rest of the fit;
 *   pcm_xchg_status     synchronises `stream`: err (1 = a wait timed out), and
 *                       the number of exchanges completed. */
#define PCM_XCHG_MAXP 16
#define PCM_XCHG_HANDLE_BYTES 64
typedef struct pcm_xchg pcm_xchg;
int pcm_xchg_create(int device, int64_t words, int nranks, int rank, double timeout_s, pcm_xchg **out);
int pcm_xchg_destroy(pcm_xchg *x);
int pcm_xchg_handle(pcm_xchg *x, void *handle /* PCM_XCHG_HANDLE_BYTES */);
int pcm_xchg_open(pcm_xchg *x, int peer, const void *handle);
int pcm_xchg_link(pcm_xchg *x, int peer, pcm_xchg *other);
int pcm_xchg_allreduce(pcm_xchg *x, uint64_t *buf, int phase, void *stream);
int pcm_xchg_status(pcm_xchg *x, uint32_t *err, uint64_t *epoch, void *stream);
int pcm_iter_exchange(pcm_engine *e, pcm_xchg *x, int phase, void *stream);

/* k-means++ seeding, replacing scikit-learn's _kmeans_plusplus
 * (sklearn/cluster/_kmeans.py:174-272; KMeans' default init, :1012-1019; the
 * reference's call site members/jasraj/land_use_classification/core.py:227-228)
 * with the canonical arithmetic of oracle/kpp_ref.py.  X: device float32[n*d]
 * (row order = the caller's); first_index: the first centre (sklearn's
 * random_state.choice draw, computed by the host); umant: host uint64
 * [(k-1)*n_local_trials], each uniform of random_state.uniform(size=L) for
 * centres 1..k-1 as its exact 53-bit mantissa (u * 2^53).  The weight
 * exponent is kpp_scale(n, sum_a (max_a - min_a)^2) of the device bounding box.
 * Writes indices (device int64[k]), stream-ordered; synchronises once (bounding
 * box -> pruning grid) and returns PCM_E_NONFINITE for NaN/Inf input.
 * workspace: caller-owned device memory of pcm_kmeanspp_workspace bytes. */
int pcm_kmeanspp_workspace(int64_t n, int d, int k, int n_local_trials, size_t *bytes);
int pcm_kmeanspp(const float *X, int64_t n, int d, int k, int n_local_trials, int64_t first_index,
                 const uint64_t *umant, int64_t *indices, void *workspace, size_t workspace_bytes, void *stream);

/* Per-pair point-cloud assembly, replacing the float64 NumPy block of
 * members/rafael/disparity/plugin.py:147-192 (height = -disparity/16, validity
 * mask, np.where row-major compaction, SVD plane fit oriented to +z, relative
 * height, 2/98 percentiles, points (z - h_min, y, x) + 'height' property).
 * disparity: device float64[H*W]; validity: device uint8[H*W] or NULL;
 * limit = MAX_DISP/2.  points: device float64[3*H*W] capacity, hnorm:
 * device float64[H*W] capacity; *m_out = number of points; normal_out (host
 * double[3], nullable) = the fitted plane normal.  Synchronises the stream. */
int pcm_cloud_assemble(const double *disparity, const uint8_t *validity, int64_t H, int64_t W, double limit,
                       double *points, double *hnorm, int64_t *m_out, double *normal_out, void *stream);

/* ---------------------------------------------------------------- stereo gathers
 * Per-pixel consistency maps of a rectified pair (H x W, row-major, device):
 * pcm_photoconsistency replaces members/rafael/disparity/processing.py:94-115
 * photoconsistency_map (left/right images PCM_F32 or PCM_F64, left_disp
 * float64 = disparity / 16; out float64 |right[y, rint(x - d)] - left[y, x]| / 255,
 * 0 where undefined); pcm_lr_consistency replaces disparity.py:229-250
 * left_right_consistency (out float64 |rd[y, rint(x - d)] + ld[y, x]|, max_disp
 * where undefined; below (nullable) uint8 = out < threshold, the caller's
 * `< 3` of disparity.py:170-172; out may be NULL when only the mask is
 * wanted).  Undefined: d NaN, rint(x - d) outside [0, W), or d < min_disp.
 * Stream-ordered, no synchronisation. */
int pcm_photoconsistency(const void *left, const void *right, int img_dtype, const double *left_disp, int64_t H,
                         int64_t W, double min_disp, double *out, void *stream);
int pcm_lr_consistency(const double *left_disp, const double *right_disp, int64_t H, int64_t W, double min_disp,
                       double max_disp, double *out, uint8_t *below, double threshold, void *stream);

/* ---------------------------------------------------------------- dense path
 * Generic-D Lloyd K-means for feature vectors (D <= PCM_DENSE_DMAX, float32 or
 * float64, computed in that precision), replacing one _kmeans_single_lloyd
 * call (sklearn/cluster/_kmeans.py:623-752) at the reference's KMeans call site
 * members/jasraj/land_use_classification/core.py:227-228 (~1500 x 20 float64).
 * Brute force over all K with the centres staged in LDS when k*d*sizeof <= 64 KB (else read from L2);
 * canonical arithmetic of oracle/dense_ref.py; everything on the device, one
 * process (no sharding).  X (device, n*d, row-major) must stay valid and
 * unchanged from pcm_dense_begin to the last call of the fit.  maxabs (host
 * double[d]) = max |X[:, a]| fixes the exact fixed-point sums. */
typedef struct pcm_dense pcm_dense;
int pcm_dense_create(int device, int64_t n, int d, int k, int dtype, int max_iter, pcm_dense **out);
int pcm_dense_destroy(pcm_dense *e);
/* centres C0: device k*d of dtype; labels := -1, history cleared (synchronises). */
int pcm_dense_begin(pcm_dense *e, const void *X, const double *maxabs, const void *C0, double tol, int max_iter,
                    void *stream);
/* n_iter Lloyd iterations (E-step + update), gated on the device after convergence. */
int pcm_dense_iterate(pcm_dense *e, int n_iter, void *stream);
/* Final E-step with the final centres: labels + exact inertia limbs. */
int pcm_dense_final(pcm_dense *e, void *stream);
/* Status (synchronises): done/iter/last_*, inertia; list_rebuilds = relocation events. */
int pcm_dense_status(pcm_dense *e, pcm_status *out, void *stream);
/* Outputs (synchronises): labels device int32[n], centres device k*d dtype,
 * history host uint64/double[cap]; any pointer may be NULL. */
int pcm_dense_outputs(pcm_dense *e, int32_t *labels, void *centers, uint64_t *changed, double *shift, int cap,
                      void *stream);
/* k-means++ for the dense path (oracle/kpp_ref.py canonical seeding in the
 * input precision), brute force; scale = kpp_scale(n, max distance bound). */
int pcm_dense_kmeanspp_workspace(int64_t n, int d, int dtype, int k, int n_local_trials, size_t *bytes);
int pcm_dense_kmeanspp(const void *X, int64_t n, int d, int dtype, int k, int n_local_trials, int64_t first_index,
                       const uint64_t *umant, int scale, int64_t *indices, void *workspace, size_t workspace_bytes,
                       void *stream);

/* Stateless E-step of the dense path for given centres (no pcm_dense object, no
 * fit state): labels device int32[n]; dist (nullable) device n of dtype, the
 * canonical squared distance to the assigned centre; inertia (nullable, host):
 * exact limbs, scale from maxabs (host double[d]) = max |.| per feature over
 * the rows of X AND C (needed only with inertia).  workspace: device memory of
 * at least PCM_DENSE_PREDICT_WS bytes.  Synchronises when inertia is given.
 * The kernel is the fit's E-step: it reads labels[i] before it writes it, to
 * count changed labels (the count goes to the workspace and is not used), so
 * labels must be readable memory; its content on entry does not matter. */
#define PCM_DENSE_PREDICT_WS 256
int pcm_dense_predict(const void *X, int dtype, int64_t n, int d, const void *C, int k, const double *maxabs,
                      int32_t *labels, void *dist, pcm_inertia *inertia, void *workspace, size_t workspace_bytes,
                      void *stream);
/* sklearn KMeans.transform (_kmeans.py:1135-1161): out (device n*k of dtype,
 * row-major) = sqrt of the canonical squared distance of row i to centre j,
 * correctly rounded in dtype.  Stream-ordered, no synchronisation. */
int pcm_dense_transform(const void *X, int dtype, int64_t n, int d, const void *C, int k, void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCM_KMEANS_H */
