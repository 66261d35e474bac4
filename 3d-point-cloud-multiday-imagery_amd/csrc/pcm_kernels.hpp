// pcm_kernels.hpp — gfx950 kernels of the multi-day point-cloud Lloyd engine.
//
// Hot path: per iteration
//   k_cand             exact candidate lists per grid cell (fp64 bisector bound)
//   k_lloyd1           nearest centroid over the cell's candidates + LDS-privatised
//                      fixed-point accumulation (replaces _k_means_lloyd.pyx:168-218)
//   k_label            final E-step: labels + inertia (_kmeans.py:736-750)
//   k_upd / k_upd1 / k_updlists (k_resume after a relocation)
//                      averaging / shift / convergence (_k_means_common.pyx:274-311,
//                      _kmeans.py:717-732)
// Layout (once per cloud): k_bbox*, the record sort of pcm_sort.hpp (cell
// order, AoSoA-4), k_cell_starts_xs, k_tiles.
//
// Canonical arithmetic (oracle/lloyd_ref.py): fp32 distance
// ((d0*d0 + d1*d1) + d2*d2) + d3*d3 with every op rounded (-ffp-contract=off),
// strict '<' scan in ascending centroid index, int64 fixed-point sums.
#pragma once
#include "pcm_kcommon.hpp"   // Grid, Ctrl, arrival helpers, QExp, dist_canon, box / prunable geometry
#include "pcm_layout.hpp"    // zero spans, bbox, sort key, tiles, compression, tile lists
#include "pcm_cand.hpp"      // cand_body, k_cand, k_coarse, refresh_body
#include "pcm_assign.hpp"    // scans, point loads, AccL, LloydArgs, k_label, k_lloyd1
#include "pcm_update.hpp"    // k_upd, k_upd1, k_lists, k_updlists, k_resume
#include "pcm_util.hpp"      // relocation, unpermute, centres in/out, synth, stats, k_bruteforce, k_predict
