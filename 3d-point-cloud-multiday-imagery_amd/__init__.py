"""MI355X-native multi-day point-cloud K-means (Lloyd) reconstruction step.

Drop-in for the K-means step of the ``members/rafael`` "Multi-day 3D Point
Cloud" plugin (see DESIGN.md / INTEGRATION.md).  Import name: ``pcm_amd``
(the repository-root shim ``pcm_amd.py`` maps it onto this directory).

Public API
----------
lloyd_fit(X, centers_init, max_iter, tol, group=None)  -> LloydResult
kmeans_plusplus(X, n_clusters, random_state=...)       -> (centers, indices), GPU k-means++
assemble_cloud(disparity, validity, max_disp=288)      -> per-pair (z,y,x) cloud + height property (GPU)
KMeans(n_clusters, init, n_init, ...).fit_predict(X)   -> the reference's KMeans call site (core.py:227-228)
dense_fit / dense_kmeanspp                             -> generic-D (float32/float64) Lloyd + k-means++ (GPU)
photoconsistency_map / left_right_consistency          -> stereo consistency gathers (GPU, processing.py / disparity.py)
lloyd_predict(X, centers, return_distance=, return_inertia=) -> LloydPrediction: labels of new points, no refit
KMeans.predict / transform / fit_transform / score     -> sklearn's API for applying a fitted model
dense_predict / dense_transform                        -> generic-D E-step and (n, K) distances for given centres
kmeans_fuse(clouds, n_clusters, ...)                   -> napari layer tuples
kmeans_assign(clouds, model)                           -> a later day's cloud labelled against a fused model
cluster_stats(X, labels, n_clusters, groups=...)       -> ClusterStats: exact per-(day, cluster) counts, sums, second moments
surface_elements(stats)                                -> per-cluster normal, roughness, planarity, rms (host, from the moments)
height_grid(X, shape, cell_log2=, labels=, groups=...) -> HeightGrid: exact per-(day, pixel) count, height sum, top and bottom
align_stats(X, centers, groups=, transforms=, max_dist=) -> AlignStats: exact per-day sums of the points and their nearest centres
register_days(X, centers, groups=, kind="rigid")       -> Registration: each day's z offset, translation or rigid motion onto the centres
apply_registration(X, registration, groups=)           -> the cloud in the centres' frame (the pass's own float32 arithmetic)
radius_support(X, radius, groups=, max_count=)         -> Support: exact per-row neighbour counts and day support within a radius
filter_outliers(X, radius, min_neighbors, min_days=)   -> bool keep mask: the radius outlier filter (speckle removal)
voxel_grid(X, voxel, origin=, groups=, q=)             -> Voxels: exact per-voxel count, centroid sums, lowest row and day mask
voxel_downsample(X, voxel, mode=, min_count=, min_days=) -> Downsampled: one point per occupied voxel (thinning, persistence filter)
nearest_points(X, Y, max_dist, groups=, target_groups=) -> Nearest: exact nearest row of another cloud within a radius, its squared distance
local_moments(X, radius, targets=, q=)                 -> LocalMoments: exact per-row count, offset sums and second moments of the rows within a radius
point_normals(X, radius, targets=, min_count=)         -> PointNormals: per-row plane normal, point-to-plane distance, roughness, planarity
HeightMapExtractor                                     -> SatellitePlugin drop-in
Engine                                                 -> the C-ABI engine wrapper
"""
from .fixed import QBITS, fixed_q  # noqa: F401
from .lloyd import LloydResult, lloyd_fit  # noqa: F401

__all__ = ["lloyd_fit", "LloydResult", "fixed_q", "QBITS", "Engine", "kmeans_fuse", "HeightMapExtractor",
           "build_library", "kmeans_plusplus", "assemble_cloud", "KMeans", "dense_fit", "dense_kmeanspp",
           "photoconsistency_map", "left_right_consistency", "lloyd_predict", "LloydPrediction", "dense_predict",
           "dense_transform", "DensePrediction", "kmeans_assign", "cluster_stats", "ClusterStats", "surface_elements",
           "SurfaceElements", "height_grid", "HeightGrid", "align_stats", "AlignStats", "register_days", "Registration",
           "apply_registration", "radius_support", "filter_outliers", "Support", "voxel_grid",
           "voxel_downsample", "Voxels", "Downsampled", "nearest_points", "Nearest",
           "local_moments", "point_normals", "LocalMoments", "PointNormals"]


def __getattr__(name):
    # lazy: the engine needs torch + the HIP library, the plugin needs neither at import
    if name == "Engine":
        from .engine import Engine
        return Engine
    if name in ("kmeans_fuse", "kmeans_assign", "HeightMapExtractor", "PREFIX"):
        from . import plugin
        return getattr(plugin, name)
    if name in ("lloyd_predict", "LloydPrediction"):
        from . import predict
        return getattr(predict, name)
    if name in ("cluster_stats", "ClusterStats", "surface_elements", "SurfaceElements"):
        from . import stats
        return getattr(stats, name)
    if name in ("height_grid", "HeightGrid"):
        from . import grid
        return getattr(grid, name)
    if name in ("align_stats", "AlignStats", "AlignPlan", "register_days", "Registration", "apply_registration"):
        from . import align
        return getattr(align, name)
    if name in ("radius_support", "filter_outliers", "Support"):
        from . import support
        return getattr(support, name)
    if name in ("voxel_grid", "voxel_downsample", "Voxels", "Downsampled"):
        from . import voxel
        return getattr(voxel, name)
    if name in ("nearest_points", "Nearest"):
        from . import nearest
        return getattr(nearest, name)
    if name in ("local_moments", "point_normals", "LocalMoments", "PointNormals"):
        from . import moments
        return getattr(moments, name)
    if name == "KMeans":
        from .estimator import KMeans
        return KMeans
    if name == "assemble_cloud":
        from .cloud import assemble_cloud
        return assemble_cloud
    if name in ("dense_fit", "dense_kmeanspp", "dense_predict", "dense_transform", "DensePrediction"):
        from . import dense
        return getattr(dense, name)
    if name in ("photoconsistency_map", "left_right_consistency"):
        from . import stereo
        return getattr(stereo, name)
    if name == "kmeans_plusplus":
        from .kpp import kmeans_plusplus
        return kmeans_plusplus
    if name == "build_library":
        from ._lib import build
        return build
    raise AttributeError(name)
