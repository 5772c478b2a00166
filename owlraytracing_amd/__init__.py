"""MI355X-native TrueKNN / RT-DBSCAN neighbour-query path behind the OWL C-ABI.

The compute path is the HIP library built from ``owlraytracing_amd/csrc`` (see ``_lib``); this
package is the thin host side above its C-ABI.  Importing the package does not load the library;
the first call that needs it does, and raises if it has not been built.
"""
__version__ = "0.1.0"


def fps(points, batch=None, ratio=0.5, **kw):
    """Farthest point sampling per cloud, torch-cluster's ``fps(x, batch, ratio)`` (trueknn.fps; loads the library)."""
    from .trueknn import fps as _fps

    return _fps(points, batch=batch, ratio=ratio, **kw)


def radius_nms(points, radius, scores=None, batch=None, **kw):
    """Greedy suppression within a radius per cloud: no two kept points within ``radius`` (trueknn.radius_nms; loads the library)."""
    from .trueknn import radius_nms as _radius_nms

    return _radius_nms(points, radius, scores=scores, batch=batch, **kw)


def voxel_down_sample(points, voxel_size, **kw):
    """Voxel-grid downsampling per cloud: one point per occupied grid cell -- centroid, first row, nearest row or cell centre --,
    values averaged with it (trueknn.voxel_down_sample; loads the library)."""
    from .trueknn import voxel_down_sample as _voxel_down_sample

    return _voxel_down_sample(points, voxel_size, **kw)


def radius_reduce(points, queries, radius, **kw):
    """Counts, kernel-weight sums and weighted value sums over the points within ``radius`` of each query, no neighbour lists
    written (trueknn.radius_reduce; loads the library)."""
    from .trueknn import radius_reduce as _radius_reduce

    return _radius_reduce(points, queries, radius, **kw)


def local_pca(points, queries, radius=None, k=None, **kw):
    """Count, centroid, covariance, eigenvalues, eigenvectors, normal and surface variation of each query's neighbourhood (a
    radius, the k nearest, or both), no neighbour lists written (trueknn.local_pca; loads the library)."""
    from .trueknn import local_pca as _local_pca

    return _local_pca(points, queries, radius=radius, k=k, **kw)


def fpfh(points, radius, normals=None, **kw):
    """The 33-bin Fast Point Feature Histogram of every point from its normal and its neighbours' within ``radius``, no neighbour lists
    written (trueknn.fpfh; loads the library)."""
    from .trueknn import fpfh as _fpfh

    return _fpfh(points, radius, normals=normals, **kw)


def orient_normals(points, normals, **kw):
    """One consistent sign per normal with no viewpoint: Hoppe's propagation along the minimum spanning tree of the kNN graph weighted
    by 1 - |n_i . n_j|, Open3D's ``orient_normals_consistent_tangent_plane`` (trueknn.orient_normals; loads the library)."""
    from .trueknn import orient_normals as _orient_normals

    return _orient_normals(points, normals, **kw)


def segment_plane(points, distance_threshold, **kw):
    """The dominant plane of a cloud by RANSAC on the device, every hypothesis scored through the box pyramid: Open3D's
    ``segment_plane``, PCL's ``SACSegmentation`` with a plane model (trueknn.segment_plane; loads the library)."""
    from .trueknn import segment_plane as _segment_plane

    return _segment_plane(points, distance_threshold, **kw)


def icp(target, source, max_dist, **kw):
    """Rigid registration of ``source`` to ``target`` by iterated closest points, point-to-point or point-to-plane, the loop and
    its fp64 sums inside the library (trueknn.icp; loads the library)."""
    from .trueknn import icp as _icp

    return _icp(target, source, max_dist, **kw)


def match_features(source_feat, target_feat, **kw):
    """Nearest and second-nearest target descriptor of every source descriptor, D <= 64, by brute force in literal fp32, with the
    mutual and ratio filters (trueknn.match_features; loads the library)."""
    from .trueknn import match_features as _match_features

    return _match_features(source_feat, target_feat, **kw)


def ransac(source, target, pairs, max_dist, **kw):
    """RANSAC over correspondences on the device: the rigid transform most pairs agree with, refitted to its inliers
    (trueknn.ransac; loads the library)."""
    from .trueknn import ransac as _ransac

    return _ransac(source, target, pairs, max_dist, **kw)


def global_registration(target, source, feature_radius, max_dist, **kw):
    """Two unaligned clouds registered on the device from end to end: normals, FPFH, feature matching, RANSAC and ICP
    (trueknn.global_registration; loads the library)."""
    from .trueknn import global_registration as _global_registration

    return _global_registration(target, source, feature_radius, max_dist, **kw)


def mean_shift(points, bandwidth, seeds=None, **kw):
    """Mean-shift clustering, sklearn's ``MeanShift``: the trajectories on the GPU inside the library, modes merged within a radius,
    every point labelled by its nearest centre (trueknn.mean_shift; loads the library)."""
    from .trueknn import mean_shift as _mean_shift

    return _mean_shift(points, bandwidth, seeds=seeds, **kw)


def bin_seeds(points, bin_size, min_bin_freq=1):
    """sklearn's ``get_bin_seeds`` on the device: the grid cells of ``bin_size`` holding at least ``min_bin_freq`` points, as seeds
    (trueknn.bin_seeds)."""
    from .trueknn import bin_seeds as _bin_seeds

    return _bin_seeds(points, bin_size, min_bin_freq)
