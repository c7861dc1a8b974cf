"""LiDARDataset (dataset/lidar_dataset.py) on the device: point-cloud files and poses in, training-sample pools out.

    from shine_mapping_amd.dataset import LiDARDataset      # instead of: from dataset.lidar_dataset import LiDARDataset
    dataset = LiDARDataset(config, octree)
    for frame_id in ...:
        dataset.process_frame(frame_id, incremental_on=False)
    coord, sdf_label, origin, ts, normal_label, sem_label, weight = dataset.get_batch()

Same constructor arguments, attributes and methods as the reference class; no open3d, natsort or pyquaternion.  A frame runs
    read (.bin / .ply) -> shine_frame_filter (z, range, crop box; fp64) -> evaluation.voxel_down_sample or a seeded random subset
    -> pose transform (fp64) -> map copy (voxel means, boxes) -> scale, fp32 -> shine_ray_sample (ONE launch, written straight
    into the pools) -> FeatureOctree.update -> pool replace / shine_pool_window_filter + append
on the device (csrc/shine_frame.hip).  Differences from the reference, all deliberate:
  * the samples come from a counter-based generator keyed by (config.seed, frame id, sample), not from torch's global stream: a
    run is reproducible whatever else draws random numbers;
  * voxel-down-sampled clouds are in ascending voxel-key order (open3d's order is that of a hash map);
  * `rand_downsample` keeps exactly int(n * rand_down_r) points (open3d keeps the first int(n * r) of a shuffle: the same count);
  * batch-mode pools grow in capacity-doubling buffers; the `*_pool` attributes are views of the used part and are REPLACED by
    every process_frame (do not keep them across frames);
  * in incremental mode without `ray_loss` the two depth pools stay empty (nothing reads them);
  * `.pcd` files, `sapce_carving_sample` and `behind_dropoff_on` are refused, and so are `semantic_on` without `config.label_path`
    (there is nothing to read labels from) and `filter_noise` / `estimate_normal` without their parameters (below).

With `config.estimate_normal` (+ `normal_radius_m`, `normal_max_nn`) and `config.filter_noise` (+ `sor_nn`, `sor_std`) a frame is
cleaned as the reference cleans it with open3d (dataset/lidar_dataset.py:144-164; csrc/shine_frame_nn.hip):
    filter and crop -> estimate_normals on the cropped cloud -> down-sampling (the normals as attribute columns of the voxel means,
    NOT re-normalised, or the same random subset) -> statistical_outlier_mask on the down-sampled cloud (points, classes and
    normals alike) -> pose transform (normals: R n, no translation, no scale, then the cast) -> ... -> the `normal_label` pool,
    [m * S, 3], row i * S + j = the normal of ray i (dataSampler.sample's repeat + transpose), which follows every path the other
    pools take -> get_batch returns normal_label for coord's rows (None without estimate_normal).
`knn`, `statistical_outlier_mask` and `estimate_normals` are plain functions on device tensors; their docstrings restate the
open3d functions.  Deliberate difference: open3d leaves a normal's SIGN to its eigen solver; here every normal faces the sensor.
`sor_nn` and `normal_max_nn` must lie in 1..32.

With `config.semantic_on` and `config.label_path` a frame also carries a class per point (dataset/lidar_dataset.py:132-136, 166-173,
197-199, 301-362):
    read (.bin + label_path/<name with 'bin' -> 'label'>, uint32) -> shine_sem_frame_filter (range, moving, outlier, learning map,
    crop box; ONE launch) -> voxel means with class / 255 carried as an attribute (shine_voxel_down_attr), class = rint(mean * 255)
    — the reference's detour through open3d's colour channel — or the seeded subset applied to points and classes alike
    -> pose transform -> map copy with the class colours averaged per map voxel -> shine_ray_sample(labels=class) into the int32
    `sem_label` pool, which the window filter compacts with the others -> get_batch returns sem_label (int64).
The label definition comes from semantic_kitti.LabelMap.from_config(config).  Differences / quirks kept:
  * the reference calls preprocess_sem_kitti(points, labels, config.min_z, config.min_range, ...) positionally into the parameters
    (min_range, filter_outlier): the RANGE cut is config.min_z (usually negative: no cut) and the outlier filter is on iff
    config.min_range is non-zero.  Reproduced as it is, so that a config gives the points the reference would have kept;
  * the semantic path never applies preprocess_kitti's `z > min_z`: only the crop box (inclusive) bounds z;
  * a voxel's class is the rounded MEAN of its points' classes (round-half-to-even), not a vote: a voxel holding classes 3 and 4
    becomes class 4, one holding 2, 9 and 9 becomes class 7.  Kept, as the reference trains on exactly these labels;
  * ray mode gathers `sem_label_pool[ray_index * ray_sample_count]`: the label of the ray's first surface sample, one per ray;
  * a raw id the label map does not hold raises ValueError (the reference: KeyError) if it survives the label filters.
"""
from __future__ import annotations

import csv
import ctypes as C
import os
import re

import numpy as np
import torch

from . import _lib
from . import evaluation as ev

_U64 = (1 << 64) - 1
UNSUPPORTED = ("estimate_normal", "filter_noise", "semantic_on", "behind_dropoff_on")
# the frame options that are served once the config carries their parameters (utils/config.py: sor_nn 25, sor_std 2.5,
# normal_radius_m 0.2, normal_max_nn 20)
OPTION_PARAMS = {"filter_noise": ("sor_nn", "sor_std"), "estimate_normal": ("normal_radius_m", "normal_max_nn")}
SEMANTIC_NEEDS = " (frame-level label files and the learning map are not read without config.label_path; ray_sample itself takes labels)"


def natural_key(name):
    """sort key that orders file names as 1, 2, ... 9, 10 (natsort's default for plain names)"""
    return [int(t) if t.isdigit() else t.lower() for t in re.split(r"(\d+)", name)]


def _rows_to_pose(values):
    pose = np.zeros((4, 4))
    pose[0, 0:4] = values[0:4]
    pose[1, 0:4] = values[4:8]
    pose[2, 0:4] = values[8:12]
    pose[3, 3] = 1.0
    return pose


def read_calib_file(filename):
    """KITTI calib.txt: {key: 4x4} (utils/pose.py:7-30)"""
    calib = {}
    with open(filename) as fh:
        for line in fh:
            if not line.strip():
                continue
            key, content = line.strip().split(":")
            calib[key] = _rows_to_pose([float(v) for v in content.strip().split()])
    return calib


def read_poses_file(filename, calibration):
    """KITTI poses.txt: the lidar pose in the world frame, Tr^-1 . P . Tr per line (utils/pose.py:33-58)"""
    Tr = calibration["Tr"]
    Tr_inv = np.linalg.inv(Tr)
    poses = []
    with open(filename) as fh:
        for line in fh:
            if not line.strip():
                continue
            pose = _rows_to_pose([float(v) for v in line.strip().split()])
            poses.append(np.matmul(Tr_inv, np.matmul(pose, Tr)))
    return poses


def quaternion_rotation_matrix(w, x, y, z):
    """rotation matrix of the quaternion (w, x, y, z), normalised first (pyquaternion's Quaternion.rotation_matrix)"""
    n = np.sqrt(w * w + x * x + y * y + z * z)
    if n > 0:
        w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def csv_odom_to_transforms(path):
    """tx,ty,tz,qx,qy,qz,qw CSV (utils/pose.py:61-87).  The reference hands the four values to Quaternion(array) in the order
    qx, qy, qz, qw, and that constructor reads a 4-array as (w, x, y, z): the column named qx is used as w, qy as x, qz as y
    and qw as z.  Kept as it is, so that a driver sees the poses the reference would have produced from the same file."""
    poses = []
    with open(path, mode="r") as fh:
        reader = csv.reader(fh)
        header = next(reader)
        header[0] = "ts"
        for row in reader:
            if not row:
                continue
            odom = {l: row[i] for i, l in enumerate(header)}
            q = [float(odom[l]) for l in ("qx", "qy", "qz", "qw")]
            tf = np.eye(4)
            tf[0:3, 3] = [float(odom[l]) for l in ("tx", "ty", "tz")]
            tf[0:3, 0:3] = quaternion_rotation_matrix(q[0], q[1], q[2], q[3])
            poses.append(tf)
    return poses


class BoundingBox:
    """what Mesher.recon_bbx_mesh takes: get_min_bound() / get_max_bound() (numpy fp64 [3]); empty until the first extend"""

    def __init__(self, min_bound=None, max_bound=None):
        self.min_bound = None if min_bound is None else np.asarray(min_bound, dtype=np.float64).copy()
        self.max_bound = None if max_bound is None else np.asarray(max_bound, dtype=np.float64).copy()

    def is_empty(self):
        return self.min_bound is None

    def get_min_bound(self):
        return np.zeros(3) if self.min_bound is None else self.min_bound

    def get_max_bound(self):
        return np.zeros(3) if self.max_bound is None else self.max_bound

    def extend(self, lo, hi):
        if self.min_bound is None:
            self.min_bound, self.max_bound = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        else:
            self.min_bound, self.max_bound = np.minimum(self.min_bound, lo), np.maximum(self.max_bound, hi)
        return self


class PointCloud:
    """the merged map cloud: fp64 [n,3] device chunks, concatenated when `points` is read; `colors` (fp64 [n,3] in 0..1, one row
    per point) likewise, None unless every chunk came with colours"""

    def __init__(self, points=None, colors=None):
        self._chunks = [] if points is None else [points]
        self._colors = [] if points is None else [colors]

    def __iadd__(self, other):
        self._chunks += other._chunks
        self._colors += other._colors
        return self

    def __len__(self):
        return sum(int(c.shape[0]) for c in self._chunks)

    def _merge(self):
        if len(self._chunks) > 1:
            self._colors = [None if any(c is None for c in self._colors) else torch.cat(self._colors, 0)]
            self._chunks = [torch.cat(self._chunks, 0)]

    @property
    def points(self):
        self._merge()
        return self._chunks[0] if self._chunks else torch.empty((0, 3), dtype=torch.float64)

    @property
    def colors(self):
        self._merge()
        return self._colors[0] if self._colors else None

    def get_min_bound(self):
        return ev.bounds(self.points)[0]

    def get_max_bound(self):
        return ev.bounds(self.points)[1]


def frame_filter(points, min_z, max_z, min_range, pc_radius):
    """preprocess_kitti + the crop box (shine_frame_filter): points = device [n,3] / [n,4] float32 or float64, contiguous.  Keeps,
    in input order, z > min_z, |p| >= min_range, |x|, |y| <= pc_radius, min_z <= z <= max_z.  -> fp64 [k,3] on the device."""
    if not points.is_cuda:
        raise _lib.ShineHipError("frame_filter runs on the device only (there is no CPU path)")
    if points.dim() != 2 or points.shape[1] not in (3, 4) or points.dtype not in (torch.float32, torch.float64):
        raise ValueError("frame_filter: expected [n,3] or [n,4] float32 / float64 points, got %s %s" % (tuple(points.shape), points.dtype))
    points = points.contiguous()
    n = int(points.shape[0])
    out = torch.empty((n, 3), dtype=torch.float64, device=points.device)
    if n == 0:
        return out
    kept = C.c_int64(0)
    _lib.call_with_workspace(
        _lib.lib().shine_frame_filter, points.device, points.data_ptr(), n, int(points.dtype == torch.float64),
        int(points.shape[1]), float(min_z), float(max_z), float(min_range), float(pc_radius), _lib.WS, _lib.WS_BYTES,
        out.data_ptr(), C.byref(kept), _lib.current_stream_handle())
    return out[:kept.value]


def sem_frame_filter(points, labels, label_map, range_min, filter_moving, filter_outlier, min_z, max_z, pc_radius):
    """preprocess_sem_kitti + the learning map + the crop box in one launch (shine_sem_frame_filter).  points = device [n,3] / [n,4]
    float32 or float64, labels = [n] raw uint32 label words (any 4-byte or wider integer tensor / array; the lower 16 bits are
    the semantic id), label_map = semantic_kitti.LabelMap.  Keeps, in input order, |p| >= range_min, id < 100 (filter_moving),
    id != 1 (filter_outlier), |x|, |y| <= pc_radius, min_z <= z <= max_z.  -> (fp64 [k,3], int32 [k] classes) on the device.
    A raw id the map does not hold, on a point that passes the range / moving / outlier tests, raises ValueError."""
    if not points.is_cuda:
        raise _lib.ShineHipError("sem_frame_filter runs on the device only (there is no CPU path)")
    if points.dim() != 2 or points.shape[1] not in (3, 4) or points.dtype not in (torch.float32, torch.float64):
        raise ValueError("sem_frame_filter: expected [n,3] or [n,4] float32 / float64 points, got %s %s"
                         % (tuple(points.shape), points.dtype))
    points = points.contiguous()
    n = int(points.shape[0])
    if not torch.is_tensor(labels):
        labels = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).astype(np.int64)))
    if labels.numel() != n:
        raise ValueError("sem_frame_filter: %d labels for %d points" % (labels.numel(), n))
    # (torch has no uint32 arithmetic: the 32-bit pattern travels as int32, the kernel reads it unsigned)
    if labels.dtype != torch.int32:
        lab = labels.to(torch.int64) & 0xFFFFFFFF
        labels = torch.where(lab >= (1 << 31), lab - (1 << 32), lab).to(torch.int32)
    labels = labels.to(points.device).reshape(-1).contiguous()
    out = torch.empty((n, 3), dtype=torch.float64, device=points.device)
    cls = torch.empty(n, dtype=torch.int32, device=points.device)
    if n == 0:
        return out, cls
    lut = label_map.device_lut(points.device)
    kept, unknown = C.c_int64(0), C.c_int64(0)
    _lib.call_with_workspace(
        _lib.lib().shine_sem_frame_filter, points.device, points.data_ptr(), n, int(points.dtype == torch.float64),
        int(points.shape[1]), labels.data_ptr(), lut.data_ptr(), float(range_min), int(bool(filter_moving)),
        int(bool(filter_outlier)), float(min_z), float(max_z), float(pc_radius), _lib.WS, _lib.WS_BYTES, out.data_ptr(),
        cls.data_ptr(), C.byref(kept), C.byref(unknown), _lib.current_stream_handle())
    if unknown.value > 0:
        ids = labels.to(torch.int64) & 0xFFFF
        bad = torch.unique(ids[lut[ids] < 0]).tolist()  # (candidates: the kernel counted those among them that pass the filters)
        raise ValueError("sem_frame_filter: %d point(s) carry a raw label id the label map does not hold (unmapped ids in this "
                         "scan: %s)" % (unknown.value, bad))
    return out[:kept.value], cls[:kept.value]


KNN_MAX = 32  # the most neighbours per point of the frame searches (the kernel's list, csrc/shine_frame_nn.hip)


def _frame_grid(points, what):
    """the search grid over a cloud itself (evaluation.NNGrid) and its leading arguments of the csrc/shine_frame_nn.hip entry points"""
    if not torch.is_tensor(points) or not points.is_cuda:
        raise _lib.ShineHipError("%s runs on the device only (there is no CPU path)" % what)
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
        raise ValueError("%s: expected a non-empty [n,3] cloud, got %s" % (what, tuple(points.shape)))
    grid = ev.NNGrid(points)
    args = (grid.grid.data_ptr(), grid.n, grid.n_fine, grid.n_coarse, ev._d3(grid.lo), grid.cell,
            (C.c_int64 * 3)(*[int(c) for c in grid.cells_per_axis]))
    return grid, args


def _check_k(what, name, k):
    if int(k) != k or not 1 <= int(k) <= KNN_MAX:
        raise ValueError("%s: %s must be an integer in 1..%d (the per-point list of the search kernel), got %r" % (what, name, KNN_MAX, k))
    return int(k)


def knn(points, k, radius=None, return_rounds=False):
    """The k nearest points of the cloud for every point of the cloud itself (shine_knn_search): points = device [n,3] (cast to
    fp64), 1 <= k <= 32, radius = None (unbounded) or a length: only neighbours with squared distance <= radius * radius.  The
    point itself is a neighbour at distance 0 — what open3d's KDTreeFlann.search_knn_vector_3d / search_hybrid_vector_3d return
    for a point of the tree.  -> (idx int32 [n,k], -1 where there is no neighbour; d2 fp64 [n,k] squared distances, ascending,
    +inf there; count int32 [n]).  Equal distances are ordered by lower index.  The squared distance is (dx*dx + dy*dy) + dz*dz
    in fp64 without fused multiply-add: numpy's bits.  return_rounds: also the number of search launches (unbounded searches
    widen the radius for the points whose list did not fill)."""
    k = _check_k("knn", "k", k)
    if radius is not None and not float(radius) >= 0.0:
        raise ValueError("knn: radius must be None or >= 0, got %r" % (radius,))
    grid, args = _frame_grid(points, "knn")
    n, dev = grid.n, grid.ref.device
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((n, k), dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    rounds = C.c_int32(0)
    _lib.call_with_workspace(
        _lib.lib().shine_knn_search, dev, *args, k, -1.0 if radius is None else float(radius), _lib.WS, _lib.WS_BYTES,
        idx.data_ptr(), d2.data_ptr(), count.data_ptr(), C.byref(rounds), _lib.current_stream_handle())
    return (idx, d2, count, int(rounds.value)) if return_rounds else (idx, d2, count)


def statistical_outlier_mask(points, nb_neighbors, std_ratio, return_rounds=False):
    """open3d's PointCloud.remove_statistical_outlier(nb_neighbors, std_ratio) as a mask (shine_sor_mean_dist): points = device
    [n,3].  With k = nb_neighbors (1..32):
        avg_i     = mean of the distances to the min(k, n) nearest points of the cloud, the point's own 0 included (open3d's
                    SearchKNN includes it), an exact unbounded search, fp64
        mean      = sum(avg_i) / n,   std = sqrt(sum((avg_i - mean)^2) / (n - 1)),   threshold = mean + std_ratio * std
        keep_i    = avg_i > 0 and avg_i < threshold
    -> (keep bool [n], mean_dist fp64 [n] = avg, threshold float).  Both sums are added in a fixed order on the device: two
    runs give the same bits.  n == 1: open3d divides by n - 1 = 0; here std is defined as 0, so threshold = mean = 0 and the
    single point (avg = 0) is dropped — as every point is whenever k == 1.  nb_neighbors < 1 or std_ratio <= 0: ValueError, as
    open3d's."""
    if nb_neighbors < 1 or not std_ratio > 0.0:
        raise ValueError("statistical_outlier_mask: nb_neighbors must be >= 1 and std_ratio > 0 (open3d: 'Illegal input "
                         "parameters, the number of neighbors and standard deviation ratio must be positive'), got %r, %r"
                         % (nb_neighbors, std_ratio))
    k = _check_k("statistical_outlier_mask", "nb_neighbors", nb_neighbors)
    grid, args = _frame_grid(points, "statistical_outlier_mask")
    n, dev = grid.n, grid.ref.device
    avg = torch.empty(n, dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    rounds = C.c_int32(0)
    _lib.call_with_workspace(_lib.lib().shine_sor_mean_dist, dev, *args, k, _lib.WS, _lib.WS_BYTES, avg.data_ptr(),
                             stats.data_ptr(), C.byref(rounds), _lib.current_stream_handle())
    mean, ssq = (float(v) for v in stats.cpu())
    std = float(np.sqrt(ssq / (n - 1))) if n > 1 else 0.0
    threshold = mean + float(std_ratio) * std
    keep = (avg > 0.0) & (avg < threshold)
    return (keep, avg, threshold, int(rounds.value)) if return_rounds else (keep, avg, threshold)


def estimate_normals(points, radius, max_nn, viewpoint=(0.0, 0.0, 0.0)):
    """open3d's PointCloud.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (shine_frame_normals): points = device [n,3].
    Per point: its max_nn (1..32) nearest points of the cloud within `radius` (itself included); their covariance about their
    own mean, subtracted before accumulating; the unit eigenvector of the smallest eigenvalue (cyclic Jacobi, fp64); (0, 0, 1)
    where fewer than 3 neighbours are found or all of them coincide (open3d's fallback); then the flip that makes
    n . (viewpoint - p) >= 0.  -> fp64 [n,3].
    The deliberate difference from the reference: open3d leaves the SIGN to its eigen solver and the reference never calls
    orient_normals_*, so its per-voxel averages and its normal_loss see arbitrary signs.  Here every normal faces `viewpoint`,
    by default the origin of the sensor frame the normals are computed in: the sensor itself."""
    k = _check_k("estimate_normals", "max_nn", max_nn)
    radius = float(radius)
    if not (radius >= 0.0 and np.isfinite(radius)):
        raise ValueError("estimate_normals: radius must be a finite length >= 0, got %r" % (radius,))
    grid, args = _frame_grid(points, "estimate_normals")
    out = torch.empty((grid.n, 3), dtype=torch.float64, device=grid.ref.device)
    _lib.call_with_workspace(_lib.lib().shine_frame_normals, out.device, *args, radius, k, ev._d3(viewpoint), _lib.WS,
                             _lib.WS_BYTES, out.data_ptr(), _lib.current_stream_handle())
    return out


class SamplerParams:
    """dataSampler's constants (utils/data_sampler.py:26-37): the scaled lengths are products in double, rounded to fp32 once —
    what `tensor * python_float` does in the reference"""

    def __init__(self, config):
        s = float(config.scale)
        self.ns = int(config.surface_sample_n)
        self.nc = int(getattr(config, "clearance_sample_n", 0))
        self.nf = int(config.free_sample_n)
        self.S = self.ns + self.nc + self.nf
        self.scale = s
        self.surface_range = float(config.surface_sample_range_m) * s
        self.clearance_dist = float(getattr(config, "clearance_dist_m", 0.0)) * s
        self.free_begin_ratio = float(config.free_sample_begin_ratio)
        self.free_end_dist = float(config.free_sample_end_dist_m) * s


def ray_sample(points, origin, params, seed=0, stream_id=0, uniforms=None, labels=None, time_value=0.0, out=None,
               depths=True, origin_time=True):
    """dataSampler.sample in ONE launch (shine_ray_sample).  points [m,3] float32 on the device (scaled space), origin = three
    floats (host), params = SamplerParams (or anything with its fields).  uniforms: None — the counter-based generator keyed by
    (seed, stream_id) — or a device float32 [m * S] tensor in the reference's draw order.  labels: int32 [m] or None.
    `out`: dict of preallocated contiguous tensors to write into (views of the pools); missing ones are allocated.  -> dict with
    coord [mS,3], sdf_label, weight [mS], and, as asked for, sample_depth [mS], ray_depth [m], origin [mS,3], time [mS],
    sem_label [mS] int32 — ray-major (sample j of ray i at i * S + j)."""
    if not points.is_cuda:
        raise _lib.ShineHipError("ray_sample runs on the device only (there is no CPU path)")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("ray_sample: points must be [m,3] float32 (config.dtype float32 is the only sample type), got %s %s"
                         % (tuple(points.shape), points.dtype))
    points = points.contiguous()
    dev, m, S = points.device, int(points.shape[0]), int(params.S)
    want = {"coord": ((m * S, 3), torch.float32), "sdf_label": ((m * S,), torch.float32), "weight": ((m * S,), torch.float32)}
    if depths:
        want["sample_depth"] = ((m * S,), torch.float32)
        want["ray_depth"] = ((m,), torch.float32)
    if origin_time:
        want["origin"] = ((m * S, 3), torch.float32)
        want["time"] = ((m * S,), torch.float32)
    if labels is not None:
        labels = labels.to(device=dev, dtype=torch.int32).contiguous()
        if labels.numel() != m:
            raise ValueError("ray_sample: labels must hold one int per ray")
        want["sem_label"] = ((m * S,), torch.int32)
    res = {}
    for name, (shape, dtype) in want.items():
        t = out.get(name) if out else None
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError("ray_sample: out[%r] must be a contiguous %s %s tensor on %s" % (name, shape, dtype, dev))
        res[name] = t
    if uniforms is not None:
        uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        if uniforms.numel() != m * S:
            raise ValueError("ray_sample: uniforms must hold m * S values")

    def p(name):
        t = res.get(name)
        return t.data_ptr() if t is not None and t.numel() else None

    o3 = (C.c_float * 3)(*[float(v) for v in origin])
    _lib.check(_lib.lib().shine_ray_sample(
        points.data_ptr() if m else None, m, o3, params.ns, params.nc, params.nf, params.surface_range, params.clearance_dist,
        params.free_begin_ratio, params.free_end_dist, params.scale, labels.data_ptr() if labels is not None and m else None,
        int(seed) & _U64, int(stream_id) & _U64, uniforms.data_ptr() if uniforms is not None and m else None, float(time_value),
        p("coord"), p("sdf_label"), p("weight"), p("sample_depth"), p("sem_label"), p("origin"), p("time"), p("ray_depth"),
        _lib.current_stream_handle()), "shine_ray_sample")
    return res


def pool_window_filter(coord, origin, radius, arrays):
    """the sliding window of the batch-mode pool (shine_pool_window_filter): the rows with |coord - origin| < radius (fp32) of up
    to six parallel device arrays ([n] or [n,3], 4-byte elements), order kept.  -> (list of new tensors with the capacity of
    the inputs, rows kept); row k of every output is the same input row."""
    n = int(coord.shape[0])
    if len(arrays) < 1 or len(arrays) > 6:
        raise ValueError("pool_window_filter: 1 to 6 arrays")
    words = []
    for a in arrays:
        if not (a.is_cuda and a.is_contiguous() and a.element_size() == 4 and int(a.shape[0]) == n
                and (a.dim() == 1 or (a.dim() == 2 and a.shape[1] == 3))):
            raise ValueError("pool_window_filter: arrays must be contiguous device [n] or [n,3] tensors of 4-byte elements")
        words.append(1 if a.dim() == 1 else 3)
    outs = [torch.empty_like(a) for a in arrays]
    if n == 0:
        return outs, 0
    if not (coord.is_cuda and coord.is_contiguous() and coord.dtype == torch.float32 and coord.dim() == 2 and coord.shape[1] == 3):
        raise ValueError("pool_window_filter: coord must be a contiguous device [n,3] float32 tensor")
    o3 = (C.c_float * 3)(*[float(v) for v in origin])
    src, dst = _lib.ptr_array([a.data_ptr() for a in arrays]), _lib.ptr_array([a.data_ptr() for a in outs])
    w = (C.c_int32 * len(words))(*words)
    kept = C.c_int64(0)
    _lib.call_with_workspace(_lib.lib().shine_pool_window_filter, coord.device, coord.data_ptr(), n, o3, float(radius), len(arrays),
                             src, dst, w, _lib.WS, _lib.WS_BYTES, C.byref(kept), _lib.current_stream_handle())
    return outs, int(kept.value)


_GOLD, _FNV, _M1, _M2 = 0x9E3779B97F4A7C15, 0x100000001B3, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def _i64(v):
    v &= _U64
    return v - (1 << 64) if v >= (1 << 63) else v


def random_subset(n, keep, seed, stream_id, device):
    """`keep` of n indices, ascending, chosen uniformly: the `keep` smallest of one 64-bit key per index — the splitmix64
    finaliser of (seed, stream_id, index), the generator of the sorted sampler (csrc/shine_sampler_dev.hpp) in int64 arithmetic
    (wrapping multiplies, logical shifts spelled out).  The same (seed, stream_id) gives the same subset on every run."""
    k = torch.arange(n, dtype=torch.int64, device=device)
    z = (k + _i64((int(stream_id) & _U64) * _FNV + 1)) * _i64(_GOLD) + _i64(int(seed))

    def lsr(v, s):
        return (v >> s) & ((1 << (64 - s)) - 1)

    z = (z ^ lsr(z, 30)) * _i64(_M1)
    z = (z ^ lsr(z, 27)) * _i64(_M2)
    z = z ^ lsr(z, 31)
    if keep >= n:
        return k
    return torch.sort(torch.topk(z, int(keep), largest=False, sorted=False).indices).values


def transform_points(points, pose):
    """open3d's PointCloud.transform with a rigid 4x4 pose: R p + t per point, fp64 on the device, products summed left to right"""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    T = np.asarray(pose, dtype=np.float64)
    return torch.stack([x * float(T[r, 0]) + y * float(T[r, 1]) + z * float(T[r, 2]) + float(T[r, 3]) for r in range(3)], 1)


def _empty(shape, dtype, device):
    """a zero-row placeholder on `device`; on a host without a GPU (where only the constructor's host logic can run: poses, frame
    selection, refusals) it lives in host memory instead of failing"""
    if torch.device(device).type == "cuda" and not torch.cuda.is_available():
        device = "cpu"
    return torch.empty(shape, dtype=dtype, device=device)


class _Pool:
    """one pool on the pool device: a capacity-doubling buffer and the number of rows in use"""

    def __init__(self, shape_tail, dtype, device):
        self.tail, self.dtype, self.device = tuple(shape_tail), dtype, device
        self.buf = _empty((0,) + self.tail, dtype, device)
        self.used = 0

    def view(self):
        return self.buf[:self.used]

    def reserve(self, extra):
        """room for `extra` more rows (capacity doubles); -> the view of those rows, which become part of the pool"""
        need = self.used + int(extra)
        cap = int(self.buf.shape[0])
        if need > cap:
            cap = max(need, 2 * cap, 1024)
            buf = torch.empty((cap,) + self.tail, dtype=self.dtype, device=self.device)
            buf[:self.used].copy_(self.buf[:self.used])
            self.buf = buf
        tail = self.buf[self.used:need]
        self.used = need
        return tail

    def replace(self, tensor, used=None):
        self.buf = tensor
        self.used = int(tensor.shape[0]) if used is None else int(used)


POOL_NAMES = ("coord", "sdf_label", "weight", "sample_depth", "ray_depth", "origin", "time")


class LiDARDataset:
    def __init__(self, config, octree=None) -> None:
        self.semantic = bool(getattr(config, "semantic_on", False)) and self._reads_labels(config)
        for name in UNSUPPORTED:
            if not getattr(config, name, False) or (name == "semantic_on" and self.semantic):
                continue
            missing = [a for a in OPTION_PARAMS.get(name, ()) if getattr(config, a, None) is None]
            if name in OPTION_PARAMS and not missing:
                continue  # (served: the parameters are checked below)
            raise NotImplementedError(
                "shine_mapping_amd.dataset.LiDARDataset does not support config.%s = True%s" % (name, {
                    "behind_dropoff_on": " (the reference's own sampler raises there: it multiplies an [N,1] weight tensor by an [N] drop-off in place)",
                    "semantic_on": SEMANTIC_NEEDS,
                }.get(name, " without config.%s" % " and config.".join(missing))))
        self.filter_noise = bool(getattr(config, "filter_noise", False))
        self.estimate_normal = bool(getattr(config, "estimate_normal", False))
        if self.filter_noise:
            _check_k("config.filter_noise", "config.sor_nn", config.sor_nn)
            if not float(config.sor_std) > 0.0:
                raise ValueError("config.filter_noise: config.sor_std must be > 0, got %r" % (config.sor_std,))
        if self.estimate_normal:
            _check_k("config.estimate_normal", "config.normal_max_nn", config.normal_max_nn)
            if not (float(config.normal_radius_m) >= 0.0 and np.isfinite(float(config.normal_radius_m))):
                raise ValueError("config.estimate_normal: config.normal_radius_m must be a finite length >= 0, got %r"
                                 % (config.normal_radius_m,))
        self.config = config
        self.dtype = getattr(config, "dtype", torch.float32)
        if self.dtype != torch.float32:
            raise NotImplementedError("shine_mapping_amd.dataset.LiDARDataset: config.dtype must be torch.float32 (the sampler kernel is fp32)")
        self.device = config.device
        if torch.device(self.device).type != "cuda":
            raise _lib.ShineHipError("shine_mapping_amd.dataset.LiDARDataset runs on the device only (config.device = %r; there is no CPU path)" % (self.device,))

        self.poses_w = self._read_poses(config)
        self.poses_ref = self.poses_w  # (the reference's aliasing: poses_w is overwritten for the used frames)

        self.pc_filenames = self._list_frames(config)
        self.total_pc_count = len(self.pc_filenames)
        self.octree = octree
        self.last_relative_tran = np.eye(4)
        self.sampler = SamplerParams(config)
        self.ray_sample_count = config.surface_sample_n + config.free_sample_n
        self.seed = int(getattr(config, "seed", 42))

        self.map_down_pc = PointCloud()
        self.map_bbx = BoundingBox()
        self.cur_bbx = BoundingBox()
        self.cur_frame_pc = PointCloud()

        self.used_pc_count = 0
        begin_flag = False
        self.begin_pose_inv = np.eye(4)
        for frame_id in range(self.total_pc_count):
            if frame_id < config.begin_frame or frame_id > config.end_frame or frame_id % config.every_frame != 0:
                continue
            if not begin_flag:  # the first frame used
                begin_flag = True
                if getattr(config, "first_frame_ref", True):
                    self.begin_pose_inv = np.linalg.inv(self.poses_w[frame_id])  # T_rw
                else:
                    self.begin_pose_inv[2, 3] += getattr(config, "global_shift_default", 0.0)
            self.poses_ref[frame_id] = np.matmul(self.begin_pose_inv, self.poses_w[frame_id])
            self.used_pc_count += 1

        if (self.used_pc_count > getattr(config, "pc_count_gpu_limit", 500)
                and not getattr(config, "continual_learning_reg", False) and not getattr(config, "window_replay_on", False)):
            self.pool_device = "cpu"  # (sampling still runs on the device; the pools live in host memory)
            self.to_cpu = True
            print("too many scans, use cpu memory")
        else:
            self.pool_device = config.device
            self.to_cpu = False

        self._pools = {n: _Pool((3,) if n in ("coord", "origin") else (), self.dtype, self.pool_device) for n in POOL_NAMES}
        self.normal_label_pool = _empty((0, 3), self.dtype, self.pool_device)
        self.color_label_pool = _empty((0, 3), self.dtype, self.pool_device)
        self.sem_label_pool = _empty((0,), torch.long, self.pool_device)
        self.label_map = None
        if self.semantic:
            from .semantic_kitti import LabelMap

            self.label_map = LabelMap.from_config(config)
            self._pools["sem_label"] = _Pool((), torch.int32, self.pool_device)
        if self.estimate_normal:  # (one row per sample, the ray's normal repeated: dataSampler.sample's repeat + transpose)
            self._pools["normal_label"] = _Pool((3,), self.dtype, self.pool_device)
        self.cur_frame_normals = None  # the normals of the last frame_points / sem_frame_points call: fp64 [m,3], SENSOR frame
        self._publish()
        self._pool_version = 0
        self._sorted = None  # (SortedPool, pool version, tables epoch)
        self._sorted_perm = None

    # ---- pools --------------------------------------------------------------------------------------------------------------
    def _publish(self):
        for n in self._pools:
            setattr(self, n + "_pool", self._pools[n].view())

    def _kept_pools(self):
        """the pools batch mode appends to (dataset/lidar_dataset.py:262-281)"""
        names = ("coord", "weight", "sample_depth", "ray_depth") if self.config.ray_loss else \
            ("coord", "weight", "sdf_label", "origin", "time")
        names = names + ("sem_label",) if self.semantic else names
        return names + ("normal_label",) if self.estimate_normal else names

    def _reads_labels(self, config):
        """semantic_on is served only with a folder of label files (rgbd.RGBDDataset: never)"""
        path = getattr(config, "label_path", None)
        return isinstance(path, str) and path != ""

    # ---- files ----------------------------------------------------------------------------------------------------------------
    # (the two things a subclass with another kind of frame file replaces, next to frame_points: rgbd.RGBDDataset)
    def _read_poses(self, config):
        """the sensor poses in the world frame, one 4x4 per frame (dataset/lidar_dataset.py:47-57)"""
        self.calib = {}
        if getattr(config, "calib_path", "") != "":
            self.calib = read_calib_file(config.calib_path)
        else:
            self.calib["Tr"] = np.eye(4)
        if config.pose_path.endswith("txt"):
            return read_poses_file(config.pose_path, self.calib)
        if config.pose_path.endswith("csv"):
            return csv_odom_to_transforms(config.pose_path)
        raise ValueError("Wrong pose file format. Please use either *.txt (KITTI format) or *.csv (xyz+quat format)")

    def _list_frames(self, config):
        """the frame files in natural order"""
        return sorted(os.listdir(config.pc_path), key=natural_key)

    def read_point_cloud(self, filename: str):
        """the raw points of a file on the device: [n,4] float32 (.bin) or [n,3] float64 (.ply)"""
        if ".bin" in filename:
            pts = torch.from_numpy(np.fromfile(filename, dtype=np.float32).reshape((-1, 4)))
        elif ".ply" in filename:
            pts = torch.from_numpy(np.ascontiguousarray(ev.read_ply(filename)["vertices"], dtype=np.float64))
        elif ".pcd" in filename:
            raise NotImplementedError("shine_mapping_amd.dataset.LiDARDataset does not read .pcd files (%s): convert to .ply or "
                                      "KITTI .bin" % filename)
        else:
            raise ValueError("The format of the imported point cloud is wrong (support only *ply and *bin): %s" % filename)
        return pts.to(self.device)

    def sapce_carving_sample(self, *args, **kwargs):
        raise NotImplementedError("shine_mapping_amd.dataset.LiDARDataset does not support sapce_carving_sample (deprecated in the "
                                  "reference; it needs kaolin's ray tracer)")

    # ---- one frame ------------------------------------------------------------------------------------------------------------
    def frame_points(self, frame_id):
        """stages 1-3 of process_frame: the frame's points in the SENSOR frame after filter, crop and down-sampling (fp64 device)"""
        cfg = self.config
        raw = self.read_point_cloud(os.path.join(cfg.pc_path, self.pc_filenames[frame_id]))
        pts = frame_filter(raw, cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius)
        return self._down_sample(pts, frame_id)

    def _down_sample(self, pts, frame_id, classes=None):
        """stage 3: the filtered points of a frame -> the seeded random subset or the voxel means; with classes (int32 [n]) ->
        (points, classes): the same subset of both, or the voxel means with rint(mean(class / 255) * 255) as the voxel's class.
        In the reference's order (dataset/lidar_dataset.py:144-164), with config.estimate_normal the normals of the cloud as it
        comes in (estimate_normals, facing the sensor) travel through the down-sampling — the same subset, or the per-voxel MEAN
        of the normals, not re-normalised: what open3d's voxel accumulator returns — and with config.filter_noise the
        down-sampled cloud loses its statistical outliers (statistical_outlier_mask), points, classes and normals alike.  The
        normals are left in `cur_frame_normals` (None without estimate_normal)."""
        cfg = self.config
        if pts.shape[0] == 0:
            raise ValueError("frame %d (%s): no point passes min_z / min_range / the crop box" % (frame_id, self.pc_filenames[frame_id]))
        normals = estimate_normals(pts, cfg.normal_radius_m, cfg.normal_max_nn) if self.estimate_normal else None
        if cfg.rand_downsample:
            n = int(pts.shape[0])
            keep = int(n * cfg.rand_down_r)
            if keep < n:
                subset = random_subset(n, keep, self.seed, frame_id, pts.device)
                pts = pts[subset]
                classes = classes[subset] if classes is not None else None
                normals = normals[subset] if normals is not None else None
        elif classes is None and normals is None:
            pts = ev.voxel_down_sample(pts, cfg.vox_down_m)
        elif normals is None:
            pts, mean = ev.voxel_down_sample(pts, cfg.vox_down_m, attrs=classes.double() / 255.0)
            classes = torch.round(mean * 255.0).to(torch.int32)  # (two roundings, as numpy's `colors * 255.0` then np.round)
        else:  # the normals as three attribute columns, behind the class column if there is one (4 columns: the limit)
            attrs = normals if classes is None else torch.cat([(classes.double() / 255.0)[:, None], normals], 1)
            pts, mean = ev.voxel_down_sample(pts, cfg.vox_down_m, attrs=attrs)
            normals = mean[:, -3:].contiguous()
            if classes is not None:
                classes = torch.round(mean[:, 0] * 255.0).to(torch.int32)
        if self.filter_noise:
            keep = statistical_outlier_mask(pts, cfg.sor_nn, cfg.sor_std)[0]
            pts = pts[keep]
            classes = classes[keep] if classes is not None else None
            normals = normals[keep] if normals is not None else None
            if pts.shape[0] == 0:
                raise ValueError("frame %d (%s): no point passes filter_noise (sor_nn %r, sor_std %r)"
                                 % (frame_id, self.pc_filenames[frame_id], cfg.sor_nn, cfg.sor_std))
        self.cur_frame_normals = normals
        return pts if classes is None else (pts, classes)

    def read_semantic_point_label(self, bin_filename, label_filename):
        """a labelled scan on the device: ([n,4] float32 points, [n] int32 holding the uint32 label words' bits)"""
        if ".bin" not in bin_filename:
            raise ValueError("The format of the imported point cloud is wrong (semantic_on supports only *bin): %s" % bin_filename)
        if ".label" not in label_filename:
            raise ValueError("The format of the imported point labels is wrong (support only *label): %s" % label_filename)
        pts = np.fromfile(bin_filename, dtype=np.float32).reshape((-1, 4))
        labels = np.fromfile(label_filename, dtype=np.uint32).reshape(-1)
        if len(labels) != len(pts):
            raise ValueError("%s holds %d labels, %s holds %d points" % (label_filename, len(labels), bin_filename, len(pts)))
        return torch.from_numpy(pts).to(self.device), torch.from_numpy(labels.view(np.int32)).to(self.device)

    def sem_frame_points(self, frame_id):
        """frame_points with semantic_on: (points fp64 [m,3] in the SENSOR frame, classes int32 [m]) after the label filters, the
        learning map, the crop and the down-sampling"""
        cfg = self.config
        name = self.pc_filenames[frame_id]
        raw, labels = self.read_semantic_point_label(os.path.join(cfg.pc_path, name),
                                                     os.path.join(cfg.label_path, name.replace("bin", "label")))
        # (the reference's positional call, dataset/lidar_dataset.py:319-321: min_z lands in min_range, min_range in filter_outlier)
        pts, classes = sem_frame_filter(raw, labels, self.label_map, cfg.min_z, getattr(cfg, "filter_moving_object", True),
                                        bool(cfg.min_range), cfg.min_z, cfg.max_z, cfg.pc_radius)
        return self._down_sample(pts, frame_id, classes)

    def process_frame(self, frame_id, incremental_on=False):
        cfg = self.config
        self.cur_pose_ref = self.poses_ref[frame_id]
        classes = None
        if self.semantic:
            pts, classes = self.sem_frame_points(frame_id)
            pts = transform_points(pts, self.cur_pose_ref)
        else:
            pts = transform_points(self.frame_points(frame_id), self.cur_pose_ref)
        frame_origin = (self.cur_pose_ref[:3, 3] * cfg.scale).astype(np.float32)
        normals = None
        if self.estimate_normal:  # R n in fp64 (a direction: no translation, and config.scale does not touch it), then the cast
            rot = np.array(self.cur_pose_ref, dtype=np.float64)
            rot[:3, 3] = 0.0
            normals = transform_points(self.cur_frame_normals, rot).to(self.dtype)

        # the copy merged into the map cloud
        if classes is not None and self.label_map.colors is not None:  # (the class colours, averaged per map voxel as open3d does)
            self.cur_frame_pc = PointCloud(*ev.voxel_down_sample(
                pts, cfg.map_vox_down_m, attrs=self.label_map.device_colors(pts.device)[classes.long()]))
        else:
            self.cur_frame_pc = PointCloud(ev.voxel_down_sample(pts, cfg.map_vox_down_m))
        self.map_down_pc += self.cur_frame_pc
        lo, hi = ev.bounds(self.cur_frame_pc.points)
        self.cur_bbx = BoundingBox(lo, hi)
        self.map_bbx = BoundingBox(self.map_bbx.min_bound, self.map_bbx.max_bound).extend(lo, hi)  # (running union)

        pts_s = (pts * cfg.scale).to(self.dtype)  # scale in fp64 as open3d does, then the cast of torch.tensor(..., dtype)
        m, S = int(pts_s.shape[0]), self.sampler.S
        on_device = not self.to_cpu
        pools = self._pools
        point_mode = not cfg.ray_loss
        if incremental_on:
            out = None  # fresh tensors replace the pools
        else:
            if getattr(cfg, "window_replay_on", False) and pools["coord"].used:
                if cfg.ray_loss:
                    raise NotImplementedError("window_replay_on with ray_loss in batch mode: the reference's window filter indexes "
                                              "the empty sdf_label_pool there and raises; switch one of them off")
                names = tuple(n for n in self._kept_pools() if n != "normal_label")
                coord, radius = pools["coord"].view(), cfg.window_radius * cfg.scale
                outs, kept = pool_window_filter(coord, frame_origin, radius, [pools[n].view() for n in names])
                if self.estimate_normal:  # (the filter takes six arrays: the normals go through a call of their own, same mask)
                    names += ("normal_label",)
                    outs += pool_window_filter(coord, frame_origin, radius, [pools["normal_label"].view()])[0]
                for n, t in zip(names, outs):
                    pools[n].replace(t, kept)
            out = None
            if on_device:  # the sampler writes straight into the pools' tails
                out = {n: pools[n].reserve(m if n == "ray_depth" else m * S) for n in self._kept_pools()}
        res = ray_sample(pts_s, frame_origin, self.sampler, seed=self.seed, stream_id=frame_id, time_value=float(frame_id), out=out,
                         depths=bool(cfg.ray_loss), origin_time=point_mode or incremental_on, labels=classes)
        if normals is not None:  # row i * S + j = the normal of ray i
            rows = normals[:, None, :].expand(m, S, 3)
            if out is not None:
                out["normal_label"].view(m, S, 3).copy_(rows)
            else:
                res["normal_label"] = rows.reshape(m * S, 3)

        if self.octree is not None:
            if cfg.octree_from_surface_samples:
                # coord[weight > 0]: the first surface_sample_n samples of every ray, in the same order
                surf = res["coord"].view(m, S, 3)[:, :self.sampler.ns].reshape(-1, 3)
                self.octree.update(surf, incremental_on)
            else:
                self.octree.update(pts_s, incremental_on)

        if incremental_on:
            for n in pools:
                t = res.get(n)
                if t is None:
                    t = torch.empty((0,) + pools[n].tail, dtype=pools[n].dtype, device=self.device)
                pools[n].replace(t.to(self.pool_device))
        elif not on_device:
            for n in self._kept_pools():
                pools[n].reserve(res[n].shape[0]).copy_(res[n])
        self.normal_label_pool = None  # (with estimate_normal: _publish sets the view of the `normal_label` pool)
        self.sem_label_pool = None  # (with semantic_on: _publish sets the int32 view of the `sem_label` pool)
        self._publish()
        self._pool_version += 1

    # ---- batches --------------------------------------------------------------------------------------------------------------
    def sorted_pool(self):
        """the point-sample pools as a SortedPool (node order + hash slots), planned when the pools or the octree changed: what
        loop.GraphedIteration / fused_train_step(pool=...) take, and what get_batch draws through"""
        from .sampler import SortedPool

        if self.octree is None:
            raise ValueError("LiDARDataset.sorted_pool needs the octree the dataset was built with")
        if self.config.ray_loss or self.to_cpu:
            raise ValueError("LiDARDataset.sorted_pool serves the point-sample pools on the device (not ray_loss, not the CPU pool)")
        key = (self._pool_version, self.octree._tables_epoch)
        if self._sorted is None or self._sorted[1] != key:
            # (semantic_on: the labels travel with the pool, checked against the head's class count)
            extra = dict(sem_label=self.sem_label_pool, n_class=int(self.config.sem_class_count) + 1) if self.semantic else {}
            if self.estimate_normal:  # (the normals travel with the pool: loop.GraphedIteration(normal=...) reads them)
                extra["normal_label"] = self.normal_label_pool
            if getattr(self.config, "time_conditioned", False):  # (the time stamps too: the loop's time route reads pool.ts)
                extra["ts"] = self.time_pool
            if self._sorted is None:
                sp = SortedPool(self.octree, self.coord_pool, self.sdf_label_pool, self.weight_pool, seed=self.seed, **extra)
            else:
                sp = self._sorted[0]
                sp.rebuild(self.coord_pool, self.sdf_label_pool, self.weight_pool, **extra)
            self._sorted = (sp, key)
            self._sorted_perm = sp.perm.long()
        return self._sorted[0]

    def ray_pool(self):
        """the pools of ray mode (config.ray_loss) as a sampler.RayPool, planned when the pools or the octree changed: what
        loop.GraphedIteration(ray=RayTerm(...)) / ops.fused_ray_step(pool=...) take"""
        from .sampler import RayPool

        if not self.config.ray_loss:
            raise ValueError("LiDARDataset.ray_pool serves ray mode (config.ray_loss); the point-sample pools are sorted_pool()'s")
        if self.octree is None or self.to_cpu:
            raise ValueError("LiDARDataset.ray_pool needs the octree the dataset was built with and the pools on the device")
        key = (self._pool_version, self.octree._tables_epoch)
        cached = getattr(self, "_ray_pool", None)
        if cached is None or cached[1] != key:
            pools = (self.coord_pool, self.weight_pool, self.sample_depth_pool, self.ray_depth_pool)
            if cached is None:
                rp = RayPool(self.octree, *pools, samples=self.ray_sample_count, seed=self.seed)
            else:
                rp = cached[0]
                rp.rebuild(*pools, samples=self.ray_sample_count)
            self._ray_pool = (rp, key)
        return self._ray_pool[0]

    def get_batch(self):
        cfg = self.config
        if cfg.ray_loss:
            n_ray = self.ray_depth_pool.shape[0]
            # (the reference's ray_sample_count = surface_sample_n + free_sample_n is the stride it indexes the pool with)
            R = self.ray_sample_count
            ray_index = torch.randint(0, n_ray, (cfg.bs,), device=self.pool_device)
            index = ((ray_index * R).repeat(R, 1) + torch.arange(0, R, dtype=torch.int64, device=self.pool_device).reshape(-1, 1)
                     ).transpose(0, 1).reshape(-1)
            coord = self.coord_pool[index, :].to(self.device)
            weight = self.weight_pool[index].to(self.device)
            sample_depth = self.sample_depth_pool[index].to(self.device)
            ray_depth = self.ray_depth_pool[ray_index].to(self.device)
            sem_label = self.sem_label_pool[ray_index * R].to(self.device).long() if self.semantic else None  # (one per ray)
            normal_label = self.normal_label_pool[index, :].to(self.device) if self.estimate_normal else None  # (coord's rows)
            return coord, sample_depth, ray_depth, normal_label, sem_label, weight
        if self.octree is not None and not self.to_cpu:
            sp = self.sorted_pool()
            idx = sp.draw(cfg.bs)
            coord, sdf_label, weight = sp.get_batch(idx)
            src = self._sorted_perm[idx.long()]
            sem_label = self.sem_label_pool[src].long() if self.semantic else None  # (int64: what NLLLoss takes)
            normal_label = self.normal_label_pool[src] if self.estimate_normal else None
            return coord, sdf_label, self.origin_pool[src], self.time_pool[src], normal_label, sem_label, weight
        n = self.sdf_label_pool.shape[0]
        index = torch.randint(0, n, (cfg.bs,), device=self.pool_device)
        sem_label = self.sem_label_pool[index].to(self.device).long() if self.semantic else None
        normal_label = self.normal_label_pool[index, :].to(self.device) if self.estimate_normal else None
        return (self.coord_pool[index, :].to(self.device), self.sdf_label_pool[index].to(self.device),
                self.origin_pool[index].to(self.device), self.time_pool[index].to(self.device), normal_label, sem_label,
                self.weight_pool[index].to(self.device))

    def write_merged_pc(self, out_path):
        from .mesher import write_ply

        pts = transform_points(self.map_down_pc.points, np.linalg.inv(self.begin_pose_inv)).cpu().numpy()  # back to the world frame
        props = [("x", pts[:, 0], "double"), ("y", pts[:, 1], "double"), ("z", pts[:, 2], "double")]
        colors = self.map_down_pc.colors
        if colors is not None:  # (a semantic map: the class colours, written as Mesher._finish writes a mesh's)
            rgb = np.clip(np.round(colors.cpu().numpy() * 255.0), 0, 255).astype(np.uint8)
            props += [("red", rgb[:, 0], "uchar"), ("green", rgb[:, 1], "uchar"), ("blue", rgb[:, 2], "uchar")]
        write_ply(out_path, props)
        print("save the merged point cloud map to %s\n" % (out_path))

    def __len__(self) -> int:
        if self.config.ray_loss:
            return self.ray_depth_pool.shape[0]  # ray count
        return self.sdf_label_pool.shape[0]  # point sample count
