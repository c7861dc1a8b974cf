"""Plain numpy fp64 restatements of the SEMANTIC frame stages of shine_mapping_amd/dataset.py (LiDARDataset with semantic_on), written
from the stage descriptions and independent of the device code; the sibling of tests/frame_oracle.py.  Host side only.

  sem_filter     preprocess_sem_kitti (dataset/lidar_dataset.py:341-362): |p| >= range_min, id < 100 (filter_moving), id != 1
                 (filter_outlier), the learning map as an int32 LUT, then the inclusive crop box; an unmapped id among the points
                 that pass the label tests raises KeyError, as the reference's dict lookup does
  voxel_attr     frame_oracle.voxel_down plus per-voxel attribute means, summed in input order (what open3d does with colours)
  voxel_classes  the reference's detour through the colour channel: class / 255 averaged per voxel, * 255.0, rounded half to even
  frame          filter -> voxel classes -> transform -> map copy with the class colours averaged per map voxel
  sample_labels  the class of a ray on its first `ns` samples, 0 on the rest: the layout dataSampler.sample gives sem_label
"""
import numpy as np

import frame_oracle as fo


def sem_filter(points, labels, lut, range_min, filter_moving, filter_outlier, min_z=-np.inf, max_z=np.inf, radius=np.inf):
    """-> (kept indices, classes of the kept points)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    s = (np.asarray(labels).astype(np.int64) & 0xFFFF)
    ok = np.linalg.norm(p, axis=1) >= range_min
    if filter_moving:
        ok &= s < 100
    if filter_outlier:
        ok &= s != 1
    cls = np.asarray(lut)[s]
    if np.any(ok & (cls < 0)):
        raise KeyError(int(s[ok & (cls < 0)][0]))
    lo, hi = np.array([-radius, -radius, min_z]), np.array([radius, radius, max_z])
    keep = ok & np.all((p >= lo) & (p <= hi), axis=1)
    idx = np.flatnonzero(keep)
    return idx, cls[idx].astype(np.int32)


def voxel_attr(points, attrs, voxel):
    """(point means [m,3], keys [m], attribute means [m,a]) in ascending key order; every sum runs in input order"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    a = np.asarray(attrs, np.float64).reshape(len(p), -1)
    if len(p) == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros((0, a.shape[1]))
    origin = p.min(0) - voxel * 0.5
    idx = np.floor((p - origin) / voxel).astype(np.int64)
    keys = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    uniq, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    sums, asums = np.zeros((len(uniq), 3)), np.zeros((len(uniq), a.shape[1]))
    np.add.at(sums, inverse, p)  # (unbuffered: one addition per point, in input order)
    np.add.at(asums, inverse, a)
    return sums / counts[:, None], uniq, asums / counts[:, None]


def voxel_classes(points, classes, voxel):
    means, keys, col = voxel_attr(points, np.asarray(classes, np.float64) / 255.0, voxel)
    return means, keys, np.round(col[:, 0] * 255.0, 0).astype(np.int32)


def frame(raw, labels, pose, cfg, lut, colors):
    """raw [n,3] (the file's float32 values), labels [n] uint32 -> dict(kept, sensor, classes (per down-sampled point), class_means (before
    rounding), world, cur, cur_colors, lo, hi) with the reference's positional quirk: range_min = cfg.min_z, filter_outlier = bool(cfg.min_range)"""
    p = np.asarray(raw, np.float64).reshape(-1, 3)
    kept, cls = sem_filter(p, labels, lut, cfg.min_z, cfg.filter_moving_object, bool(cfg.min_range), cfg.min_z, cfg.max_z,
                           cfg.pc_radius)
    sensor, skeys, col = voxel_attr(p[kept], np.asarray(cls, np.float64) / 255.0, cfg.vox_down_m)
    class_means = col[:, 0] * 255.0  # (not an integer where a voxel holds several classes)
    classes = np.round(class_means, 0).astype(np.int32)
    world = fo.transform(sensor, pose)
    cur, ckeys, cur_colors = voxel_attr(world, np.asarray(colors, np.float64)[classes], cfg.map_vox_down_m)
    return dict(kept=kept, kept_classes=cls, sensor=sensor, classes=classes, class_means=class_means, world=world, cur=cur, cur_colors=cur_colors,
                lo=cur.min(0), hi=cur.max(0))


def sample_labels(classes, ns, S):
    out = np.zeros((len(classes), S), np.int32)
    out[:, :ns] = np.asarray(classes, np.int32)[:, None]
    return out.reshape(-1)


def read_labels(path):
    return np.fromfile(path, dtype=np.uint32).reshape(-1)
