"""Plain numpy fp64 restatements of the evaluation stages (shine_mapping_amd/evaluation.py), written from the stage descriptions
and independent of the device code: the role tests/mc_oracle.py plays for marching cubes.  Everything is host side."""
import math

import numpy as np

METRIC_KEYS = ["MAE_accuracy (m)", "MAE_completeness (m)", "Chamfer_L1 (m)", "Chamfer_L2 (m)", "Precision [Accuracy] (%)",
               "Recall [Completeness] (%)", "F-score (%)", "Spacing (m)", "Inlier_threshold (m)", "Outlier_truncation_acc (m)",
               "Outlier_truncation_com (m)"]


def have_scipy():
    try:
        import scipy.spatial  # noqa: F401

        return True
    except Exception:
        return False


def crop_mesh(verts, faces, min_bound, max_bound):
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.all((verts >= np.asarray(min_bound)) & (verts <= np.asarray(max_bound)), axis=1)
    new_id = np.cumsum(keep) - 1
    fk = keep[faces].all(1) if len(faces) else np.zeros(0, bool)
    return verts[keep], new_id[faces[fk]].astype(np.int32).reshape(-1, 3)


def triangle_areas(verts, faces):
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    return 0.5 * np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)


def sample_points(verts, faces, uniforms):
    """(points, triangle of every sample) for injected uniforms [n,3]"""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    u = np.asarray(uniforms, np.float64)
    cum = np.cumsum(triangle_areas(verts, faces))
    cdf = cum / cum[-1]
    tri = np.searchsorted(cdf, u[:, 0], side="right")  # first i with cdf[i] > u0
    r = np.sqrt(u[:, 1])
    w0, w1, w2 = 1.0 - r, r * (1.0 - u[:, 2]), r * u[:, 2]
    f = faces[tri]
    pts = w0[:, None] * verts[f[:, 0]] + w1[:, None] * verts[f[:, 1]] + w2[:, None] * verts[f[:, 2]]
    return pts, tri, cdf


def voxel_down_sample(points, voxel):
    """(means [m,3], keys [m]) in ascending key order; key = ix << 42 | iy << 21 | iz"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64)
    origin = p.min(0) - voxel * 0.5
    idx = np.floor((p - origin) / voxel).astype(np.int64)
    keys = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    counts = np.diff(np.r_[start, len(ks)])
    means = np.stack([np.add.reduceat(p[order, a], start) for a in range(3)], 1) / counts[:, None]
    return means, ks[start]


def nn_brute(ref, query, chunk=None, second=False):
    """(index, distance[, second-best distance]) of the nearest reference point of every query by chunked brute force; first
    index on ties"""
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    query = np.asarray(query, np.float64).reshape(-1, 3)
    if chunk is None:
        chunk = max(1, int(2.5e7 // max(len(ref), 1)))
    idx = np.empty(len(query), np.int64)
    d = np.empty(len(query))
    d2nd = np.full(len(query), np.inf)
    for s in range(0, len(query), chunk):
        q = query[s:s + chunk]
        d2 = ((q[:, None, :] - ref[None, :, :]) ** 2).sum(-1)
        i = d2.argmin(1)
        idx[s:s + chunk] = i
        rows = np.arange(len(q))
        d[s:s + chunk] = np.sqrt(d2[rows, i])
        if second and len(ref) > 1:
            d2[rows, i] = np.inf
            d2nd[s:s + chunk] = np.sqrt(d2.min(1))
    return (idx, d, d2nd) if second else (idx, d)


def nn_tree(ref, query, second=False, workers=16):
    """the same through scipy's cKDTree (when scipy imports)"""
    from scipy.spatial import cKDTree

    tree = cKDTree(np.asarray(ref, np.float64))
    if second and len(ref) > 1:
        d, i = tree.query(np.asarray(query, np.float64), k=2, workers=workers)
        return i[:, 0], d[:, 0], d[:, 1]
    d, i = tree.query(np.asarray(query, np.float64), k=1, workers=workers)
    return (i, d, np.full(len(d), np.inf)) if second else (i, d)


def nn(ref, query, second=False):
    """cKDTree distances are sqrt of the same fp64 squared sums; brute force is the fallback"""
    return nn_tree(ref, query, second) if have_scipy() else nn_brute(ref, query, second=second)


def nn_correspondence(ref, query, truncation, ignore_outlier=True, nearest=None):
    """(indices, distances, keep) in the reference's compacted form; `nearest` = a precomputed (index, distance)"""
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    query = np.asarray(query, np.float64).reshape(-1, 3)
    if len(ref) == 0 or len(query) == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0, bool)
    idx, d = nearest if nearest is not None else nn(ref, query)[:2]
    d2 = ((query - ref[idx]) ** 2).sum(-1)  # the squared distance itself, as the reference compares it
    keep = d2 < truncation ** 2
    if ignore_outlier:
        return idx[keep], np.sqrt(d2[keep]), keep
    return idx, np.where(keep, np.sqrt(d2), truncation), keep


def metrics(dist_p, dist_r, down_sample_res, threshold, truncation_acc, truncation_com):
    dist_p, dist_r = np.asarray(dist_p, np.float64), np.asarray(dist_r, np.float64)
    with np.errstate(all="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mp, mr = np.mean(dist_p), np.mean(dist_r)
            mp2, mr2 = np.mean(np.square(dist_p)), np.mean(np.square(dist_r))
            precision = np.mean((dist_p < threshold).astype("float")) * 100.0
            recall = np.mean((dist_r < threshold).astype("float")) * 100.0
        fscore = 2 * precision * recall / (precision + recall) if precision + recall != 0 else float("nan")
    vals = [mp, mr, 0.5 * (mp + mr), math.sqrt(0.5 * (mp2 + mr2)) if not math.isnan(mp2 + mr2) else float("nan"), precision,
            recall, fscore, down_sample_res, threshold, truncation_acc, truncation_com]
    return dict(zip(METRIC_KEYS, [float(v) for v in vals]))


def eval_mesh_from_points(pred_pts, trgt_pts, down_sample_res=0.02, threshold=0.05, truncation_acc=0.50, truncation_com=0.50,
                          return_distances=False):
    """eval_mesh from the sampling step on: pred_pts = the points sampled from the (already cropped) mesh"""
    pred = np.asarray(pred_pts, np.float64).reshape(-1, 3)
    trgt = np.asarray(trgt_pts, np.float64).reshape(-1, 3)
    if down_sample_res > 0:
        pred = voxel_down_sample(pred, down_sample_res)[0]
        trgt = voxel_down_sample(trgt, down_sample_res)[0]
    _, dist_p, _ = nn_correspondence(trgt, pred, truncation_acc, True)
    _, dist_r, _ = nn_correspondence(pred, trgt, truncation_com, False)
    m = metrics(dist_p, dist_r, down_sample_res, threshold, truncation_acc, truncation_com)
    return (m, dist_p, dist_r) if return_distances else m


def fibonacci_sphere(n, radius, centre=(0.0, 0.0, 0.0)):
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1) * radius + np.asarray(centre, np.float64)
