"""Plain numpy restatement of shine_depth_unproject's rules (include/shine_hip.h; shine_mapping_amd/rgbd.py), written from the rule
text and independent of the device code: the role tests/frame_oracle.py plays for the LiDAR stages.  Host side only.

  unproject   depth image -> (points [n,3] float64, pixel indices [n] int32) in ascending pixel index v * width + u:
                d = float32(raw) / float32(depth_scale)                      one fp32 division
                valid iff d > 0, d < float32(depth_trunc), d finite
                z = float64(d), x = (u - cx) * z / fx, y = (v - cy) * z / fy   fp64, in this order
                p = M (x, y, z, 1), each row m0 * x + m1 * y + m2 * z + m3 summed left to right (M = cam_to_sensor or identity)
                kept iff z > min_z, |p| >= min_range (sqrt(x*x + y*y + z*z)), |x|, |y| <= pc_radius, min_z <= z <= max_z
              numpy evaluates every one of these as a single correctly rounded IEEE operation (no fused multiply-add).
  surface_distance   how far a world point is from the synthetic room's surface of a given kind (synth.write_rgbd_drive)
"""
import numpy as np

FILTER_OFF = (-np.inf, np.inf, 0.0, np.inf)


def unproject(depth, fx, fy, cx, cy, depth_scale, depth_trunc, cam_to_sensor=None, box=None):
    raw = np.asarray(depth)
    assert raw.ndim == 2 and raw.dtype in (np.uint16, np.float32)
    h, w = raw.shape
    with np.errstate(invalid="ignore", over="ignore"):
        d = raw.astype(np.float32) / np.float32(depth_scale)
        assert d.dtype == np.float32
        valid = (d > 0) & (d < np.float32(depth_trunc)) & np.isfinite(d)
    v, u = np.nonzero(valid)  # row-major: ascending v * w + u
    z = d[v, u].astype(np.float64)
    x = (u.astype(np.float64) - np.float64(cx)) * z / np.float64(fx)
    y = (v.astype(np.float64) - np.float64(cy)) * z / np.float64(fy)
    M = np.eye(4) if cam_to_sensor is None else np.asarray(cam_to_sensor, dtype=np.float64)
    p = np.stack([M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] for r in range(3)], 1).reshape(-1, 3)
    min_z, max_z, min_range, radius = FILTER_OFF if box is None else box
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(px * px + py * py + pz * pz)
        keep = (pz > min_z) & (r >= min_range) & (px >= -radius) & (px <= radius) & (py >= -radius) & (py <= radius) \
            & (pz >= min_z) & (pz <= max_z)
    index = (v.astype(np.int64) * w + u).astype(np.int32)
    return p[keep], index[keep]


def transform(points, pose):
    """R p + t, every row summed left to right (dataset.transform_points)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    T = np.asarray(pose, np.float64)
    return np.stack([p[:, 0] * T[r, 0] + p[:, 1] * T[r, 1] + p[:, 2] * T[r, 2] + T[r, 3] for r in range(3)], 1)


def surface_distance(world, kind, room, boxes):
    """distance (m) of every world point from the room surface of its kind: 0 ground (the plane z = 0), 1 facade (the nearer of
    the planes |y| = half_width, plus how far z leaves [0, facade_h]), 2 box (the nearest box surface)"""
    p = np.asarray(world, np.float64).reshape(-1, 3)
    kind = np.asarray(kind).reshape(-1)
    out = np.full(len(p), np.inf)
    g = kind == 0
    out[g] = np.abs(p[g, 2])
    f = kind == 1
    zf = p[f, 2]
    out[f] = np.maximum(np.abs(np.abs(p[f, 1]) - room["half_width"]), np.maximum(np.maximum(-zf, zf - room["facade_h"]), 0.0))
    b = kind == 2
    if b.any():
        lo, hi = boxes
        q = p[b][:, None, :]
        outside = np.maximum(np.maximum(lo[None] - q, q - hi[None]), 0.0)  # [m, boxes, 3]
        d_out = np.sqrt((outside ** 2).sum(-1))
        inside = np.minimum(q - lo[None], hi[None] - q).min(-1)  # depth below the nearest face, where the point is inside
        d = np.where(d_out > 0, d_out, np.maximum(inside, 0.0))
        out[b] = d.min(1)
    return out
