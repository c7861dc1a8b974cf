"""Synthetic LiDAR workloads shaped like the reference's datasets (there is no network for the real ones).

SURVEY.md §8(d): an analytic street canyon ray-cast from a 64-beam spinning sensor, then the reference's
per-ray sampling scheme (utils/data_sampler.py:18-139: uniform +-range around the hit, uniform in free
space from 0.3 x range to a bit behind the surface), giving the (coord, sdf_label, weight) sample pool
that LiDARDataset.get_batch draws from (dataset/lidar_dataset.py:430-450).  Everything is torch and
device-agnostic, so bench.py generates the pool on the GPU in a second or two.

Workload presets follow the shipped yamls:
  maicity : config/maicity/maicity_batch.yaml  leaf 0.2 m, L=3 (or 4), sigma 0.05, BCE only
  kitti   : config/kitti/kitti_batch.yaml      leaf 0.3 m, L=3, sigma 0.1, eikonal on (w_e 0.1); 600 m polyline with
            two turns
  kitti_large : the same sensor/config on an 8 x 1 km serpentine (8.4 km of trajectory): a map whose feature tables
            (> 256 MiB) do not fit the Infinity Cache — the regime dataset/lidar_dataset.py:93-97 anticipates
  ncd     : config/ncd/ncd_incre_reg.yaml      leaf 0.2 m, L=3, sigma 0.1, sum reduction + regulariser
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

PRESETS = {
    "maicity": dict(tree_level_world=12, tree_level_feat=3, leaf_vox_size=0.2, sigma_sigmoid_m=0.05,
                    surface_sample_range_m=0.15, surface_sample_n=3, free_sample_n=3, free_sample_begin_ratio=0.3,
                    free_sample_end_dist_m=0.8, ekional_loss_on=False, weight_e=0.1, loss_reduction="mean",
                    pc_radius_m=50.0, min_range_m=1.5, street_len=100.0, turns=0, lr=0.01),
    "kitti": dict(tree_level_world=12, tree_level_feat=3, leaf_vox_size=0.3, sigma_sigmoid_m=0.1,
                  surface_sample_range_m=0.3, surface_sample_n=3, free_sample_n=3, free_sample_begin_ratio=0.3,
                  free_sample_end_dist_m=0.8, ekional_loss_on=True, weight_e=0.1, loss_reduction="mean",
                  pc_radius_m=50.0, min_range_m=3.0, street_len=600.0, turns=2, lr=0.01),
    "kitti_large": dict(tree_level_world=12, tree_level_feat=3, leaf_vox_size=0.3, sigma_sigmoid_m=0.1,
                        surface_sample_range_m=0.3, surface_sample_n=3, free_sample_n=3, free_sample_begin_ratio=0.3,
                        free_sample_end_dist_m=0.8, ekional_loss_on=True, weight_e=0.1, loss_reduction="mean",
                        pc_radius_m=50.0, min_range_m=3.0, street_len=8420.0, turns=-8, lr=0.01),
    "ncd": dict(tree_level_world=12, tree_level_feat=3, leaf_vox_size=0.2, sigma_sigmoid_m=0.1,
                surface_sample_range_m=0.3, surface_sample_n=3, free_sample_n=3, free_sample_begin_ratio=0.3,
                free_sample_end_dist_m=1.0, ekional_loss_on=False, weight_e=0.1, loss_reduction="sum",
                lambda_forget=1e4, pc_radius_m=25.0, min_range_m=1.5, street_len=40.0, turns=0, lr=0.01),
}


def make_config(kind: str, device="cuda", **over) -> SimpleNamespace:
    """Attribute bag with the names utils/config.py uses (so FeatureOctree / Decoder take it as-is)."""
    c = SimpleNamespace(
        feature_dim=8, feature_std=0.05, poly_int_on=True, geo_mlp_level=2, geo_mlp_hidden_dim=32,
        geo_mlp_bias_on=True, sem_mlp_level=2, sem_mlp_hidden_dim=32, sem_mlp_bias_on=True, sem_class_count=20,
        logistic_gaussian_ratio=0.55, lambda_forget=0.0, device=device, bs=4096, weight_decay=1e-7,
        mc_vis_level=1, pad_voxel=2, dtype=torch.float32, time_conditioned=False,  # utils/config.py:140-146,27
    )
    c.__dict__.update(PRESETS[kind])
    c.__dict__.update(over)
    c.scale = 1.0 / (c.leaf_vox_size * (2 ** (c.tree_level_world - 1)))  # utils/config.py:372-374
    c.sigma_sigmoid = c.logistic_gaussian_ratio * c.sigma_sigmoid_m * c.scale  # shine_batch.py:87
    return c


def _boxes(street_len: float, gen: torch.Generator, n=20):
    cx = torch.rand(n, generator=gen) * street_len
    cy = (torch.rand(n, generator=gen) * 2 - 1) * 6.0
    sx = torch.rand(n, generator=gen) * 3 + 1
    sy = torch.rand(n, generator=gen) * 2 + 1
    sz = torch.rand(n, generator=gen) * 2.5 + 0.5
    lo = torch.stack((cx - sx / 2, cy - sy / 2, torch.zeros(n)), 1)
    hi = torch.stack((cx + sx / 2, cy + sy / 2, sz), 1)
    return lo, hi


def cast_scan(origin, dirs, lo, hi, half_width=8.0, facade_h=10.0, max_range=50.0, min_range=1.5, kinds=False):
    """Analytic ray cast of one scan: ground z=0, facades y=+-half_width, axis-aligned boxes. -> hit points [M,3] (with kinds
    also what each ray met first, int64 [M] of GROUND / FACADE / BOX)."""
    o = origin
    big = torch.full((dirs.shape[0],), float("inf"), device=dirs.device)
    dz = dirs[:, 2]
    t = torch.where(dz < -1e-6, -o[2] / dz, big)
    t_ground = t
    for sgn in (-1.0, 1.0):
        dy = dirs[:, 1]
        tf = torch.where(dy * sgn > 1e-6, (sgn * half_width - o[1]) / dy, big)
        zf = o[2] + tf * dz
        tf = torch.where((zf >= 0) & (zf <= facade_h), tf, big)
        t = torch.minimum(t, tf)
    inv = 1.0 / torch.where(dirs.abs() < 1e-9, torch.full_like(dirs, 1e-9), dirs)
    t0 = (lo[None] - o[None, None]) * inv[:, None]
    t1 = (hi[None] - o[None, None]) * inv[:, None]
    tn = torch.minimum(t0, t1).amax(-1)
    tx = torch.maximum(t0, t1).amin(-1)
    tb = torch.where((tx >= tn) & (tn > 0), tn, torch.full_like(tn, float("inf"))).amin(-1)
    t_flat = t
    t = torch.minimum(t, tb)
    ok = (t < max_range) & (t > min_range)
    if kinds:
        kind = torch.where(tb < t_flat, BOX, torch.where(t_flat < t_ground, FACADE, GROUND))
        return o[None] + t[ok, None] * dirs[ok], kind[ok]
    return o[None] + t[ok, None] * dirs[ok]


def sensor_dirs(beams=64, azimuths=450, fov=(-24.8, 2.0), device="cpu"):
    el = torch.deg2rad(torch.linspace(fov[0], fov[1], beams, device=device))
    az = torch.linspace(0, 2 * math.pi, azimuths + 1, device=device)[:-1]
    ce, se = torch.cos(el)[:, None], torch.sin(el)[:, None]
    d = torch.stack((ce * torch.cos(az)[None], ce * torch.sin(az)[None], se.expand(-1, azimuths)), -1)
    return d.reshape(-1, 3)


def sample_rays(points, origin, cfg, gen=None):
    """Per-ray samples in the [-1,1] space: utils/data_sampler.py:18-139 (labels/normals off). Ray-major order."""
    dev = points.device
    ns, nf = cfg.surface_sample_n, cfg.free_sample_n
    S = ns + nf
    rel = points - origin
    m = rel.shape[0]
    dist = torch.linalg.norm(rel, dim=1, keepdim=True)
    r_s = cfg.surface_sample_range_m * cfg.scale
    disp_s = (torch.rand(m * ns, 1, device=dev, generator=gen) - 0.5) * 2 * r_s
    ratio_s = disp_s / dist.repeat(ns, 1) + 1.0
    rd = dist.repeat(nf, 1)
    hi = cfg.free_sample_end_dist_m * cfg.scale / rd + 1.0
    lo = cfg.free_sample_begin_ratio
    ratio_f = torch.rand(m * nf, 1, device=dev, generator=gen) * (hi - lo) + lo
    disp_f = (ratio_f - 1.0) * rd
    disp = torch.cat((disp_s, disp_f), 0)
    ratio = torch.cat((ratio_s, ratio_f), 0)
    xyz = rel.repeat(S, 1) * ratio + origin
    w = torch.ones(m * S, device=dev)
    w[m * ns:] = -1.0
    xyz = xyz.reshape(S, -1, 3).transpose(0, 1).reshape(-1, 3)
    label = disp.squeeze(1).reshape(S, -1).transpose(0, 1).reshape(-1)
    w = w.reshape(S, -1).transpose(0, 1).reshape(-1)
    return xyz.contiguous(), label.contiguous(), w.contiguous()


def trajectory(street_len: float, turns: int):
    """The sensor path as axis-aligned segments [(x0, y0, heading_deg, length)].
    turns == 0: one straight street; turns > 0: a polyline with that many 90-degree turns (alternating left/right, equal
    legs — SURVEY.md §8d's KITTI-like "600 m polyline with two turns"); turns < 0: a serpentine of |turns| long rows
    joined by 60 m connectors (a large map that still fits the [-1,1] cube)."""
    if turns == 0:
        return [(0.0, 0.0, 0.0, float(street_len))]
    segs, x, y = [], 0.0, 0.0
    if turns > 0:
        leg = street_len / (turns + 1)
        for k in range(turns + 1):
            h = 0.0 if k % 2 == 0 else 90.0
            segs.append((x, y, h, leg))
            x, y = (x + leg, y) if h == 0.0 else (x, y + leg)
        return segs
    rows, gap = -turns, 60.0
    row_len = (street_len - gap * (rows - 1)) / rows
    for k in range(rows):
        h = 0.0 if k % 2 == 0 else 180.0
        segs.append((x, y, h, row_len))
        x = x + row_len if h == 0.0 else x - row_len
        if k + 1 < rows:
            segs.append((x, y, 90.0, gap))
            y += gap
    return segs


def _rot(heading_deg: float, device):
    c, s_ = round(math.cos(math.radians(heading_deg))), round(math.sin(math.radians(heading_deg)))
    return torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]], device=device)


def make_frames(cfg, frames=100, beams=64, azimuths=450, seed=42, device="cuda"):
    """Yield per-frame (coord, sdf_label, weight) in the scaled space, like LiDARDataset.process_frame (:115-233).
    Each segment of the trajectory is a street canyon in its own frame (ground, two facades, boxes); a scan is ray-cast
    against the canyon of the segment the sensor is in."""
    gen = torch.Generator(device=device).manual_seed(seed + 1) if str(device) != "cpu" else \
        torch.Generator().manual_seed(seed + 1)
    for hits, origin, shift in make_scans(cfg, frames, beams, azimuths, seed, device):
        yield sample_rays((hits - shift) * cfg.scale, (origin - shift) * cfg.scale, cfg, gen)


def make_scans(cfg, frames=100, beams=64, azimuths=450, seed=42, device="cuda", kinds=False):
    """Yield per-frame (hit points [M,3], sensor origin [3], map centre [3]) in metres: the scans make_frames samples (with kinds
    a fourth element: what each point lies on, cast_scan's kinds)."""
    g = torch.Generator().manual_seed(seed)
    segs = trajectory(cfg.street_len, getattr(cfg, "turns", 0))
    boxes = []
    for (_, _, _, length) in segs:
        lo, hi = _boxes(length, g, n=max(4, int(20 * length / 100.0)) if len(segs) > 1 else 20)
        boxes.append((lo.to(device), hi.to(device)))
    dirs = sensor_dirs(beams, azimuths, device=device)
    total = sum(sg[3] for sg in segs)
    step = total / max(frames, 1)
    # centre the map on the origin so it fits the [-1,1] cube (the reference shifts by the first pose, first_frame_ref)
    ends = [(x0 + math.cos(math.radians(h)) * ln, y0 + math.sin(math.radians(h)) * ln) for (x0, y0, h, ln) in segs]
    xs = [sg[0] for sg in segs] + [e[0] for e in ends]
    ys = [sg[1] for sg in segs] + [e[1] for e in ends]
    shift = torch.tensor([(min(xs) + max(xs)) / 2, (min(ys) + max(ys)) / 2, 0.0], device=device)
    k, acc = 0, 0.0
    rots = [(_rot(sg[2], device), _rot(-sg[2], device)) for sg in segs]
    for f in range(frames):
        s_ = f * step
        while k + 1 < len(segs) and s_ >= acc + segs[k][3]:
            acc += segs[k][3]
            k += 1
        x0, y0, _, _ = segs[k]
        R, Rinv = rots[k]
        lo, hi = boxes[k]
        local_origin = torch.tensor([s_ - acc, 0.3 * math.sin(0.2 * f), 1.8], device=device)
        hits = cast_scan(local_origin, dirs @ Rinv.T if len(segs) > 1 else dirs, lo, hi, max_range=cfg.pc_radius_m,
                         min_range=cfg.min_range_m, kinds=kinds)
        if kinds:
            hits, kind = hits
        base = torch.tensor([x0, y0, 0.0], device=device)
        if len(segs) > 1:
            hits = hits @ R.T + base
            origin = local_origin @ R.T + base
        else:
            origin = local_origin
        if kinds:
            yield hits, origin, shift, kind
        else:
            yield hits, origin, shift


# the labelled drive's label definition, in SemanticKITTI's id ranges (ids >= 100 move, 1 is the outlier id): raw id -> class, and
# class -> (r, g, b).  DRIVE_RAW_IDS: what ground, facade and boxes carry; DRIVE_UNMAPPED_ID is in neither dict.
DRIVE_RAW_IDS = {0: 40, 1: 50, 2: 10}  # GROUND, FACADE, BOX (the kinds of cast_scan / cast_depth)
DRIVE_LABEL_MAP = {0: 0, 1: 0, 10: 1, 40: 2, 44: 2, 50: 3, 51: 4, 252: 1, 254: 5}
DRIVE_COLOR_MAP = {0: (255, 255, 255), 1: (100, 150, 245), 2: (255, 0, 255), 3: (255, 200, 0), 4: (255, 120, 50), 5: (255, 30, 30)}
DRIVE_UNMAPPED_ID = 77


def write_kitti_drive(folder, cfg, frames=6, beams=64, azimuths=450, seed=42, device="cpu", yaw_per_frame=0.05, labels=False,
                      unmapped=0):
    """Write make_scans' drive as a KITTI-format folder — velodyne/%06d.bin (float32 x, y, z, intensity in the SENSOR frame),
    poses.txt (camera-frame poses, 12 values per line) and calib.txt (Tr: lidar -> camera) — the input LiDARDataset reads.
    The sensor yaws by `yaw_per_frame` rad per frame, so the poses carry a rotation.  Returns a SimpleNamespace with pc_path,
    pose_path, calib_path and lidar_poses (the [4,4] float64 lidar-to-world poses the files encode: Tr^-1 . P . Tr).
    labels=True: also labels/%06d.label, one uint32 per point in SemanticKITTI's layout — the lower 16 bits the raw semantic id
    of what the point lies on (DRIVE_RAW_IDS), the upper 16 a random instance id — with a seeded sprinkle of special ids: about
    2 % moving (252, 254), 1 % outlier (1), 1 % unlabeled (0), 2 % a second ground id (44) and a second facade id (51), and
    `unmapped` points per frame (default none) with DRIVE_UNMAPPED_ID, an id the map does not hold.  The result then also carries
    label_path, label_map (raw id -> class) and color_map (class -> (r, g, b)).  The scans are the same bytes with and without
    labels."""
    import os

    import numpy as np

    pc_path = os.path.join(folder, "velodyne")
    os.makedirs(pc_path, exist_ok=True)
    label_path = os.path.join(folder, "labels")
    if labels:
        os.makedirs(label_path, exist_ok=True)
        rng = np.random.default_rng(seed + 7)
    # KITTI's axis convention (camera x = -lidar y, y = -lidar z, z = lidar x) plus a small lever arm
    Tr = np.array([[0.0, -1.0, 0.0, 0.05], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27], [0.0, 0.0, 0.0, 1.0]])
    Tr_inv = np.linalg.inv(Tr)
    poses, lines = [], []
    for f, scan_f in enumerate(make_scans(cfg, frames, beams, azimuths, seed, device, kinds=labels)):
        hits, origin, shift = scan_f[:3]
        if labels:
            kind = scan_f[3].cpu().numpy()
            raw = np.select([kind == k for k in DRIVE_RAW_IDS], list(DRIVE_RAW_IDS.values())).astype(np.uint32)
            u = rng.random(len(raw))
            for lo_u, hi_u, ids in ((0.00, 0.02, (252, 254)), (0.02, 0.03, (1,)), (0.03, 0.04, (0,)), (0.04, 0.06, (44, 51))):
                pick = np.flatnonzero((u >= lo_u) & (u < hi_u))
                raw[pick] = np.asarray(ids, np.uint32)[rng.integers(0, len(ids), len(pick))]
            if unmapped:
                raw[rng.choice(len(raw), size=min(int(unmapped), len(raw)), replace=False)] = DRIVE_UNMAPPED_ID
            instance = rng.integers(1, 1 << 16, len(raw)).astype(np.uint32)
            ((instance << 16) | raw).astype(np.uint32).tofile(os.path.join(label_path, "%06d.label" % f))
        yaw = yaw_per_frame * f
        W = np.eye(4)
        W[:3, :3] = [[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
        W[:3, 3] = (origin - shift).double().cpu().numpy()
        local = ((hits - shift).double().cpu().numpy() - W[:3, 3]) @ W[:3, :3]  # R^T (p - t)
        scan = np.zeros((local.shape[0], 4), dtype=np.float32)
        scan[:, :3] = local
        scan.tofile(os.path.join(pc_path, "%06d.bin" % f))
        P = Tr @ W @ Tr_inv
        lines.append(" ".join(repr(float(v)) for v in P[:3].reshape(-1)))
        poses.append(Tr_inv @ (_pose_from_line(lines[-1]) @ Tr))  # (as a reader of the file computes it)
    pose_path, calib_path = os.path.join(folder, "poses.txt"), os.path.join(folder, "calib.txt")
    with open(pose_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(calib_path, "w") as fh:
        for key in ("P0", "P1", "P2", "P3"):
            fh.write("%s: 1.0 0.0 0.0 0.0 0.0 1.0 0.0 0.0 0.0 0.0 1.0 0.0\n" % key)
        fh.write("Tr: " + " ".join(repr(float(v)) for v in Tr[:3].reshape(-1)) + "\n")
    drive = SimpleNamespace(pc_path=pc_path, pose_path=pose_path, calib_path=calib_path, lidar_poses=poses, frames=frames)
    if labels:
        drive.__dict__.update(label_path=label_path, label_map=dict(DRIVE_LABEL_MAP), color_map=dict(DRIVE_COLOR_MAP))
    return drive


def dataset_config(kind, drive, device="cuda", **over):
    """make_config(kind) plus the fields LiDARDataset reads (utils/config.py's names and defaults, the preset's crop radius and
    minimum range), pointed at a write_kitti_drive folder (a labelled one also sets label_path and the drive's label / colour maps)"""
    c = make_config(kind, device=device)
    c.__dict__.update(
        pc_path=drive.pc_path, pose_path=drive.pose_path, calib_path=drive.calib_path, first_frame_ref=False, begin_frame=0,
        end_frame=drive.frames - 1, every_frame=1, seed=42, pc_count_gpu_limit=500, global_shift_default=0.0,
        min_range=c.min_range_m, pc_radius=c.pc_radius_m, min_z=-10.0, max_z=30.0, rand_downsample=False, vox_down_m=0.05,
        rand_down_r=1.0, map_vox_down_m=0.2, estimate_normal=False, filter_noise=False, semantic_on=False,
        behind_dropoff_on=False, octree_from_surface_samples=True, clearance_dist_m=0.3, clearance_sample_n=0,
        continual_learning_reg=False, window_replay_on=False, window_radius=50.0, ray_loss=False)
    if getattr(drive, "label_path", None):  # a labelled drive (write_kitti_drive(labels=True)); semantic_on stays the caller's choice
        c.__dict__.update(label_path=drive.label_path, sem_label_map=drive.label_map, sem_color_map=drive.color_map,
                          filter_moving_object=True)
    c.__dict__.update(over)
    return c


def _pose_from_line(line):
    import numpy as np

    P = np.eye(4)
    P[:3, :] = np.array([float(v) for v in line.split()]).reshape(3, 4)
    return P


def build_workload(kind="maicity", frames=100, device="cuda", seed=42, beams=64, azimuths=450, **over):
    """Pool + octree + decoder for a preset: what shine_batch.py:69-95 has in hand when the hot loop starts."""
    import hashlib
    import os

    from .decoder import Decoder
    from .feature_octree import FeatureOctree

    cfg = make_config(kind, device=device, **over)
    # measurement aid: SHINE_WORKLOAD_CACHE=<dir> keeps the built workload on disk, so that the profiler passes of
    # tools/collect_profiles.sh (one process per counter group) build a large map once instead of once per pass
    cache = os.environ.get("SHINE_WORKLOAD_CACHE")
    path = None
    if cache:
        key = repr((kind, frames, seed, beams, azimuths, sorted(over.items())))
        path = os.path.join(cache, "workload_%s.pt" % hashlib.sha1(key.encode()).hexdigest()[:16])
        if os.path.isfile(path):
            blob = torch.load(path, weights_only=False)
            octree, decoder = blob["octree"], blob["decoder"].to(device)
            pool = SimpleNamespace(**{k: v.to(device) for k, v in blob["pool"].items()})
            return SimpleNamespace(cfg=cfg, octree=octree, decoder=decoder, pool=pool)
    torch.manual_seed(seed)
    octree = FeatureOctree(cfg)
    decoder = Decoder(cfg)
    coords, labels, weights = [], [], []
    for c, l, w in make_frames(cfg, frames, beams, azimuths, seed, device):
        octree.update(c[w > 0], False)  # octree_from_surface_samples: True (lidar_dataset.py:213-215)
        coords.append(c)
        labels.append(l)
        weights.append(w)
    pool = SimpleNamespace(coord=torch.cat(coords), sdf_label=torch.cat(labels), weight=torch.cat(weights))
    if path is not None:
        os.makedirs(cache, exist_ok=True)
        torch.save(dict(octree=octree, decoder=decoder, pool={k: v.cpu() for k, v in vars(pool).items()}), path)
    return SimpleNamespace(cfg=cfg, octree=octree, decoder=decoder, pool=pool)


def draw_batch(pool, n, gen=None):
    """LiDARDataset.get_batch, point-sample branch (dataset/lidar_dataset.py:430-450)."""
    idx = torch.randint(0, pool.sdf_label.shape[0], (n,), device=pool.sdf_label.device, generator=gen)
    return pool.coord[idx, :], pool.sdf_label[idx], pool.weight[idx]


def semantic_labels(coord, weight, n_class=21, cell=0.02):
    """Class labels for samples, the way dataSampler.sample assigns them (utils/data_sampler.py:59,70): a surface sample
    (weight > 0) carries the class of the point it was drawn around — here a class in 1..n_class-1 that is a fixed function of
    the sample's cell of size `cell`, so any batch drawn from a pool is labelled consistently — and clearance / free-space
    samples carry 0.  int64 [N] on coord's device."""
    q = torch.floor(coord.detach() / cell).to(torch.int64)
    h = (q[:, 0] * 73856093) ^ (q[:, 1] * 19349663) ^ (q[:, 2] * 83492791)
    lab = 1 + torch.remainder(h, n_class - 1)
    return torch.where(weight > 0, lab, torch.zeros_like(lab))


# ---- a synthetic RGB-D drive (config/rgbd/*.yaml: Neural-RGBD / Replica rooms) ---------------------------------------------------
PRESETS["rgbd"] = dict(tree_level_world=12, tree_level_feat=4, leaf_vox_size=0.02, sigma_sigmoid_m=0.02,
                       surface_sample_range_m=0.05, surface_sample_n=3, free_sample_n=3, free_sample_begin_ratio=0.5,
                       free_sample_end_dist_m=0.3, ekional_loss_on=False, weight_e=0.1, loss_reduction="mean",
                       pc_radius_m=5.0, min_range_m=0.2, street_len=8.0, turns=0, lr=0.01)

ROOM = dict(half_width=2.5, facade_h=3.0)  # the street canyon of cast_scan at the size of a room
GROUND, FACADE, BOX, MISS = 0, 1, 2, 3  # what a pixel's ray meets first


def room_boxes(length=8.0, n=8, seed=42):
    """n axis-aligned boxes standing on the ground of a room `length` long -> (lo [n,3], hi [n,3]) float64 numpy"""
    import numpy as np

    g = torch.Generator().manual_seed(seed)
    r = torch.rand((5, n), generator=g, dtype=torch.float64).numpy()
    cx, cy = 1.0 + r[0] * (length - 2.0), (r[1] * 2 - 1) * 1.6
    sx, sy, sz = 0.3 + 0.5 * r[2], 0.3 + 0.5 * r[3], 0.3 + 0.7 * r[4]
    return np.stack((cx - sx / 2, cy - sy / 2, np.zeros(n)), 1), np.stack((cx + sx / 2, cy + sy / 2, sz), 1)


def cast_depth(origin, dirs, lo, hi, half_width=ROOM["half_width"], facade_h=ROOM["facade_h"]):
    """cast_scan's intersection maths per ray, in float64 numpy, WITHOUT its range cut: the ray parameter t of the first surface
    along origin + t * dirs (inf: nothing is met) and which kind it is (GROUND / FACADE / BOX / MISS).  dirs need not be unit
    vectors: with the pixel directions ((u - cx) / fx, (v - cy) / fy, 1) rotated into the world, t IS the z-depth."""
    import numpy as np

    o = np.asarray(origin, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    inf = np.full(d.shape[0], np.inf)
    dz = d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dz < -1e-6, -o[2] / dz, inf)
        kind = np.where(np.isfinite(t), GROUND, MISS)
        for sgn in (-1.0, 1.0):
            dy = d[:, 1]
            tf = np.where(dy * sgn > 1e-6, (sgn * half_width - o[1]) / dy, inf)
            zf = o[2] + tf * dz
            tf = np.where((zf >= 0) & (zf <= facade_h), tf, inf)
            kind = np.where(tf < t, FACADE, kind)
            t = np.minimum(t, tf)
        inv = 1.0 / np.where(np.abs(d) < 1e-9, 1e-9, d)
        t0 = (lo[None] - o[None, None]) * inv[:, None]
        t1 = (hi[None] - o[None, None]) * inv[:, None]
        tn = np.minimum(t0, t1).max(-1)
        tx = np.maximum(t0, t1).min(-1)
        tb = np.where((tx >= tn) & (tn > 0), tn, np.inf).min(-1)
    kind = np.where(tb < t, BOX, kind)
    return np.minimum(t, tb), kind


def camera_pose(position, yaw, pitch_down):
    """sensor-to-world pose [4,4] of a camera at `position` heading `yaw` (rad, about world z) and looking `pitch_down` rad below
    the horizon.  The sensor frame is the converter's flipped camera frame (x right, y up, z backwards: dataset/
    rgbd_to_kitti_format.py:42), so the camera looks along the sensor's -z."""
    import numpy as np

    fwd = np.array([math.cos(yaw) * math.cos(pitch_down), math.sin(yaw) * math.cos(pitch_down), -math.sin(pitch_down)])
    right = np.array([math.sin(yaw), -math.cos(yaw), 0.0])
    up = np.cross(right, fwd)
    W = np.eye(4)
    W[:3, 0], W[:3, 1], W[:3, 2], W[:3, 3] = right, up, -fwd, position
    return W


def write_rgbd_drive(folder, cfg=None, frames=6, width=160, height=120, focal=130.0, fmt="npy", seed=42, max_depth_m=5.0,
                     max_range_m=8.0, depth_scale=1000.0, yaw_per_frame=0.12, pitch_down=0.35, step_m=0.25):
    """Write a pinhole camera's pass through a room (ground, two facades, boxes: cast_depth) as an RGB-D folder in the Neural-RGBD
    layout — depth/%06d.npy or .png (uint16 millimetres; 0 where the ray meets nothing or only beyond max_range_m, which lies
    beyond max_depth_m so that some pixels carry a depth the reader must drop), focal.txt (one focal length; cx = (W - 1) / 2,
    cy = (H - 1) / 2) and poses.txt (four lines per sensor-to-world matrix).  The camera advances step_m per frame, sways, and
    turns by yaw_per_frame.  `cfg` is accepted for symmetry with write_kitti_drive (not read).  Returns a SimpleNamespace with
    depth_path, intrinsic_path, pose_path, poses ([4,4] float64 as a reader of the file gets them), frames, width, height, focal,
    depth_scale, max_depth_m, exact_depths ([H,W] float64 z-depths before rounding, inf = nothing met), kinds ([H,W] of GROUND /
    FACADE / BOX / MISS), boxes (lo, hi) and the ROOM sizes."""
    import os

    import numpy as np

    if fmt not in ("npy", "png"):
        raise ValueError("write_rgbd_drive: fmt must be 'npy' or 'png'")
    depth_path = os.path.join(folder, "depth")
    os.makedirs(depth_path, exist_ok=True)
    lo, hi = room_boxes(seed=seed)
    cx, cy = (width - 1.0) / 2.0, (height - 1.0) / 2.0
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    cam_dirs = np.stack(((u - cx) / focal, (v - cy) / focal, np.ones_like(u)), -1).reshape(-1, 3)
    flipped = cam_dirs * np.array([1.0, -1.0, -1.0])  # the flip: camera frame -> sensor frame
    poses, lines, exact, kinds = [], [], [], []
    for f in range(frames):
        W = camera_pose([0.4 + step_m * f, 0.3 * math.sin(0.4 * f), 1.2], -0.3 + yaw_per_frame * f, pitch_down)
        text = "\n".join(" ".join(repr(float(x)) for x in row) for row in W)
        W = np.array([[float(x) for x in row.split()] for row in text.split("\n")])  # (as a reader of the file gets it)
        t, kind = cast_depth(W[:3, 3], flipped @ W[:3, :3].T, lo, hi)
        raw = np.where(t < max_range_m, np.rint(t * depth_scale), 0.0).astype(np.uint16).reshape(height, width)
        name = os.path.join(depth_path, "%06d.%s" % (f, fmt))
        if fmt == "npy":
            np.save(name, raw)
        else:
            from PIL import Image

            Image.fromarray(raw).save(name)
        poses.append(W)
        lines.append(text)
        exact.append(t.reshape(height, width))
        kinds.append(kind.reshape(height, width))
    intrinsic_path, pose_path = os.path.join(folder, "focal.txt"), os.path.join(folder, "poses.txt")
    with open(intrinsic_path, "w") as fh:
        fh.write(repr(float(focal)) + "\n")
    with open(pose_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return SimpleNamespace(depth_path=depth_path, intrinsic_path=intrinsic_path, pose_path=pose_path, poses=poses, frames=frames,
                           width=width, height=height, focal=float(focal), depth_scale=float(depth_scale),
                           max_depth_m=float(max_depth_m), exact_depths=exact, kinds=kinds, boxes=(lo, hi), room=dict(ROOM))


def rgbd_config(kind, drive, device="cuda", **over):
    """dataset_config's sibling for RGBDDataset: make_config(kind) ("rgbd": the process / sampler / octree values of
    config/rgbd/rgbd_batch.yaml) plus the fields RGBDDataset reads, pointed at a write_rgbd_drive folder"""
    c = make_config(kind, device=device)
    c.__dict__.update(
        depth_path=drive.depth_path, intrinsic_path=drive.intrinsic_path, is_focal_file=True, pose_path=drive.pose_path,
        pose_kitti_format=False, max_depth_m=drive.max_depth_m, first_frame_ref=False, begin_frame=0, end_frame=drive.frames - 1,
        every_frame=1, seed=42, pc_count_gpu_limit=500, global_shift_default=0.0, min_range=c.min_range_m, pc_radius=c.pc_radius_m,
        min_z=-10.0, max_z=30.0, rand_downsample=False, vox_down_m=0.01, rand_down_r=0.2, map_vox_down_m=0.05,
        estimate_normal=False, filter_noise=False, semantic_on=False, behind_dropoff_on=False, octree_from_surface_samples=True,
        clearance_dist_m=0.3, clearance_sample_n=0, continual_learning_reg=False, window_replay_on=False, window_radius=50.0,
        ray_loss=False)
    c.__dict__.update(over)
    return c
