"""CPU suite of shine_mapping_amd/dataset.py: the host logic of LiDARDataset (pose files, frame selection, file order, refusals),
the argument checks of the three frame entry points (csrc/shine_frame.hip) and the self-checks of tests/frame_oracle.py on
hand-made clouds.  Nothing here needs a GPU; the device stages are in tests/test_gpu_dataset.py."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frame_oracle as fo


def make_cfg(tmp_path, n_files=5, **over):
    pc = tmp_path / "velodyne"
    pc.mkdir(exist_ok=True)
    for k in range(n_files):
        (pc / ("%d.bin" % k)).write_bytes(b"")
    poses = tmp_path / "poses.txt"
    if not poses.exists():
        lines = []
        for k in range(n_files):
            c, s = math.cos(0.1 * k), math.sin(0.1 * k)
            lines.append(" ".join(repr(v) for v in (c, -s, 0.0, 1.5 * k, s, c, 0.0, -0.25 * k, 0.0, 0.0, 1.0, 0.125 * k)))
        poses.write_text("\n".join(lines) + "\n")
    cfg = SimpleNamespace(
        device="cuda", dtype=torch.float32, pc_path=str(pc), pose_path=str(poses), calib_path="", first_frame_ref=True,
        begin_frame=0, end_frame=n_files - 1, every_frame=1, pc_count_gpu_limit=500, global_shift_default=0.0, seed=42,
        min_range=1.5, pc_radius=25.0, min_z=-3.0, max_z=30.0, rand_downsample=False, vox_down_m=0.05, rand_down_r=1.0,
        map_vox_down_m=0.2, estimate_normal=False, filter_noise=False, semantic_on=False, behind_dropoff_on=False,
        octree_from_surface_samples=True, surface_sample_range_m=0.3, surface_sample_n=3, free_sample_begin_ratio=0.3,
        free_sample_end_dist_m=1.0, free_sample_n=3, clearance_dist_m=0.3, clearance_sample_n=0, continual_learning_reg=False,
        window_replay_on=False, window_radius=50.0, ray_loss=False, bs=256, scale=0.01)
    cfg.__dict__.update(over)
    return cfg


# ---- the oracle's own checks ------------------------------------------------------------------------------------------------------
def test_oracle_filter_keeps_the_faces_and_min_range_and_drops_min_z():
    R, min_z, max_z, min_range = 25.0, -3.0, 30.0, 2.5
    pts = np.array([
        [25.0, 0.0, 0.0],    # on the +x face: kept
        [-25.0, 25.0, 1.0],  # on an edge: kept
        [3.0, 4.0, 30.0],    # on the top face: kept
        [25.000001, 0.0, 0.0],  # just outside
        [2.5, 0.0, 0.0],     # exactly min_range: kept
        [1.5, 2.0, 0.0],     # |p| = 2.5 exactly (3-4-5 triangle halved): kept
        [2.4999, 0.0, 0.0],  # inside min_range: dropped
        [5.0, 5.0, -3.0],    # exactly min_z: dropped (z > min_z is strict)
        [5.0, 5.0, -2.999],  # above it: kept
        [0.0, 0.0, 31.0],    # above the box
    ])
    assert fo.filter_mask(pts, min_z, max_z, min_range, R).tolist() == [True, True, True, False, True, True, False, False, True, False]


def test_oracle_voxel_rule_on_a_hand_made_cloud():
    # min bound (0, 0, 0), voxel 1: origin -0.5, so [0, 0.5) is voxel 0 and [0.5, 1.5) voxel 1 on every axis
    pts = np.array([[0.0, 0.0, 0.0], [0.4, 0.0, 0.0], [0.5, 0.0, 0.0], [1.4, 0.2, 0.0], [0.0, 0.6, 0.0], [0.0, 0.0, 1.6]])
    means, keys = fo.voxel_down(pts, 1.0)
    assert keys.tolist() == [0, 2, 1 << 21, 1 << 42]  # (0,0,0), (0,0,2), (0,1,0), (1,0,0): ascending keys
    assert np.allclose(means, [[0.2, 0.0, 0.0], [0.0, 0.0, 1.6], [0.0, 0.6, 0.0], [0.95, 0.1, 0.0]], rtol=1e-15)
    assert fo.voxel_down(np.zeros((0, 3)), 1.0)[0].shape == (0, 3)


def test_oracle_transform_frame_and_window():
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [10.0, 20.0, 30.0]
    assert np.array_equal(fo.transform([[1.0, 2.0, 3.0]], T), [[8.0, 21.0, 33.0]])
    cfg = SimpleNamespace(min_z=-3.0, max_z=30.0, min_range=1.0, pc_radius=25.0, vox_down_m=1.0, map_vox_down_m=4.0)
    raw = np.array([[2.0, 0.0, 0.0], [2.1, 0.0, 0.0], [0.5, 0.0, 0.0], [4.0, 0.0, 0.0], [40.0, 0.0, 0.0]], np.float32)
    fr = fo.frame(raw, T, cfg)
    assert fr["kept"].tolist() == [0, 1, 3] and len(fr["sensor"]) == 2 and len(fr["cur"]) == 1
    assert np.allclose(fr["world"][0], fo.transform([[np.float32(2.0) / 2 + np.float64(np.float32(2.1)) / 2, 0, 0]], T)[0])
    assert np.allclose(fr["lo"], fr["hi"])
    keep, dist = fo.window_mask(np.array([[0.3, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.2]], np.float32), [0.0, 0.0, 0.0], 0.5)
    assert keep.tolist() == [True, False, True] and dist.dtype == np.float32


# ---- poses and the constructor ------------------------------------------------------------------------------------------------------
def test_poses_ref_from_a_kitti_pose_file_with_calibration(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset

    pose_text = ("1 0 0 0 0 1 0 0 0 0 1 0\n"
                 "0.9950041652780258 0 0.09983341664682815 0.3 0 1 0 -0.02 -0.09983341664682815 0 0.9950041652780258 2.0\n"
                 "0.9800665778412416 0 0.19866933079506122 0.9 0 1 0 -0.05 -0.19866933079506122 0 0.9800665778412416 4.1\n")
    calib_text = ("P0: 7.0e+02 0 6.0e+02 0 0 7.0e+02 1.8e+02 0 0 0 1 0\n"
                  "Tr: 4.276802385584e-04 -9.999672484946e-01 -8.084491683471e-03 -1.198459927713e-02 "
                  "-7.210626507497e-03 8.081198471645e-03 -9.999413164504e-01 -5.403984729748e-02 "
                  "9.999738645903e-01 4.859485810390e-04 -7.206933692422e-03 -2.921968648686e-01\n")
    (tmp_path / "poses.txt").write_text(pose_text)
    (tmp_path / "calib.txt").write_text(calib_text)
    cfg = make_cfg(tmp_path, n_files=3, calib_path=str(tmp_path / "calib.txt"))
    ds = LiDARDataset(cfg)
    want_w = fo.kitti_poses(pose_text, calib_text)
    inv0 = np.linalg.inv(want_w[0])
    assert np.allclose(ds.begin_pose_inv, inv0, rtol=1e-13, atol=1e-15)
    for k in range(3):
        assert np.allclose(ds.poses_ref[k], inv0 @ want_w[k], rtol=1e-12, atol=1e-14)
    assert np.allclose(ds.poses_ref[0], np.eye(4), atol=1e-14)
    assert ds.used_pc_count == 3 and ds.total_pc_count == 3 and len(ds) == 0
    # without a calib path Tr is the identity; first_frame_ref off: the world frame shifted by global_shift_default in z
    cfg2 = make_cfg(tmp_path, n_files=3, first_frame_ref=False, global_shift_default=0.17241)
    ds2 = LiDARDataset(cfg2)
    plain = fo.kitti_poses(pose_text)
    shift = np.eye(4)
    shift[2, 3] = 0.17241
    for k in range(3):
        assert np.allclose(ds2.poses_ref[k], shift @ plain[k], rtol=1e-13, atol=1e-15)


def test_csv_poses_keep_the_reference_quaternion_order(tmp_path):
    """the reference passes (qx, qy, qz, qw) to Quaternion(array), which reads (w, x, y, z): a file whose qx column holds
    cos(a/2) and whose qy column holds sin(a/2) therefore yields a rotation by `a` about x"""
    from shine_mapping_amd.dataset import LiDARDataset, quaternion_rotation_matrix

    a = 0.7
    rows = ["ts,tx,ty,tz,qx,qy,qz,qw", "0.0,1.0,2.0,3.0,1.0,0.0,0.0,0.0",
            "0.1,1.5,2.5,3.5,%r,%r,0.0,0.0" % (math.cos(a / 2), math.sin(a / 2)),
            "0.2,0.0,0.0,0.0,0.0,0.0,0.0,2.0"]  # (w, x, y, z) = (0, 0, 0, 2): normalised, a half turn about z
    (tmp_path / "odom.csv").write_text("\n".join(rows) + "\n")
    cfg = make_cfg(tmp_path, n_files=3, pose_path=str(tmp_path / "odom.csv"), first_frame_ref=False)
    ds = LiDARDataset(cfg)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    assert np.allclose(ds.poses_ref[0], [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], atol=1e-15)
    assert np.allclose(ds.poses_ref[1][:3, :3], Rx, atol=1e-15) and np.allclose(ds.poses_ref[1][:3, 3], [1.5, 2.5, 3.5])
    assert np.allclose(ds.poses_ref[2][:3, :3], np.diag([-1.0, -1.0, 1.0]), atol=1e-15)
    R = quaternion_rotation_matrix(0.3, -0.4, 0.5, 0.7)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1.0) < 1e-14
    with pytest.raises(ValueError, match="pose file format"):
        LiDARDataset(make_cfg(tmp_path, n_files=3, pose_path=str(tmp_path / "odom.json")))


def test_frame_selection_natural_order_and_the_cpu_pool_rule(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset, natural_key

    cfg = make_cfg(tmp_path, n_files=12, begin_frame=2, end_frame=9, every_frame=3)
    ds = LiDARDataset(cfg)
    assert ds.pc_filenames == ["%d.bin" % k for k in range(12)]  # 1, 2, ... 9, 10, 11 — not 1, 10, 11, 2
    assert sorted(["10.bin", "9.bin", "scan_2.ply", "scan_10.ply", "1.bin"], key=natural_key) == \
        ["1.bin", "9.bin", "10.bin", "scan_2.ply", "scan_10.ply"]
    assert ds.used_pc_count == 3  # frames 3, 6, 9
    plain = fo.kitti_poses(open(cfg.pose_path).read())
    inv3 = np.linalg.inv(plain[3])
    assert np.allclose(ds.begin_pose_inv, inv3, rtol=1e-13, atol=1e-15)
    for k in range(12):
        want = inv3 @ plain[k] if k in (3, 6, 9) else plain[k]
        assert np.allclose(ds.poses_ref[k], want, rtol=1e-12, atol=1e-14)
    assert ds.pool_device == "cuda" and not ds.to_cpu
    assert ds.ray_sample_count == 6 and ds.coord_pool.shape == (0, 3) and ds.time_pool.shape == (0,)
    few = dict(begin_frame=0, end_frame=11, every_frame=1, pc_count_gpu_limit=5)
    assert LiDARDataset(make_cfg(tmp_path, n_files=12, **few)).pool_device == "cpu"
    assert LiDARDataset(make_cfg(tmp_path, n_files=12, window_replay_on=True, **few)).pool_device == "cuda"
    assert LiDARDataset(make_cfg(tmp_path, n_files=12, continual_learning_reg=True, **few)).pool_device == "cuda"


def test_unsupported_options_are_refused_by_name(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset

    for name in ("estimate_normal", "filter_noise", "semantic_on", "behind_dropoff_on"):
        with pytest.raises(NotImplementedError, match=name):
            LiDARDataset(make_cfg(tmp_path, **{name: True}))
    ds = LiDARDataset(make_cfg(tmp_path))
    with pytest.raises(NotImplementedError, match="sapce_carving_sample"):
        ds.sapce_carving_sample(None, None, 10, 0.5, 0.1)
    with pytest.raises(NotImplementedError, match=r"\.pcd"):
        ds.read_point_cloud(str(tmp_path / "scan.pcd"))
    with pytest.raises(ValueError, match="format"):
        ds.read_point_cloud(str(tmp_path / "scan.xyz"))
    with pytest.raises(NotImplementedError, match="dtype"):
        LiDARDataset(make_cfg(tmp_path, dtype=torch.float64))
    with pytest.raises(Exception, match="device"):
        LiDARDataset(make_cfg(tmp_path, device="cpu"))


def test_random_subset_is_exact_reproducible_and_keyed_by_frame():
    from shine_mapping_amd.dataset import random_subset

    n = 10007
    a = random_subset(n, int(n * 0.37), 42, 3, "cpu")
    assert a.numel() == int(n * 0.37) and torch.equal(a, torch.unique(a)) and int(a.min()) >= 0 and int(a.max()) < n
    assert torch.equal(a, random_subset(n, int(n * 0.37), 42, 3, "cpu"))
    assert not torch.equal(a, random_subset(n, int(n * 0.37), 42, 4, "cpu"))
    assert not torch.equal(a, random_subset(n, int(n * 0.37), 43, 3, "cpu"))
    assert torch.equal(random_subset(50, 50, 1, 0, "cpu"), torch.arange(50))
    # uniform: every tenth of the index range gets its share (binomial, 5 standard deviations)
    counts = torch.bincount((a * 10 // n).long(), minlength=10).double()
    p = 0.37
    assert float((counts - n / 10 * p).abs().max()) <= 5 * math.sqrt(n / 10 * p * (1 - p)) + 1


def test_written_kitti_drive_reads_back_as_the_poses_it_encodes(tmp_path):
    from shine_mapping_amd import synth
    from shine_mapping_amd.dataset import LiDARDataset

    cfg = synth.make_config("ncd", device="cuda")
    drive = synth.write_kitti_drive(str(tmp_path), cfg, frames=3, beams=8, azimuths=60, device="cpu")
    assert sorted(os.listdir(drive.pc_path)) == ["000000.bin", "000001.bin", "000002.bin"]
    scan = fo.read_kitti_bin(os.path.join(drive.pc_path, "000001.bin"))
    assert scan.shape[0] > 100 and scan.dtype == np.float32
    want = fo.kitti_poses(open(drive.pose_path).read(), open(drive.calib_path).read())
    for k in range(3):
        assert np.allclose(want[k], drive.lidar_poses[k], rtol=1e-12, atol=1e-12)
    # the sensor yaws from frame to frame and moves along the street
    assert abs(math.atan2(want[2][1, 0], want[2][0, 0]) - 0.1) < 1e-9 and want[2][0, 3] > want[0][0, 3]
    full = SimpleNamespace(**vars(make_cfg(tmp_path, n_files=0)))
    full.__dict__.update(pc_path=drive.pc_path, pose_path=drive.pose_path, calib_path=drive.calib_path, end_frame=2,
                         first_frame_ref=False)
    ds = LiDARDataset(full)
    for k in range(3):
        assert np.allclose(ds.poses_ref[k], want[k], rtol=1e-12, atol=1e-12)
    # a scan in the sensor frame, put back through its pose, lies in the street canyon: ground at z = 0, facades at |y| <= 8 m
    world = fo.transform(scan, want[1])
    assert world[:, 2].min() > -1e-3 and np.abs(world[:, 1]).max() < 8.0 + 1e-3


# ---- the C ABI's argument checks (no device is touched) ------------------------------------------------------------------------------
def test_frame_entry_points_reject_bad_arguments_without_a_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    INVALID = -1
    need = C.c_size_t(0)
    host = (C.c_char * 4096)()  # stands in for device memory: every call below returns before anything would touch it
    p = C.cast(host, C.c_void_p)
    kept = C.c_int64(-7)
    o3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    # shine_frame_filter
    assert lib.shine_frame_filter(None, 1000, 0, 4, -3.0, 30.0, 2.5, 25.0, None, C.byref(need), None, None, None) == 0
    assert need.value >= 8
    big = C.c_size_t(1 << 20)
    assert lib.shine_frame_filter(None, 1000, 0, 4, -3.0, 30.0, 2.5, 25.0, None, None, None, None, None) == INVALID
    assert lib.shine_frame_filter(p, -1, 0, 4, -3.0, 30.0, 2.5, 25.0, p, C.byref(big), p, C.byref(kept), None) == INVALID
    assert lib.shine_frame_filter(p, 1000, 0, 5, -3.0, 30.0, 2.5, 25.0, p, C.byref(big), p, C.byref(kept), None) == INVALID
    assert lib.shine_frame_filter(None, 1000, 0, 4, -3.0, 30.0, 2.5, 25.0, p, C.byref(big), p, C.byref(kept), None) == INVALID
    assert lib.shine_frame_filter(p, 1000, 0, 4, -3.0, 30.0, 2.5, 25.0, p, C.byref(big), None, C.byref(kept), None) == INVALID
    assert lib.shine_frame_filter(p, 1000, 0, 4, -3.0, 30.0, 2.5, 25.0, p, C.byref(big), p, None, None) == INVALID
    assert lib.shine_frame_filter(p, 1000, 0, 4, -3.0, 30.0, 2.5, -1.0, p, C.byref(big), p, C.byref(kept), None) == INVALID
    small = C.c_size_t(8)
    assert lib.shine_frame_filter(p, 1000, 0, 4, -3.0, 30.0, 2.5, 25.0, p, C.byref(small), p, C.byref(kept), None) == INVALID
    assert b"shine_frame_filter" in lib.shine_error_string(INVALID)
    assert lib.shine_frame_filter(None, 0, 0, 4, -3.0, 30.0, 2.5, 25.0, p, C.byref(big), None, C.byref(kept), None) == 0
    assert kept.value == 0

    # shine_ray_sample
    def sample(points=p, m=10, origin=o3, ns=3, nc=0, nf=3, scale=0.02, labels=None, coord=p, sdf=p, weight=p, sem=None):
        return lib.shine_ray_sample(points, m, origin, ns, nc, nf, 0.006, 0.005, 0.3, 0.02, scale, labels, 1, 0, None, 0.0,
                                    coord, sdf, weight, None, sem, None, None, None, None)

    assert sample(points=None) == INVALID and sample(origin=None) == INVALID and sample(coord=None) == INVALID
    assert sample(sdf=None) == INVALID and sample(weight=None) == INVALID
    assert sample(m=-1) == INVALID and sample(ns=-1) == INVALID and sample(nf=-2) == INVALID
    assert sample(ns=0, nc=0, nf=0) == INVALID and b"zero" in lib.shine_error_string(INVALID)
    assert sample(scale=0.0) == INVALID and sample(sem=p, labels=None) == INVALID
    assert sample(m=1 << 40) == INVALID
    assert sample(m=0, points=None, coord=None, sdf=None, weight=None) == 0  # the zero-ray call: nothing to launch

    # shine_pool_window_filter
    src, dst = _lib.ptr_array([C.addressof(host)]), _lib.ptr_array([C.addressof(host) + 2048])
    words = (C.c_int32 * 1)(3)

    def window(coord=p, n=100, origin=o3, radius=0.5, k=1, src=src, dst=dst, words=words, ws=p, size=big, out=kept):
        return lib.shine_pool_window_filter(coord, n, origin, radius, k, src, dst, words, ws,
                                            C.byref(size) if size is not None else None,
                                            C.byref(out) if out is not None else None, None)

    assert lib.shine_pool_window_filter(None, 100, o3, 0.5, 1, None, None, None, None, C.byref(need), None, None) == 0
    assert need.value >= 100
    assert window(coord=None) == INVALID and window(origin=None) == INVALID and window(out=None) == INVALID
    assert window(size=None) == INVALID and window(n=-5) == INVALID
    assert window(radius=0.0) == INVALID and window(radius=-1.0) == INVALID and b"radius" in lib.shine_error_string(INVALID)
    assert window(k=0) == INVALID and window(k=7) == INVALID and window(src=None) == INVALID and window(words=None) == INVALID
    assert window(words=(C.c_int32 * 1)(2)) == INVALID
    assert window(dst=src) == INVALID  # not in place
    assert window(size=small) == INVALID
    assert window(n=0, coord=None) == 0 and kept.value == 0
