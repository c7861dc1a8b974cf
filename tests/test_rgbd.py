"""CPU suite of shine_mapping_amd/rgbd.py: the readers (intrinsics, poses, depth frames), the synthetic RGB-D drive of synth.py
against the room's analytic surfaces, the argument checks of shine_depth_unproject (csrc/shine_frame.hip) and the host logic of
RGBDDataset's constructor.  Nothing here needs a GPU; the device stages are in tests/test_gpu_rgbd.py."""
import ctypes as C
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rgbd_oracle as ro


def _pose(k):
    c, s = math.cos(0.1 * k), math.sin(0.1 * k)
    return np.array([[c, -s, 0.0, 1.5 * k], [s, c, 0.0, -0.25 * k], [0.0, 0.0, 1.0, 0.125 * k], [0.0, 0.0, 0.0, 1.0]])


def _write_poses(path, n, kitti):
    with open(path, "w") as fh:
        for k in range(n):
            P = _pose(k)
            if kitti:
                fh.write(" ".join(repr(float(v)) for v in P[:3].reshape(-1)) + "\n")
            else:
                fh.write("\n".join(" ".join(repr(float(v)) for v in row) for row in P) + "\n")


def make_cfg(tmp_path, n_files=5, size=(8, 6), **over):
    depth = tmp_path / "depth"
    depth.mkdir(exist_ok=True)
    for k in range(n_files):
        np.save(str(depth / ("%d.npy" % k)), np.full((size[1], size[0]), 1000 + k, np.uint16))
    poses = tmp_path / "poses.txt"
    if not poses.exists():
        _write_poses(str(poses), n_files, kitti=False)
    focal = tmp_path / "focal.txt"
    focal.write_text("10.5\n")
    cfg = SimpleNamespace(
        device="cuda", dtype=torch.float32, depth_path=str(depth), intrinsic_path=str(focal), is_focal_file=True,
        pose_path=str(poses), pose_kitti_format=False, max_depth_m=5.0, first_frame_ref=True, begin_frame=0,
        end_frame=n_files - 1, every_frame=1, pc_count_gpu_limit=500, global_shift_default=0.0, seed=42, min_range=0.2,
        pc_radius=5.0, min_z=-10.0, max_z=30.0, rand_downsample=False, vox_down_m=0.01, rand_down_r=1.0, map_vox_down_m=0.05,
        estimate_normal=False, filter_noise=False, semantic_on=False, behind_dropoff_on=False, octree_from_surface_samples=True,
        surface_sample_range_m=0.05, surface_sample_n=3, free_sample_begin_ratio=0.5, free_sample_end_dist_m=0.3, free_sample_n=3,
        clearance_dist_m=0.3, clearance_sample_n=0, continual_learning_reg=False, window_replay_on=False, window_radius=50.0,
        ray_loss=False, bs=256, scale=1.0 / 40.96)
    cfg.__dict__.update(over)
    return cfg


# ---- the oracle's own checks ------------------------------------------------------------------------------------------------------
def test_oracle_on_a_hand_made_image():
    # 5 x 3 image, principal point at pixel (2, 1), fx = fy = 2, scale 1000, trunc 5
    img = np.zeros((3, 5), np.uint16)
    img[1, 2] = 1500   # principal point: p = (0, 0, 1.5) exactly
    img[0, 0] = 2000   # x = (0 - 2) * 2 / 2 = -2, y = (0 - 1) * 2 / 2 = -1
    img[2, 4] = 5000   # d == depth_trunc: dropped
    img[2, 3] = 4999   # one raw step below: kept
    pts, idx = ro.unproject(img, 2.0, 2.0, 2.0, 1.0, 1000.0, 5.0)
    assert idx.tolist() == [0, 7, 13] and idx.dtype == np.int32
    assert np.array_equal(pts[0], [-2.0, -1.0, 2.0]) and np.array_equal(pts[1], [0.0, 0.0, 1.5])
    z = np.float64(np.float32(4999) / np.float32(1000))
    assert np.array_equal(pts[2], [(3 - 2.0) * z / 2.0, (2 - 1.0) * z / 2.0, z])
    flipped, _ = ro.unproject(img, 2.0, 2.0, 2.0, 1.0, 1000.0, 5.0, np.diag([1.0, -1.0, -1.0, 1.0]))
    assert np.array_equal(flipped, pts * [1.0, -1.0, -1.0])
    # the filter: inclusive faces, inclusive min_range, strict min_z
    kept, idx = ro.unproject(img, 2.0, 2.0, 2.0, 1.0, 1000.0, 5.0, None, (-10.0, 2.0, 1.5, 2.0))
    assert idx.tolist() == [0, 7]  # (-2, -1, 2) on the -x face and at max_z; (0, 0, 1.5) at exactly min_range; the third beyond max_z
    assert ro.unproject(img, 2.0, 2.0, 2.0, 1.0, 1000.0, 5.0, None, (1.5, 30.0, 0.0, 5.0))[1].tolist() == [0, 13]  # z == min_z drops
    f = np.array([[np.nan, np.inf, -1.0, 0.0, 1.0]], np.float32)
    assert ro.unproject(f, 1.0, 1.0, 0.0, 0.0, 1.0, np.inf)[1].tolist() == [4]


# ---- readers ------------------------------------------------------------------------------------------------------------------------
def test_the_three_intrinsics_cases_and_their_defaults(tmp_path):
    from shine_mapping_amd.rgbd import FLIP, read_intrinsics

    k = read_intrinsics("")
    assert (k.width, k.height, k.fx, k.fy, k.cx, k.cy, k.depth_scale) == (640, 480, 525.0, 525.0, 319.5, 239.5, 1000.0)
    assert np.array_equal(k.extrinsic, np.diag([1.0, -1.0, -1.0, 1.0])) and np.array_equal(k.cam_to_sensor, FLIP)
    focal = tmp_path / "focal.txt"
    focal.write_text("554.2562584220408\nanything else\n")
    k = read_intrinsics(str(focal), True, (641, 480))
    assert (k.width, k.height, k.fx, k.fy, k.cx, k.cy, k.depth_scale) == (641, 480, 554.2562584220408, 554.2562584220408, 320.0,
                                                                          239.5, 1000.0)
    assert np.array_equal(k.cam_to_sensor, FLIP)
    with pytest.raises(ValueError, match="focal.txt.*image_size"):
        read_intrinsics(str(focal), True)
    cam = tmp_path / "cam.json"
    cam.write_text(json.dumps({"camera": {"w": 1200, "h": 680, "fx": 600.0, "fy": 601.0, "cx": 599.5, "cy": 339.5, "scale": 6553.5}}))
    k = read_intrinsics(str(cam), False)
    assert (k.width, k.height, k.fx, k.fy, k.cx, k.cy, k.depth_scale) == (1200, 680, 600.0, 601.0, 599.5, 339.5, 6553.5)
    assert np.array_equal(k.cam_to_sensor, np.eye(4))  # Replica: no flip
    # each mix-up names the file and the cause
    with pytest.raises(ValueError, match=r"cam\.json.*focal length"):
        read_intrinsics(str(cam), True, (1200, 680))
    with pytest.raises(ValueError, match=r"focal\.txt.*JSON"):
        read_intrinsics(str(focal), False)
    cam.write_text(json.dumps({"camera": {"w": 1200, "h": 680, "fx": 600.0}}))
    with pytest.raises(ValueError, match=r"cam\.json.*lacks fy, cx, cy, scale"):
        read_intrinsics(str(cam), False)


def test_four_line_and_kitti_pose_files_give_the_same_matrices(tmp_path):
    from shine_mapping_amd.rgbd import read_poses, write_poses_kitti

    _write_poses(str(tmp_path / "four.txt"), 4, kitti=False)
    _write_poses(str(tmp_path / "kitti.txt"), 4, kitti=True)
    a, b = read_poses(str(tmp_path / "four.txt")), read_poses(str(tmp_path / "kitti.txt"), kitti_format=True)
    assert len(a) == len(b) == 4
    for k in range(4):
        assert np.array_equal(a[k], _pose(k)) and np.array_equal(b[k], _pose(k))  # (repr floats: bit for bit)
    write_poses_kitti(str(tmp_path / "again.txt"), a)
    assert open(str(tmp_path / "again.txt")).read() == open(str(tmp_path / "kitti.txt")).read()
    with pytest.raises(ValueError, match=r"four\.txt.*12"):
        read_poses(str(tmp_path / "four.txt"), kitti_format=True)
    with pytest.raises(ValueError, match=r"kitti\.txt.*four lines"):
        read_poses(str(tmp_path / "kitti.txt"))
    (tmp_path / "odom.csv").write_text("ts,tx,ty,tz,qx,qy,qz,qw\n0.0,1.0,2.0,3.0,1.0,0.0,0.0,0.0\n")
    assert np.array_equal(read_poses(str(tmp_path / "odom.csv"))[0], [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])


def test_depth_frames_read_back_equal_and_bad_ones_are_named(tmp_path, monkeypatch):
    from shine_mapping_amd.rgbd import read_depth

    rng = np.random.default_rng(3)
    raw = rng.integers(0, 65536, size=(7, 9)).astype(np.uint16)
    np.save(str(tmp_path / "a.npy"), raw)
    got = read_depth(str(tmp_path / "a.npy"))
    assert got.dtype == np.uint16 and np.array_equal(got, raw)
    metres = rng.uniform(0, 6, size=(7, 9)).astype(np.float32)
    np.save(str(tmp_path / "b.npy"), metres)
    got = read_depth(str(tmp_path / "b.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, metres)
    np.save(str(tmp_path / "c.npy"), metres.astype(np.float64))
    with pytest.raises(ValueError, match=r"c\.npy.*float64"):
        read_depth(str(tmp_path / "c.npy"))
    np.save(str(tmp_path / "d.npy"), np.zeros((2, 3, 4), np.uint16))
    with pytest.raises(ValueError, match=r"d\.npy"):
        read_depth(str(tmp_path / "d.npy"))
    (tmp_path / "e.exr").write_bytes(b"")
    with pytest.raises(ValueError, match=r"e\.exr.*unknown depth frame format"):
        read_depth(str(tmp_path / "e.exr"))
    # a .png without PIL: the error names the file and the missing module
    (tmp_path / "f.png").write_bytes(b"")
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match=r"f\.png.*PIL"):
        read_depth(str(tmp_path / "f.png"))


def test_sixteen_bit_png_frames_read_back_equal(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from shine_mapping_amd import synth
    from shine_mapping_amd.rgbd import read_depth

    raw = np.random.default_rng(4).integers(0, 65536, size=(11, 13)).astype(np.uint16)
    Image.fromarray(raw).save(str(tmp_path / "a.png"))
    got = read_depth(str(tmp_path / "a.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, raw)
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(str(tmp_path / "rgb.png"))
    with pytest.raises(ValueError, match=r"rgb\.png.*single-channel"):
        read_depth(str(tmp_path / "rgb.png"))
    # the synthetic drive writes the same frames in both formats
    a = synth.write_rgbd_drive(str(tmp_path / "npy"), frames=2, width=32, height=24, focal=26.0, fmt="npy")
    b = synth.write_rgbd_drive(str(tmp_path / "png"), frames=2, width=32, height=24, focal=26.0, fmt="png")
    for f in range(2):
        assert np.array_equal(read_depth(os.path.join(a.depth_path, "%06d.npy" % f)), read_depth(os.path.join(b.depth_path, "%06d.png" % f)))


# ---- the synthetic drive ----------------------------------------------------------------------------------------------------------
def test_written_rgbd_drive_lies_on_the_rooms_surfaces(tmp_path):
    """Every valid pixel, back-projected by the oracle and put through its pose, lies on the analytic surface its ray was cast
    against, within (0.5 / depth_scale + 2^-24 * max_depth_m) * |dir| + 1e-9 m: half a depth step from the rounding to
    millimetres and the fp32 rounding of d, both along the ray of direction ((u - cx) / fx, (v - cy) / fy, 1), plus fp64 slack."""
    from shine_mapping_amd import synth
    from shine_mapping_amd.rgbd import read_depth, read_intrinsics, read_poses

    drive = synth.write_rgbd_drive(str(tmp_path), frames=4)
    W, H = drive.width, drive.height
    k = read_intrinsics(drive.intrinsic_path, True, (W, H))
    assert (k.fx, k.cx, k.cy) == (drive.focal, (W - 1) / 2.0, (H - 1) / 2.0)
    poses = read_poses(drive.pose_path)
    assert sorted(os.listdir(drive.depth_path)) == ["%06d.npy" % f for f in range(4)]
    all_kinds = 0
    for f in range(4):
        assert np.array_equal(poses[f], drive.poses[f])
        R = poses[f][:3, :3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
        raw = read_depth(os.path.join(drive.depth_path, "%06d.npy" % f))
        assert raw.shape == (H, W) and raw.dtype == np.uint16
        pts, idx = ro.unproject(raw, k.fx, k.fy, k.cx, k.cy, k.depth_scale, drive.max_depth_m, k.cam_to_sensor)
        world = ro.transform(pts, poses[f])
        kind, exact = drive.kinds[f].reshape(-1), drive.exact_depths[f].reshape(-1)
        u, v = idx % W, idx // W
        length = np.sqrt(((u - k.cx) / k.fx) ** 2 + ((v - k.cy) / k.fy) ** 2 + 1.0)
        bound = (0.5 / k.depth_scale + 2.0 ** -24 * drive.max_depth_m) * length + 1e-9
        dist = ro.surface_distance(world, kind[idx], drive.room, drive.boxes)
        worst = int(np.argmax(dist / bound))
        print("frame %d: %d valid pixels, worst distance / bound = %.3e / %.3e m" % (f, len(idx), dist[worst], bound[worst]))
        assert np.all(kind[idx] != synth.MISS) and np.all(dist <= bound)
        # and the depths are the exact ones rounded to millimetres, 0 for a miss or a hit beyond the written range
        assert np.all(np.abs(raw.reshape(-1)[idx] / k.depth_scale - exact[idx]) <= 0.5 / k.depth_scale + 1e-12)
        flat = raw.reshape(-1)
        seen = {"ground": np.any(kind[idx] == synth.GROUND), "facade": np.any(kind[idx] == synth.FACADE),
                "box": np.any(kind[idx] == synth.BOX), "beyond max_depth_m": np.any(flat >= drive.max_depth_m * k.depth_scale),
                "missing": np.any((flat == 0) & (kind == synth.MISS)), "beyond the written range": np.any((flat == 0) & (kind != synth.MISS))}
        print("frame %d:" % f, {n: bool(s) for n, s in seen.items()})
        all_kinds += all(seen.values())
        assert np.all(flat[kind == synth.MISS] == 0)
    assert all_kinds >= 1  # at least one frame shows every kind of pixel


# ---- the C ABI's argument checks (no device is touched) ------------------------------------------------------------------------------
def test_depth_unproject_rejects_bad_arguments_without_a_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    INVALID = -1
    host = (C.c_char * 4096)()  # stands in for device memory: every call below returns before anything would touch it
    p = C.cast(host, C.c_void_p)
    big, small, need, kept = C.c_size_t(1 << 20), C.c_size_t(8), C.c_size_t(0), C.c_int64(-7)
    inf = float("inf")

    def call(depth=p, f32=0, w=64, h=48, pitch=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5, scale=1000.0, trunc=5.0, M=None,
             box=(-inf, inf, 0.0, inf), ws=p, size=big, out=p, index=None, n_out=kept):
        return lib.shine_depth_unproject(depth, f32, w, h, pitch, fx, fy, cx, cy, scale, trunc, M, *box, ws,
                                         C.byref(size) if size is not None else None, out, index,
                                         C.byref(n_out) if n_out is not None else None, None)

    assert call(depth=None, ws=None, size=need, out=None, n_out=None) == 0 and need.value >= 8 + 8 * 3  # 64 x 48 = 3 tiles
    first = need.value
    assert call(depth=None, w=640, h=480, pitch=640, ws=None, size=need, out=None, n_out=None) == 0 and need.value > first
    assert call(size=None) == INVALID
    assert call(w=-1) == INVALID and call(h=-1) == INVALID and call(w=1 << 16, h=1 << 15, pitch=1 << 16) == INVALID
    assert call(pitch=63) == INVALID and b"row_pitch" in lib.shine_error_string(INVALID)
    assert call(size=small) == INVALID and b"workspace too small" in lib.shine_error_string(INVALID)
    assert call(n_out=None) == INVALID
    assert call(fx=0.0) == INVALID and call(fy=0.0) == INVALID and call(fx=float("nan")) == INVALID
    assert b"fx" in lib.shine_error_string(INVALID)
    assert call(scale=0.0) == INVALID and call(scale=-1000.0) == INVALID and b"depth_scale" in lib.shine_error_string(INVALID)
    assert call(trunc=float("nan")) == INVALID
    assert call(box=(-3.0, 30.0, 0.2, -1.0)) == INVALID and call(box=(3.0, -3.0, 0.2, 5.0)) == INVALID
    assert call(box=(-3.0, 30.0, float("nan"), 5.0)) == INVALID
    assert call(depth=None) == INVALID and call(out=None) == INVALID and b"shine_depth_unproject" in lib.shine_error_string(INVALID)
    # the zero-pixel call: nothing to launch, whatever the pointers
    assert call(depth=None, w=0, h=48, pitch=0, out=None) == 0 and kept.value == 0
    kept.value = -7
    assert call(depth=None, w=64, h=0, out=None) == 0 and kept.value == 0


# ---- RGBDDataset's constructor ------------------------------------------------------------------------------------------------------
def test_rgbd_dataset_constructor_host_logic(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset
    from shine_mapping_amd.rgbd import RGBDDataset

    cfg = make_cfg(tmp_path, n_files=12, begin_frame=2, end_frame=9, every_frame=3)
    ds = RGBDDataset(cfg)
    assert isinstance(ds, LiDARDataset)
    assert ds.pc_filenames == ["%d.npy" % k for k in range(12)]  # 1, 2, ... 9, 10, 11 — not 1, 10, 11, 2
    assert ds.total_pc_count == 12 and ds.used_pc_count == 3 and len(ds) == 0  # frames 3, 6, 9
    inv3 = np.linalg.inv(_pose(3))
    assert np.allclose(ds.begin_pose_inv, inv3, rtol=1e-13, atol=1e-15)
    for k in range(12):
        want = inv3 @ _pose(k) if k in (3, 6, 9) else _pose(k)
        assert np.allclose(ds.poses_ref[k], want, rtol=1e-12, atol=1e-14)
    k = ds.intrinsics  # the focal file + the first frame's size
    assert (k.width, k.height, k.fx, k.fy, k.cx, k.cy, k.depth_scale) == (8, 6, 10.5, 10.5, 3.5, 2.5, 1000.0)
    assert ds.max_depth_m == 5.0 and ds.pool_device == "cuda" and ds.coord_pool.shape == (0, 3)
    assert np.array_equal(ds.read_depth_frame(4), np.full((6, 8), 1004, np.uint16))
    # first_frame_ref off: the world frame shifted by global_shift_default; KITTI-format poses; the PrimeSense default
    _write_poses(str(tmp_path / "kitti.txt"), 12, kitti=True)
    ds2 = RGBDDataset(make_cfg(tmp_path, n_files=12, first_frame_ref=False, global_shift_default=0.25, intrinsic_path="",
                               pose_path=str(tmp_path / "kitti.txt"), pose_kitti_format=True))
    shift = np.eye(4)
    shift[2, 3] = 0.25
    for f in range(12):
        assert np.allclose(ds2.poses_ref[f], shift @ _pose(f), rtol=1e-13, atol=1e-15)
    assert (ds2.intrinsics.width, ds2.intrinsics.height, ds2.intrinsics.fx) == (640, 480, 525.0)
    with pytest.raises(ValueError, match=r"4\.npy.*8 x 6.*PrimeSense default.*640 x 480"):
        ds2.read_depth_frame(4)
    few = dict(begin_frame=0, end_frame=11, every_frame=1, pc_count_gpu_limit=5)
    assert RGBDDataset(make_cfg(tmp_path, n_files=12, **few)).pool_device == "cpu"
    assert RGBDDataset(make_cfg(tmp_path, n_files=12, window_replay_on=True, **few)).pool_device == "cuda"
    # the refusals LiDARDataset makes hold here too
    with pytest.raises(Exception, match="device"):
        RGBDDataset(make_cfg(tmp_path, device="cpu"))
    with pytest.raises(NotImplementedError, match="semantic_on"):
        RGBDDataset(make_cfg(tmp_path, semantic_on=True))
    # a frame of another size than the intrinsics', an unknown extension: named when the frame is read
    np.save(os.path.join(cfg.depth_path, "3.npy"), np.zeros((6, 9), np.uint16))
    with pytest.raises(ValueError, match=r"3\.npy.*9 x 6.*8 x 6"):
        ds.read_depth_frame(3)
    os.rename(os.path.join(cfg.depth_path, "11.npy"), os.path.join(cfg.depth_path, "11.tiff"))
    ds3 = RGBDDataset(make_cfg(tmp_path, n_files=11))
    with pytest.raises(ValueError, match=r"11\.tiff.*unknown depth frame format"):
        ds3.read_depth_frame(11)


def test_unproject_depth_has_no_cpu_path():
    from shine_mapping_amd import _lib
    from shine_mapping_amd.rgbd import Intrinsics, unproject_depth

    k = Intrinsics(8, 6, 10.0, 10.0, 3.5, 2.5)
    with pytest.raises(_lib.ShineHipError, match="device only"):
        unproject_depth(torch.zeros((6, 8), dtype=torch.float32), k)
    with pytest.raises(ValueError, match="uint16"):
        unproject_depth(np.zeros((6, 8), np.float64), k)
