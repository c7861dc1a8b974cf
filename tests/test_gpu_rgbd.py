"""GPU suite of the RGB-D front-end (shine_mapping_amd/rgbd.py, shine_depth_unproject in csrc/shine_frame.hip):
  * the kernel against the numpy oracle (tests/rgbd_oracle.py), EXACT: points, pixel indices and count — every operation of the
    rules is one correctly rounded IEEE operation in a fixed order, so there is nothing to tolerate;
  * determinism across repeated calls and across a workspace reused by a larger image;
  * route equality: RGBDDataset (direct) against the converter followed by the existing LiDARDataset, torch.equal pools;
  * RGBDDataset end to end on a synthetic drive: octree growth, the fused loop, meshing, eval_mesh;
  * the converter's command line in a child process.
Every test here fails without shine_mapping_amd.rgbd / shine_depth_unproject."""
import ctypes as C
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rgbd_oracle as ro
from conftest import ROOT

pytestmark = pytest.mark.gpu

TILE = 1024  # pixels per workgroup of k_depth_unproject (4 per lane, 256 lanes)
FLIP = np.diag([1.0, -1.0, -1.0, 1.0])
BOX = (-1.0, 2.5, 0.4, 1.5)  # min_z, max_z, min_range, pc_radius: every bound cuts through the random images below


def _rigid():
    a, b = 0.3, -0.2
    Rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Rx
    M[:3, 3] = [0.11, -0.07, 0.23]
    return M


def _intrinsics(w, h, scale=1000.0):
    from shine_mapping_amd.rgbd import Intrinsics

    f = 0.8 * max(w, h, 2)
    return Intrinsics(w, h, f, 1.01 * f, (w - 1) / 2.0, (h - 1) / 2.0, scale)


def _image(w, h, dtype, seed):
    """a random depth image: a fifth of the pixels hold no depth, the rest 0.2 - 7 m (so that depth_trunc = 5 m drops some); the
    float32 kind (metres, depth_scale 1) also holds NaN, +-inf, negative and denormal depths"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.2, 7.0, size=(h, w))
    d[rng.random((h, w)) < 0.2] = 0.0
    if dtype == np.uint16:
        return np.rint(d * 1000.0).astype(np.uint16)
    d = d.astype(np.float32)
    bad = rng.random((h, w))
    d[bad < 0.01] = np.nan
    d[(bad >= 0.01) & (bad < 0.02)] = np.inf
    d[(bad >= 0.02) & (bad < 0.03)] = -np.inf
    d[(bad >= 0.03) & (bad < 0.04)] = -1.5
    d[(bad >= 0.04) & (bad < 0.05)] = 1e-42
    return d


def _want(img, k, trunc, M, box):
    return ro.unproject(img, k.fx, k.fy, k.cx, k.cy, k.depth_scale, trunc, M, box)


def _check(img_dev, img_host, k, trunc, M, box, what):
    from shine_mapping_amd.rgbd import unproject_depth

    pts, idx = unproject_depth(img_dev, k, cam_to_sensor=M, max_depth_m=trunc, filter=box, return_index=True)
    want_p, want_i = _want(img_host, k, trunc, M, box)
    print("%s: %d of %d pixels kept (oracle %d)" % (what, pts.shape[0], img_host.size, len(want_i)))
    assert pts.dtype == torch.float64 and idx.dtype == torch.int32 and pts.shape == (idx.shape[0], 3)
    assert pts.shape[0] == len(want_i)
    assert torch.equal(idx.cpu(), torch.from_numpy(want_i))
    assert torch.equal(pts.cpu(), torch.from_numpy(want_p)), what
    only = unproject_depth(img_dev, k, cam_to_sensor=M, max_depth_m=trunc, filter=box)  # index_out == NULL
    assert torch.equal(only, pts)
    return pts, idx


SIZES = [(1, 1), (2, 3), (3, 1), (32, 32), (31, 33), (41, 25), (37, 29), (1, 2050), (2049, 1), (640, 480), (643, 481), (1920, 1080)]


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_equals_the_oracle_exactly(w, h, dtype):
    """sizes from 1 x 1 over one tile (32 x 32 = 1024 pixels), one tile - 1 (31 x 33) and + 1 (41 x 25) to 1920 x 1080; widths that
    are no multiple of the 4-pixel vector; identity, flip and a general rigid cam_to_sensor; filter on and off"""
    assert 32 * 32 == TILE and 31 * 33 == TILE - 1 and 41 * 25 == TILE + 1
    scale = 1000.0 if dtype == np.uint16 else 1.0
    k = _intrinsics(w, h, scale)
    img = _image(w, h, dtype, 7 * w + h)
    dev = torch.from_numpy(img.view(np.int16) if dtype == np.uint16 else img).cuda()
    cases = [(None, None), (np.eye(4), BOX), (FLIP, None), (FLIP, BOX), (_rigid(), BOX), (_rigid(), None)]
    if w * h > 1 << 20:
        cases = [(FLIP, BOX), (_rigid(), None)]
    for M, box in cases:
        what = "%d x %d %s, %s, filter %s" % (w, h, np.dtype(dtype).name,
                                              "default" if M is None else "identity" if np.array_equal(M, np.eye(4)) else
                                              "flip" if np.array_equal(M, FLIP) else "rigid", "on" if box else "off")
        pts, idx = _check(dev, img, k, 5.0, M, box, what)  # (M = None: the intrinsics' own, here the identity)
        if w * h >= 1024:
            assert 0 < pts.shape[0] < w * h
    # the host-array entry (one upload) gives the same
    from shine_mapping_amd.rgbd import unproject_depth

    a = unproject_depth(img, k, cam_to_sensor=FLIP, filter=BOX)
    assert torch.equal(a.cpu(), torch.from_numpy(_want(img, k, 5.0, FLIP, BOX)[0]))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("w,h,pitch,offset", [(37, 29, 40, 0), (37, 29, 41, 1), (64, 48, 64 + 4, 1), (64, 48, 67, 3), (640, 480, 641, 1),
                                              (5, 7, 9, 2), (1, 33, 3, 1)])
def test_row_pitch_and_unaligned_base(w, h, pitch, offset, dtype):
    """the image is a view into a wider buffer: row_pitch > width, the base address `offset` pixels past an aligned one; what lies
    outside the view is poisoned with valid depths, so a read of the wrong pixel changes the result"""
    scale = 1000.0 if dtype == np.uint16 else 1.0
    k = _intrinsics(w, h, scale)
    img = _image(w, h, dtype, 1000 + w + pitch)
    buf = np.full((h, pitch), 1234 if dtype == np.uint16 else 1.234, dtype)
    buf[:, offset:offset + w] = img
    dev = torch.from_numpy(buf.view(np.int16) if dtype == np.uint16 else buf).cuda()
    view = dev[:, offset:offset + w]
    assert view.stride(0) == pitch and view.data_ptr() == dev.data_ptr() + offset * dev.element_size()
    for M, box in ((FLIP, None), (_rigid(), BOX)):
        _check(view, img, k, 5.0, M, box, "%d x %d in pitch %d at +%d %s" % (w, h, pitch, offset, np.dtype(dtype).name))


def test_all_zero_and_all_valid_images():
    from shine_mapping_amd.rgbd import unproject_depth

    k = _intrinsics(643, 481)
    zero = np.zeros((481, 643), np.uint16)
    pts, idx = unproject_depth(zero, k, return_index=True)
    assert pts.shape == (0, 3) and idx.shape == (0,)
    full = np.full((481, 643), 2500, np.uint16)
    pts, idx = _check(torch.from_numpy(full.view(np.int16)).cuda(), full, k, 5.0, FLIP, None, "all valid")
    assert pts.shape[0] == 643 * 481 and torch.equal(idx.cpu(), torch.arange(643 * 481, dtype=torch.int32))
    f = np.full((48, 64), 1.0, np.float32)
    pts = unproject_depth(f, _intrinsics(64, 48, 1.0), max_depth_m=float("inf"))
    assert pts.shape[0] == 64 * 48
    empty = unproject_depth(torch.empty((0, 0), dtype=torch.float32, device="cuda"), _intrinsics(0, 0, 1.0))
    assert empty.shape == (0, 3)


def test_pixels_on_the_boundaries():
    """cases built with the oracle so that they sit exactly on the bounds: identity cam_to_sensor, integer principal point (a pixel
    there gives p = (0, 0, z) exactly), fx = fy = 2"""
    from shine_mapping_amd.rgbd import Intrinsics, unproject_depth

    w, h = 13, 9
    k = Intrinsics(w, h, 2.0, 2.0, 6.0, 4.0, 1000.0, np.eye(4))
    pp = 4 * w + 6  # the principal point's pixel index

    def run(img, trunc, box):
        dev = torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda()
        pts, idx = unproject_depth(dev, k, max_depth_m=trunc, filter=box, return_index=True)
        want_p, want_i = _want(img, k, trunc, None, box)
        assert torch.equal(idx.cpu(), torch.from_numpy(want_i)) and torch.equal(pts.cpu(), torch.from_numpy(want_p))
        return want_p, want_i.tolist()

    # depth_trunc: d == trunc is dropped, one raw step below is kept
    img = np.zeros((h, w), np.uint16)
    img[0, 0], img[0, 1], img[0, 2] = 5000, 4999, 5001
    assert np.float32(5000) / np.float32(1000) == np.float32(5.0)
    _, idx = run(img, 5.0, None)
    assert idx == [1]
    kf = Intrinsics(w, h, 2.0, 2.0, 6.0, 4.0, 1.0, np.eye(4))
    imf = np.zeros((h, w), np.float32)
    imf[0, 0], imf[0, 1] = 5.0, np.nextafter(np.float32(5.0), np.float32(0.0))
    got = unproject_depth(imf, kf, max_depth_m=5.0, return_index=True)[1]
    assert got.tolist() == [1] == ro.unproject(imf, 2.0, 2.0, 6.0, 4.0, 1.0, 5.0)[1].tolist()
    # the crop faces: x = (u - 6) * z / 2 with z = 1 -> u = 10 gives x = 2 exactly, u = 11 gives 2.5; y likewise
    img = np.zeros((h, w), np.uint16)
    img[4, 10], img[4, 11], img[4, 2], img[4, 1] = 1000, 1000, 1000, 1000
    img[8, 6], img[0, 6] = 1000, 1000  # y = (8 - 4) / 2 = 2 and -2
    pts, idx = run(img, 5.0, (-10.0, 30.0, 0.0, 2.0))
    assert idx == [0 * w + 6, 4 * w + 2, 4 * w + 10, 8 * w + 6]
    assert pts[:, 0].tolist() == [0.0, -2.0, 2.0, 0.0] and pts[:, 1].tolist() == [-2.0, 0.0, 0.0, 2.0]  # on the faces: kept
    # min_range and max_z at the principal point: p = (0, 0, z)
    img = np.zeros((h, w), np.uint16)
    img[4, 6] = 500
    assert np.float64(np.float32(500) / np.float32(1000)) == 0.5
    assert run(img, 5.0, (-10.0, 30.0, 0.5, 5.0))[1] == [pp]  # |p| == min_range: kept
    assert run(img, 5.0, (-10.0, 30.0, np.nextafter(0.5, 1.0), 5.0))[1] == []
    assert run(img, 5.0, (-10.0, 0.5, 0.0, 5.0))[1] == [pp]  # z == max_z: kept
    assert run(img, 5.0, (-10.0, np.nextafter(0.5, 0.0), 0.0, 5.0))[1] == []
    assert run(img, 5.0, (0.5, 30.0, 0.0, 5.0))[1] == []  # z == min_z: dropped (strict)
    assert run(img, 5.0, (np.nextafter(0.5, 0.0), 30.0, 0.0, 5.0))[1] == [pp]
    # an off-axis point, p = (1.5, 2, 1): min_range set to its own no-FMA norm keeps it, one ulp more drops it
    img = np.zeros((h, w), np.uint16)
    img[8, 9] = 1000
    r = math.sqrt(1.5 * 1.5 + 2.0 * 2.0 + 1.0)
    assert run(img, 5.0, (-10.0, 30.0, r, 5.0))[1] == [8 * w + 9]
    assert run(img, 5.0, (-10.0, 30.0, np.nextafter(r, 10.0), 5.0))[1] == []


def _raw_call(lib, img, k, ws, M, box, trunc=5.0):
    """shine_depth_unproject through ctypes with a caller-owned workspace -> (points, indices)"""
    from shine_mapping_amd import _lib

    h, w = img.shape
    n = w * h
    pts = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    m16 = (C.c_double * 16)(*[float(v) for v in np.asarray(M).reshape(-1)])
    size, kept = C.c_size_t(ws.numel()), C.c_int64(0)
    _lib.check(lib.shine_depth_unproject(img.data_ptr(), int(img.dtype == torch.float32), w, h, w, k.fx, k.fy, k.cx, k.cy,
                                         k.depth_scale, trunc, m16, *box, ws.data_ptr(), C.byref(size), pts.data_ptr(),
                                         idx.data_ptr(), C.byref(kept), _lib.current_stream_handle()), "shine_depth_unproject")
    return pts[:kept.value].clone(), idx[:kept.value].clone()


def test_repeated_calls_and_a_reused_workspace_give_identical_outputs():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    small, large = _image(643, 481, np.uint16, 11), _image(1920, 1080, np.uint16, 12)
    ks, kl = _intrinsics(643, 481), _intrinsics(1920, 1080)
    ds = torch.from_numpy(small.view(np.int16)).cuda()
    dl = torch.from_numpy(large.view(np.int16)).cuda()
    need = C.c_size_t(0)
    _lib.check(lib.shine_depth_unproject(None, 0, 1920, 1080, 1920, kl.fx, kl.fy, kl.cx, kl.cy, 1000.0, 5.0, None, *BOX, None,
                                         C.byref(need), None, None, None, None), "shine_depth_unproject")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")  # sized for the larger image, shared by every call below
    M = _rigid()
    first = _raw_call(lib, ds, ks, ws, M, BOX)
    want_p, want_i = _want(small, ks, 5.0, M, BOX)
    assert torch.equal(first[0].cpu(), torch.from_numpy(want_p)) and torch.equal(first[1].cpu(), torch.from_numpy(want_i))
    for _ in range(5):
        again = _raw_call(lib, ds, ks, ws, M, BOX)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    big = _raw_call(lib, dl, kl, ws, M, BOX)
    want_p, want_i = _want(large, kl, 5.0, M, BOX)
    assert torch.equal(big[0].cpu(), torch.from_numpy(want_p)) and torch.equal(big[1].cpu(), torch.from_numpy(want_i))
    for _ in range(3):  # the workspace now holds the larger image's tile states
        again = _raw_call(lib, ds, ks, ws, M, BOX)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    assert torch.equal(_raw_call(lib, dl, kl, ws, M, BOX)[0], big[0])


# ---- the dataset ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    from shine_mapping_amd import synth

    return synth.write_rgbd_drive(str(tmp_path_factory.mktemp("rgbd")), frames=5)


@pytest.fixture(scope="module")
def converted(drive, tmp_path_factory):
    """the converter's output for the drive (in this process; the command line has its own test)"""
    from shine_mapping_amd.rgbd import rgbd_to_kitti_format

    out = str(tmp_path_factory.mktemp("kitti_format"))
    assert rgbd_to_kitti_format(drive.depth_path, drive.pose_path, out, drive.intrinsic_path, True, False, drive.max_depth_m) == drive.frames
    return out


def _pair(drive, converted, **over):
    """(cfg, RGBDDataset) on the drive and (cfg, LiDARDataset) on the converter's output, same seed, same filter values"""
    from shine_mapping_amd import FeatureOctree, synth
    from shine_mapping_amd.dataset import LiDARDataset
    from shine_mapping_amd.rgbd import RGBDDataset

    # (a crop radius, a minimum range and a z window inside the frames' extent, so that the filter really drops points)
    cfg_a = synth.rgbd_config("rgbd", drive, **dict(dict(pc_radius=2.0, min_range=0.8, min_z=-3.5, max_z=1.0), **over))
    cfg_b = SimpleNamespace(**vars(cfg_a))
    cfg_b.__dict__.update(pc_path=os.path.join(converted, "rgbd_ply"), pose_path=os.path.join(converted, "poses.txt"), calib_path="")
    torch.manual_seed(1)
    a = RGBDDataset(cfg_a, FeatureOctree(cfg_a))
    torch.manual_seed(1)
    b = LiDARDataset(cfg_b, FeatureOctree(cfg_b))
    return cfg_a, a, b


def _assert_same_state(a, b, pools):
    for n in pools:
        pa, pb = getattr(a, n + "_pool"), getattr(b, n + "_pool")
        assert pa.shape == pb.shape and pa.shape[0] > 0 and torch.equal(pa, pb), n
    assert np.array_equal(a.map_bbx.get_min_bound(), b.map_bbx.get_min_bound())
    assert np.array_equal(a.map_bbx.get_max_bound(), b.map_bbx.get_max_bound())
    assert len(a.map_down_pc) == len(b.map_down_pc) > 0 and torch.equal(a.map_down_pc.points, b.map_down_pc.points)
    assert len(a) == len(b)


POINT_POOLS = ("coord", "sdf_label", "weight", "origin", "time")


@pytest.mark.parametrize("mode", ["batch", "incremental", "window_replay", "ray_loss"])
def test_direct_route_equals_converter_plus_lidar_dataset(drive, converted, mode):
    over = {"window_replay": dict(window_replay_on=True, window_radius=1.5), "ray_loss": dict(ray_loss=True)}.get(mode, {})
    cfg, a, b = _pair(drive, converted, **over)
    for f in range(drive.frames):
        assert np.array_equal(a.poses_ref[f], b.poses_ref[f])
        a.process_frame(f, incremental_on=mode == "incremental")
        b.process_frame(f, incremental_on=mode == "incremental")
        assert torch.equal(a.cur_frame_pc.points, b.cur_frame_pc.points)
    print("%s: %d samples, %d map points, box %s .. %s" % (mode, a.coord_pool.shape[0], len(a.map_down_pc),
                                                          a.map_bbx.get_min_bound(), a.map_bbx.get_max_bound()))
    _assert_same_state(a, b, ("coord", "weight", "sample_depth", "ray_depth") if mode == "ray_loss" else POINT_POOLS)
    # the filter and the down-sampling really dropped points, and the direct route read fewer points than the files hold
    from shine_mapping_amd.evaluation import read_ply

    raw = read_ply(os.path.join(converted, "rgbd_ply", "%06d.ply" % 2))["vertices"]
    kept = a.frame_points(2)
    assert 0 < kept.shape[0] < len(raw) < drive.width * drive.height
    if mode == "window_replay":
        n_all = a.sampler.S * sum(int(a.frame_points(f).shape[0]) for f in range(drive.frames))
        assert len(a) < n_all
    if mode != "ray_loss":
        # the octrees grew alike
        assert [int(p.shape[0]) for p in a.octree.hier_features] == [int(p.shape[0]) for p in b.octree.hier_features]


def test_rgbd_dataset_end_to_end_trains_meshes_and_evaluates(drive, tmp_path):
    from shine_mapping_amd import Decoder, FeatureOctree, StepOptions, synth
    from shine_mapping_amd.evaluation import eval_mesh, read_ply
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.mesher import Mesher
    from shine_mapping_amd.optim import setup_optimizer
    from shine_mapping_amd.rgbd import RGBDDataset

    cfg = synth.rgbd_config("rgbd", drive)
    torch.manual_seed(1)
    octree = FeatureOctree(cfg)
    ds = RGBDDataset(cfg, octree)
    k = ds.intrinsics
    total, exact = 0, []
    for f in range(drive.frames):
        raw = np.load(os.path.join(drive.depth_path, "%06d.npy" % f))
        want, _ = ro.unproject(raw, k.fx, k.fy, k.cx, k.cy, k.depth_scale, cfg.max_depth_m, k.cam_to_sensor,
                               (cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius))
        m = int(ds.frame_points(f).shape[0])
        assert 0 < m <= len(want)
        ds.process_frame(f, incremental_on=False)
        total += ds.sampler.S * m
        assert len(ds) == total == ds.coord_pool.shape[0]
        # the cloud of the exact (unquantised) depths, in the world frame the map is built in (first_frame_ref off)
        t = drive.exact_depths[f]
        v, u = np.nonzero(t < cfg.max_depth_m)
        z = t[v, u]
        cam = np.stack(((u - k.cx) * z / k.fx, -((v - k.cy) * z / k.fy), -z), 1)
        exact.append(ro.transform(cam, ds.poses_ref[f]))
    exact = np.concatenate(exact)
    print("batch mode: %d samples from %d frames of %d x %d" % (total, drive.frames, drive.width, drive.height))
    assert len(octree.hier_features) == cfg.tree_level_feat and all(p.shape[0] > 100 for p in octree.hier_features)
    # the surface samples lie within the sampling range of the exact surface cloud's box
    lo, hi = exact.min(0) - 0.1, exact.max(0) + 0.1
    surf = ds.coord_pool[ds.weight_pool > 0].double().cpu().numpy() / cfg.scale
    assert np.all(surf >= lo) and np.all(surf <= hi)
    torch.manual_seed(2)
    dec = Decoder(cfg).cuda()
    opt = setup_optimizer(cfg, list(octree.parameters()), dec.fused_params())
    pool = ds.sorted_pool()
    assert pool is ds.sorted_pool() and pool.size == total
    it = GraphedIteration(octree, dec, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid, loss_reduction="mean"), cfg.bs)
    losses = [float(it()) for _ in range(300)]
    torch.cuda.synchronize()
    print("fused loop: loss %.5f -> %.5f" % (losses[0], losses[-1]))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    cfg.min_cluster_vertices = 10
    path = str(tmp_path / "mesh.ply")
    mesh = Mesher(cfg, octree, dec).recon_bbx_mesh(ds.map_bbx, 0.04, path, None, estimate_normal=False, filter_isolated_mesh=False)
    print("mesh: %d vertices, %d triangles" % (len(np.asarray(mesh.vertices)), len(np.asarray(mesh.triangles))))
    assert len(np.asarray(mesh.triangles)) > 0 and os.path.getsize(path) > 0
    ds.write_merged_pc(str(tmp_path / "merged.ply"))
    assert read_ply(str(tmp_path / "merged.ply"))["vertices"].shape == (len(ds.map_down_pc), 3)
    metrics = eval_mesh(path, torch.from_numpy(exact).cuda(), down_sample_res=0.02, threshold=0.05, truncation_acc=0.2,
                        truncation_com=0.2, mesh_sample_point=1000000)
    print("eval_mesh against the exact cloud (recorded in DESIGN.md §3.12, not asserted):", metrics)
    assert all(math.isfinite(float(v)) for v in metrics.values())


def test_converter_command_line_in_a_child_process(tmp_path):
    from shine_mapping_amd import synth
    from shine_mapping_amd.evaluation import read_ply
    from shine_mapping_amd.rgbd import read_depth, read_intrinsics, read_poses, unproject_depth

    drive = synth.write_rgbd_drive(str(tmp_path / "in"), frames=3, width=64, height=48, focal=52.0)
    out = str(tmp_path / "out")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "shine_mapping_amd.rgbd", "--depth_img_folder", drive.depth_path, "--pose_file",
                        drive.pose_path, "--intrinsic_file", drive.intrinsic_path, "--is_focal_file", "True", "--output_root", out,
                        "--max_depth_m", "4.0"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(os.path.join(out, "rgbd_ply"))) == ["%06d.ply" % f for f in range(3)]
    k = read_intrinsics(drive.intrinsic_path, True, (64, 48))
    for f in range(3):
        path = os.path.join(out, "rgbd_ply", "%06d.ply" % f)
        head = open(path, "rb").read(400).split(b"end_header")[0].decode().split("\n")
        want = unproject_depth(read_depth(os.path.join(drive.depth_path, "%06d.npy" % f)), k, max_depth_m=4.0).cpu().numpy()
        assert head[:6] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(want), "property double x",
                            "property double y", "property double z"]
        assert len(want) > 0 and np.array_equal(read_ply(path)["vertices"], want)
    got, src = read_poses(os.path.join(out, "poses.txt"), kitti_format=True), read_poses(drive.pose_path)
    assert len(got) == len(src) == 3 and all(np.array_equal(a, b) for a, b in zip(got, src))


def test_converter_gathers_colour_through_the_pixel_indices(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from shine_mapping_amd import synth
    from shine_mapping_amd.evaluation import read_ply
    from shine_mapping_amd.rgbd import read_depth, read_intrinsics, rgbd_to_kitti_format, unproject_depth

    drive = synth.write_rgbd_drive(str(tmp_path / "in"), frames=2, width=64, height=48, focal=52.0, fmt="png")
    os.makedirs(str(tmp_path / "rgb"))
    rng = np.random.default_rng(5)
    colours = [rng.integers(0, 256, size=(48, 64, 3)).astype(np.uint8) for _ in range(2)]
    for f in range(2):
        Image.fromarray(colours[f]).save(str(tmp_path / "rgb" / ("%d.png" % f)))
    out = str(tmp_path / "out")
    rgbd_to_kitti_format(drive.depth_path, drive.pose_path, out, drive.intrinsic_path, rgb_img_folder=str(tmp_path / "rgb"))
    k = read_intrinsics(drive.intrinsic_path, True, (64, 48))
    for f in range(2):
        d = read_ply(os.path.join(out, "rgbd_ply", "%06d.ply" % f))
        pts, idx = unproject_depth(read_depth(os.path.join(drive.depth_path, "%06d.png" % f)), k, return_index=True)
        assert np.array_equal(d["vertices"], pts.cpu().numpy())
        want = colours[f].reshape(-1, 3)[idx.cpu().numpy()]
        assert np.array_equal(np.stack([d["red"], d["green"], d["blue"]], 1), want) and d["red"].dtype == np.uint8
