"""CPU suite of the frame neighbourhood searches (shine_mapping_amd.dataset.knn / statistical_outlier_mask / estimate_normals and
LiDARDataset's filter_noise / estimate_normal): the numpy oracle (tests/frame_nn_oracle.py) on hand-built clouds, the two
conditions the shared scene must meet for the GPU suite's exact comparisons, the constructor's acceptance and refusals, and the
argument checks of the three entry points (csrc/shine_frame_nn.hip).  Nothing here needs a GPU; the device runs are in
tests/test_gpu_frame_nn.py."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frame_nn_oracle as fno

SOR = dict(sor_nn=25, sor_std=2.5)
NORMAL = dict(normal_radius_m=0.2, normal_max_nn=20)


# ---- the oracle on hand-built clouds --------------------------------------------------------------------------------------------
def test_oracle_on_a_line_of_equally_spaced_points():
    n = 10
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n, dtype=np.float64)
    idx, d2, count = fno.knn(p, 3)
    assert count.tolist() == [3] * n
    # the point itself first; of the two neighbours at distance 1 the lower index first; the ends reach two steps inwards
    assert idx[0].tolist() == [0, 1, 2] and d2[0].tolist() == [0.0, 1.0, 4.0]
    assert idx[4].tolist() == [4, 3, 5] and d2[4].tolist() == [0.0, 1.0, 1.0]
    assert idx[9].tolist() == [9, 8, 7] and d2[9].tolist() == [0.0, 1.0, 4.0]
    keep, avg, threshold = fno.sor(p, 3, 1.0)
    want = np.array([1.0] + [2.0 / 3.0] * (n - 2) + [1.0])
    assert np.allclose(avg, want, rtol=1e-15, atol=0)
    mean = want.sum() / n
    std = math.sqrt(((want - mean) ** 2).sum() / (n - 1))
    assert abs(threshold - (mean + std)) <= 1e-15 and keep.tolist() == [False] + [True] * (n - 2) + [False]
    # radius: distance 1 is inside radius 1 (<=), distance 2 is not
    idx, d2, count = fno.knn(p, 3, radius=1.0)
    assert count.tolist() == [2] + [3] * (n - 2) + [2] and idx[0].tolist() == [0, 1, -1] and d2[0, 2] == np.inf
    # k = 1: every mean distance is the point's own 0 and everything is dropped
    keep, avg, _ = fno.sor(p, 1, 2.0)
    assert not avg.any() and not keep.any()
    # a straight line has no normal plane: the oracle still returns unit vectors
    nrm, lam, count, fallback = fno.normals(p, 2.5, 5)
    assert not fallback.any() and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-14)
    assert np.allclose(np.abs(nrm[:, 0]), 0.0, atol=1e-12)  # (orthogonal to the line, whichever way)


def test_oracle_normal_of_a_flat_patch_faces_the_viewpoint():
    g = np.arange(6, dtype=np.float64) * 0.1
    x, y = np.meshgrid(g, g, indexing="ij")
    p = np.stack([x.ravel() + 3.0, y.ravel() - 1.0, np.full(x.size, 2.0)], 1)  # the plane z = 2 above the sensor
    nrm, lam, count, fallback = fno.normals(p, 0.25, 20)
    assert not fallback.any() and count.min() >= 3
    assert np.allclose(nrm, [[0.0, 0.0, -1.0]] * len(p), atol=1e-12)  # n . (0 - p) >= 0: downwards, towards the origin
    assert np.all(np.abs(lam[:, 0]) <= 1e-15) and np.all(fno.relative_gap(lam) > 0.1)
    nrm_up, _, _, _ = fno.normals(p, 0.25, 20, viewpoint=(3.0, -1.0, 10.0))
    assert np.allclose(nrm_up, [[0.0, 0.0, 1.0]] * len(p), atol=1e-12)
    # fewer than 3 neighbours inside the radius: open3d's fallback (0, 0, 1), then the same flip
    nrm, lam, count, fallback = fno.normals(p, 0.05, 20)
    assert fallback.all() and count.tolist() == [1] * len(p) and np.array_equal(nrm, np.tile([0.0, 0.0, -1.0], (len(p), 1)))


def test_oracle_with_fewer_points_than_k_and_with_one_point():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(7, 3))
    idx, d2, count = fno.knn(p, 25)
    assert count.tolist() == [7] * 7 and np.all(idx[:, 7:] == -1) and np.all(np.isinf(d2[:, 7:]))
    assert np.all(np.sort(idx[:, :7], axis=1) == np.arange(7)) and np.all(np.diff(d2[:, :7], axis=1) >= 0)
    keep, avg, threshold = fno.sor(p, 25, 2.0)
    assert np.allclose(avg, np.sqrt(fno.dist2_matrix(p)).sum(1) / 7, rtol=1e-15)
    keep, avg, threshold = fno.sor(p[:1], 25, 2.0)  # n == 1: std is defined as 0, the point (avg = 0) is dropped
    assert avg.tolist() == [0.0] and threshold == 0.0 and keep.tolist() == [False]
    # exact duplicates: all distances 0, neighbours in index order, no direction -> the fallback normal
    dup = np.tile([[4.0, -2.0, 1.0]], (6, 1))
    idx, d2, count = fno.knn(dup, 4)
    assert idx.tolist() == [[0, 1, 2, 3]] * 6 and not d2.any()
    nrm, _, _, fallback = fno.normals(dup, 0.2, 20)
    assert fallback.all() and np.array_equal(nrm, np.tile([0.0, 0.0, -1.0], (6, 1)))


# ---- the shared scene's conditions (not measurements: the GPU suite's exact comparisons rest on them) ------------------------------
def test_scene_meets_the_conditions_of_the_exact_comparisons():
    r = fno.scene_results()
    p = r["points"]
    assert p.shape == (3945, 3)
    ok = ~r["fallback"]
    gap = fno.relative_gap(r["lam"][ok])
    margin = np.abs(r["avg"] - r["threshold"]).min() / r["threshold"]
    print("scene: smallest (l1 - l0) / l2 = %.3e over %d points; %d fallback normals; SOR keeps %d of %d; min |avg - thr| / thr = %.3e"
          % (gap.min(), ok.sum(), r["fallback"].sum(), r["keep"].sum(), len(p), margin))
    # (a) every point with >= 3 neighbours has a usable gap: nothing is excluded from the normal comparison on this scene
    assert gap.min() >= 1e-3
    assert np.array_equal(r["fallback"], r["count"] < 3) and 30 <= r["fallback"].sum() <= 45  # (the sparse outliers)
    # (b) no mean distance sits at the threshold: the keep mask can be demanded exactly
    assert margin > 1e-6
    assert 0 < (~r["keep"]).sum() <= 45 and r["keep"][:3900].all()  # only sparse points (and duplicates' avg > 0) are at stake
    # the widening is forced: some point's 25th neighbour is metres away
    assert np.sqrt(r["sorted"][1][:, fno.SCENE_K - 1]).max() > 10.0


# ---- the constructor ----------------------------------------------------------------------------------------------------------------
def make_cfg(tmp_path, **over):
    pc = tmp_path / "velodyne"
    pc.mkdir(exist_ok=True)
    for k in range(3):
        (pc / ("%d.bin" % k)).write_bytes(b"")
    poses = tmp_path / "poses.txt"
    poses.write_text("\n".join("1 0 0 %d 0 1 0 0 0 0 1 0" % k for k in range(3)) + "\n")
    cfg = SimpleNamespace(
        device="cuda", dtype=torch.float32, pc_path=str(pc), pose_path=str(poses), calib_path="", first_frame_ref=True,
        begin_frame=0, end_frame=2, every_frame=1, pc_count_gpu_limit=500, global_shift_default=0.0, seed=42, min_range=1.5,
        pc_radius=25.0, min_z=-3.0, max_z=30.0, rand_downsample=False, vox_down_m=0.05, rand_down_r=1.0, map_vox_down_m=0.2,
        estimate_normal=False, filter_noise=False, semantic_on=False, behind_dropoff_on=False, octree_from_surface_samples=True,
        surface_sample_range_m=0.3, surface_sample_n=3, free_sample_begin_ratio=0.3, free_sample_end_dist_m=1.0, free_sample_n=3,
        clearance_dist_m=0.3, clearance_sample_n=0, continual_learning_reg=False, window_replay_on=False, window_radius=50.0,
        ray_loss=False, bs=256, scale=0.01)
    cfg.__dict__.update(over)
    return cfg


def test_constructor_serves_both_options_once_their_parameters_are_present(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset

    ds = LiDARDataset(make_cfg(tmp_path, filter_noise=True, **SOR))
    assert ds.filter_noise and not ds.estimate_normal and "normal_label" not in ds._kept_pools()
    ds = LiDARDataset(make_cfg(tmp_path, estimate_normal=True, **NORMAL))
    assert ds.estimate_normal and not ds.filter_noise and ds._kept_pools()[-1] == "normal_label"
    assert ds.normal_label_pool.shape == (0, 3) and ds.normal_label_pool.dtype == torch.float32
    ds = LiDARDataset(make_cfg(tmp_path, estimate_normal=True, filter_noise=True, ray_loss=True, **SOR, **NORMAL))
    assert ds.estimate_normal and ds.filter_noise and ds._kept_pools() == ("coord", "weight", "sample_depth", "ray_depth", "normal_label")
    ds = LiDARDataset(make_cfg(tmp_path, **SOR, **NORMAL))  # parameters alone switch nothing on
    assert not ds.estimate_normal and not ds.filter_noise and "normal_label" not in ds._pools


def test_constructor_refuses_an_option_without_its_parameters_by_name(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset

    with pytest.raises(NotImplementedError, match=r"filter_noise.*sor_nn.*sor_std"):
        LiDARDataset(make_cfg(tmp_path, filter_noise=True))
    with pytest.raises(NotImplementedError, match=r"filter_noise.*without config\.sor_std$"):
        LiDARDataset(make_cfg(tmp_path, filter_noise=True, sor_nn=25))
    with pytest.raises(NotImplementedError, match=r"estimate_normal.*normal_radius_m.*normal_max_nn"):
        LiDARDataset(make_cfg(tmp_path, estimate_normal=True, **SOR))
    with pytest.raises(NotImplementedError, match=r"estimate_normal.*without config\.normal_max_nn$"):
        LiDARDataset(make_cfg(tmp_path, estimate_normal=True, normal_radius_m=0.2))
    ds = LiDARDataset(make_cfg(tmp_path, filter_noise=True, estimate_normal=True, **SOR, **NORMAL))
    with pytest.raises(NotImplementedError, match=r"\.pcd"):
        ds.read_point_cloud(str(tmp_path / "scan.pcd"))


@pytest.mark.parametrize("name, over", [
    ("sor_nn", dict(filter_noise=True, sor_nn=0, sor_std=2.5)), ("sor_nn", dict(filter_noise=True, sor_nn=33, sor_std=2.5)),
    ("sor_nn", dict(filter_noise=True, sor_nn=2.5, sor_std=2.5)), ("sor_std", dict(filter_noise=True, sor_nn=25, sor_std=0.0)),
    ("normal_max_nn", dict(estimate_normal=True, normal_radius_m=0.2, normal_max_nn=0)),
    ("normal_max_nn", dict(estimate_normal=True, normal_radius_m=0.2, normal_max_nn=33)),
    ("normal_radius_m", dict(estimate_normal=True, normal_radius_m=-1.0, normal_max_nn=20)),
    ("normal_radius_m", dict(estimate_normal=True, normal_radius_m=float("inf"), normal_max_nn=20))])
def test_constructor_names_the_limit_of_out_of_range_parameters(tmp_path, name, over):
    from shine_mapping_amd.dataset import LiDARDataset

    with pytest.raises(ValueError, match=name) as e:
        LiDARDataset(make_cfg(tmp_path, **over))
    if name in ("sor_nn", "normal_max_nn"):
        assert "1..32" in str(e.value)


def test_the_three_functions_check_their_arguments_before_touching_a_device():
    from shine_mapping_amd import _lib
    from shine_mapping_amd.dataset import estimate_normals, knn, statistical_outlier_mask

    p = torch.zeros((5, 3), dtype=torch.float64)
    for k in (0, 33, 2.5):
        with pytest.raises(ValueError, match=r"1\.\.32"):
            knn(p, k)
        with pytest.raises(ValueError, match=r"1\.\.32"):
            estimate_normals(p, 0.2, k)
    with pytest.raises(ValueError, match=r"1\.\.32"):
        statistical_outlier_mask(p, 33, 2.0)
    for nb, ratio in ((0, 2.0), (-1, 2.0), (25, 0.0), (25, -1.0)):
        with pytest.raises(ValueError, match="nb_neighbors"):
            statistical_outlier_mask(p, nb, ratio)
    with pytest.raises(ValueError, match="radius"):
        knn(p, 3, radius=-0.1)
    with pytest.raises(ValueError, match="radius"):
        estimate_normals(p, float("nan"), 20)
    for call in (lambda: knn(p, 3), lambda: statistical_outlier_mask(p, 3, 2.0), lambda: estimate_normals(p, 0.2, 20)):
        with pytest.raises(_lib.ShineHipError, match="device only"):
            call()  # (host tensors: there is no CPU path)


def test_entry_points_answer_the_workspace_query_and_reject_bad_arguments_on_the_host():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    INVALID = -1
    need = C.c_size_t(0)
    n = 5000
    grid = (n, 400, 20, None, 0.3, None)
    assert lib.shine_knn_search(None, *grid, 25, -1.0, None, C.byref(need), None, None, None, None, None) == 0
    assert need.value >= 2 * 4 * n + 4
    knn_need = need.value
    assert lib.shine_sor_mean_dist(None, *grid, 25, None, C.byref(need), None, None, None, None) == 0 and need.value == knn_need
    assert lib.shine_frame_normals(None, *grid, 0.2, 20, None, None, C.byref(need), None, None) == 0 and need.value == knn_need
    # sizes and k are checked before anything else
    assert lib.shine_knn_search(None, *grid, 0, -1.0, None, C.byref(need), None, None, None, None, None) == INVALID
    assert b"shine_knn_search" in lib.shine_error_string(INVALID) and b"1..32" in lib.shine_error_string(INVALID)
    assert lib.shine_knn_search(None, *grid, 33, -1.0, None, C.byref(need), None, None, None, None, None) == INVALID
    assert lib.shine_sor_mean_dist(None, *grid, 33, None, C.byref(need), None, None, None, None) == INVALID
    assert lib.shine_frame_normals(None, *grid, 0.2, 0, None, None, C.byref(need), None, None) == INVALID
    assert b"max_nn" in lib.shine_error_string(INVALID)
    assert lib.shine_knn_search(None, 0, 0, 0, None, 0.3, None, 3, -1.0, None, C.byref(need), None, None, None, None, None) == INVALID
    assert lib.shine_knn_search(None, 1 << 31, 4, 2, None, 0.3, None, 3, -1.0, None, C.byref(need), None, None, None, None, None) == INVALID
    assert lib.shine_knn_search(None, n, n + 1, 2, None, 0.3, None, 3, -1.0, None, C.byref(need), None, None, None, None, None) == INVALID
    assert lib.shine_knn_search(None, *grid, 3, -1.0, None, None, None, None, None, None, None) == INVALID
    # with a workspace: too small, null outputs, null grid, bad radius, cells_per_axis out of range — all before any launch
    p = 256  # a non-null dummy address: every call below fails its checks before anything is dereferenced or launched
    big, small = C.c_size_t(1 << 30), C.c_size_t(16)
    o3, cells, bad_cells = (C.c_double * 3)(0, 0, 0), (C.c_int64 * 3)(10, 10, 10), (C.c_int64 * 3)(10, 0, 10)
    assert lib.shine_knn_search(p, n, 400, 20, o3, 0.3, cells, 3, -1.0, p, C.byref(small), p, p, p, None, None) == INVALID
    assert b"workspace too small" in lib.shine_error_string(INVALID)
    assert lib.shine_knn_search(p, n, 400, 20, o3, 0.3, cells, 3, -1.0, p, C.byref(big), None, p, p, None, None) == INVALID
    assert lib.shine_knn_search(p, n, 400, 20, o3, 0.3, cells, 3, float("nan"), p, C.byref(big), p, p, p, None, None) == INVALID
    assert lib.shine_knn_search(None, n, 400, 20, o3, 0.3, cells, 3, -1.0, p, C.byref(big), p, p, p, None, None) == INVALID
    assert lib.shine_knn_search(p, n, 400, 20, o3, 0.0, cells, 3, -1.0, p, C.byref(big), p, p, p, None, None) == INVALID
    assert lib.shine_knn_search(p, n, 400, 20, o3, 0.3, bad_cells, 3, -1.0, p, C.byref(big), p, p, p, None, None) == INVALID
    assert b"cells_per_axis" in lib.shine_error_string(INVALID)
    assert lib.shine_sor_mean_dist(p, n, 400, 20, o3, 0.3, cells, 3, p, C.byref(big), p, None, None, None) == INVALID
    assert lib.shine_frame_normals(p, n, 400, 20, o3, 0.3, cells, -0.1, 20, o3, p, C.byref(big), p, None) == INVALID
    assert lib.shine_frame_normals(p, n, 400, 20, o3, 0.3, cells, float("inf"), 20, o3, p, C.byref(big), p, None) == INVALID
    assert lib.shine_frame_normals(p, n, 400, 20, o3, 0.3, cells, 0.2, 20, None, p, C.byref(big), p, None) == INVALID
    assert b"shine_frame_normals" in lib.shine_error_string(INVALID)
