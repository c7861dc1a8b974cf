"""GPU suite of the frame neighbourhood searches (csrc/shine_frame_nn.hip; shine_mapping_amd.dataset.knn, statistical_outlier_mask,
estimate_normals) and of LiDARDataset / RGBDDataset with config.filter_noise and config.estimate_normal:
  * the three functions against the numpy brute-force oracle (tests/frame_nn_oracle.py) on the shared scene — whose conditions
    tests/test_frame_nn.py asserts on the CPU — and on small and degenerate clouds;
  * the datasets end to end on a small synthetic KITTI-format drive with outliers added to its scans.
Bounds (all from the number formats, none from what the kernels return):
  d2          1e-13 relative + 1e-300: both sides add three fp64 products of the same differences
  mean_dist,  1e-12 relative: at most 32 correctly rounded square roots and their sum are ~4e-15; the margin covers the order
  threshold   of the sums
  normals     sin(angle to the oracle's) <= 1e-9 where the oracle's relative eigenvalue gap is >= 1e-3: a backward-stable fp64
              eigen solve gives ~eps * l2 / gap ~ 1e-13, four more orders cover the covariance's own rounding
Every comparison prints its figures before it asserts."""
import math
import os

import numpy as np
import pytest
import torch

import frame_nn_oracle as fno

pytestmark = pytest.mark.gpu

TIE = 1e-12      # neighbouring sorted distances closer than this (relative) may come in either order
TIE_SHARE = 0.05  # at most this share of the points may hold such a pair


@pytest.fixture(scope="module")
def scene():
    r = fno.scene_results()
    return r, torch.from_numpy(r["points"]).cuda()


def _check_knn(points_np, got, k, radius, sorted_=None, what=""):
    """count exact, d2 within the bound, indices equal wherever the oracle's order is not a near-tie; -> share of points excluded"""
    order, d2_sorted = sorted_ if sorted_ is not None else fno.sorted_neighbours(points_np)
    want_idx, want_d2, want_count = fno.knn(points_np, k, radius, (order, d2_sorted))
    idx, d2, count = (t.cpu().numpy() for t in got)
    n = len(points_np)
    assert idx.shape == (n, k) and d2.shape == (n, k) and count.shape == (n,) and idx.dtype == np.int32 and count.dtype == np.int32
    assert np.array_equal(count, want_count), "%s: %d counts differ" % (what, (count != want_count).sum())
    found = want_idx >= 0
    assert np.array_equal(idx >= 0, found) and np.all(np.isinf(d2[~found])) and np.all(d2[~found] > 0)
    err = np.abs(d2[found] - want_d2[found])
    bound = 1e-13 * want_d2[found] + 1e-300
    print("%s k=%d radius=%s: max |d2 - oracle| / bound = %.3e (bit-identical: %s)"
          % (what, k, radius, (err / bound).max(), np.array_equal(d2[found], want_d2[found])))
    assert np.all(err <= bound)
    assert np.all(found[:, :-1] | ~found[:, 1:])  # the padding comes last ...
    assert np.all(d2[:, 1:][found[:, 1:]] >= d2[:, :-1][found[:, 1:]])  # ... behind ascending distances
    # near-ties of the oracle's order among the first k + 1 (the pair (k-1, k) decides who is the last neighbour)
    m = min(k + 1, n)
    head = d2_sorted[:, :m]
    near = np.zeros((n, k + 1), dtype=bool)  # near[:, t]: sorted entries t and t + 1 are a near-tie
    near[:, :m - 1] = np.diff(head, axis=1) <= TIE * head[:, 1:]
    unsure = near[:, :k].copy()
    unsure[:, 1:] |= near[:, :k - 1] if k > 1 else False
    unsure &= found
    excluded = unsure.any(1).mean()
    print("%s k=%d radius=%s: %.2f %% of the points hold a near-tie" % (what, k, radius, 100 * excluded))
    compare = found & ~unsure
    assert np.array_equal(idx[compare], want_idx[compare]), "%s: %d indices differ" % (what, (idx[compare] != want_idx[compare]).sum())
    # exact ties in OUR list are ordered by lower index
    tie = (d2[:, 1:] == d2[:, :-1]) & found[:, 1:]
    assert np.all(idx[:, 1:][tie] > idx[:, :-1][tie])
    return excluded


def _expected_launches(pts, d2_sorted, k, radius):
    """how many search launches the widening rule makes: one for a bounded search; else the radius starts at one coarse cell edge
    (at the grid's diagonal if no list can fill) and doubles while some point's k-th neighbour lies outside it and it does not yet
    hold the grid"""
    from shine_mapping_amd import evaluation as ev

    n = d2_sorted.shape[0]
    if radius is not None or n <= k:
        return 1
    grid = ev.NNGrid(pts)
    diag = math.sqrt(sum((float(c) * grid.cell) ** 2 for c in grid.cells_per_axis)) * (1.0 + 2.0 ** -20)
    worst = d2_sorted[:, k - 1].max()
    r, launches = grid.coarse_cell, 1
    while r < diag and worst > r * r:
        r, launches = 2.0 * r, launches + 1
    return launches


@pytest.mark.parametrize("radius", [None, 0.2])
@pytest.mark.parametrize("k", [1, 3, 20, 25, 32])
def test_knn_on_the_scene(scene, k, radius):
    from shine_mapping_amd.dataset import knn

    r, pts = scene
    *got, rounds = knn(pts, k, radius, return_rounds=True)
    torch.cuda.synchronize()
    excluded = _check_knn(r["points"], got, k, radius, r["sorted"], "scene")
    print("scene k=%d radius=%s: %d search launches" % (k, radius, rounds))
    assert excluded <= TIE_SHARE
    assert rounds == _expected_launches(pts, r["sorted"][1], k, radius)
    if radius is None and k >= 20:
        assert rounds > 1  # (the sparse points force the unbounded search to widen)


def _cluster_and_far_point():
    rng = np.random.default_rng(11)
    return np.concatenate([rng.normal(0.0, 0.05, (200, 3)), [[1000.0, 0.0, 0.0]]])


def _one_cell_cloud():
    rng = np.random.default_rng(12)  # 300 points within a millimetre, two far points that make the grid's cells metres wide
    return np.concatenate([2.0 + rng.uniform(0.0, 1e-3, (300, 3)), [[-5.0, -5.0, -5.0], [9.0, 9.0, 9.0]]])


SMALL = {
    "one_point": lambda: np.array([[1.0, 2.0, 3.0]]),
    "seven_points": lambda: np.random.default_rng(3).normal(size=(7, 3)),
    "one_cell": _one_cell_cloud,
    "duplicates": lambda: np.tile([[4.0, -2.0, 1.0]], (50, 1)),
    "far_point": _cluster_and_far_point,
}


@pytest.mark.parametrize("name", list(SMALL))
def test_small_and_degenerate_clouds(name):
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd.dataset import estimate_normals, knn, statistical_outlier_mask

    p = np.ascontiguousarray(SMALL[name](), dtype=np.float64)
    pts = torch.from_numpy(p).cuda()
    n, k = len(p), 25
    s = fno.sorted_neighbours(p)
    grid = ev.NNGrid(pts)
    print("%s: n=%d, %d fine / %d coarse cells of %.4g m" % (name, n, grid.n_fine, grid.n_coarse, grid.cell))
    if name == "one_cell":
        assert grid.n_fine == 3  # the 300 share one cell
    for radius in (None, 0.1):
        *got, rounds = knn(pts, k, radius, return_rounds=True)
        torch.cuda.synchronize()
        excluded = _check_knn(p, got, k, radius, s, name)
        print("%s radius=%s: %d search launches" % (name, radius, rounds))
        assert rounds == _expected_launches(pts, s[1], k, radius)  # the widening reaches what it must and then stops
        if name not in ("duplicates",):  # (a cloud of copies is nothing but ties; its order is checked exactly by _check_knn)
            assert excluded <= TIE_SHARE
    if name == "far_point":  # the widening reached the lonely point: its neighbours are itself and the cluster's nearest 24
        idx, d2, count, rounds = knn(pts, k, return_rounds=True)
        assert int(count[200]) == k and int(idx[200, 0]) == 200 and float(d2[200, 1]) > 990.0 ** 2
        assert 1 < rounds <= 12
    keep, avg, threshold = statistical_outlier_mask(pts, k, 2.0)
    want_keep, want_avg, want_thr = fno.sor(p, k, 2.0, s)
    err = np.abs(avg.cpu().numpy() - want_avg)
    print("%s: max |avg - oracle| = %.3e, threshold %.17g (oracle %.17g)" % (name, err.max(), threshold, want_thr))
    assert np.all(err <= 1e-12 * want_avg) and abs(threshold - want_thr) <= 1e-12 * want_thr
    if np.abs(want_avg - want_thr).min() > 1e-6 * max(want_thr, 1e-300) or want_thr == 0.0:
        assert np.array_equal(keep.cpu().numpy(), want_keep)
    if name in ("one_point", "duplicates"):
        assert not keep.any() and not avg.any() and threshold == 0.0  # nothing but zero distances: everything is dropped
    nrm = estimate_normals(pts, 0.1, 20).cpu().numpy()
    want_nrm, lam, count, fallback = fno.normals(p, 0.1, 20, sorted_=s)
    assert np.all(np.isfinite(nrm)) and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-12
    assert np.all((nrm * -p).sum(1) >= 0.0)
    if name in ("one_point", "seven_points", "duplicates"):
        assert fallback.all() and np.array_equal(nrm, want_nrm)


def test_statistical_outlier_mask_on_the_scene(scene):
    from shine_mapping_amd.dataset import statistical_outlier_mask

    r, pts = scene
    keep, avg, threshold, rounds = statistical_outlier_mask(pts, fno.SCENE_K, fno.SCENE_STD_RATIO, return_rounds=True)
    torch.cuda.synchronize()
    assert keep.dtype == torch.bool and avg.dtype == torch.float64 and isinstance(threshold, float)
    rel = np.abs(avg.cpu().numpy() - r["avg"]) / r["avg"]
    rel_thr = abs(threshold - r["threshold"]) / r["threshold"]
    print("SOR on the scene: max relative error of mean_dist %.3e, of the threshold %.3e; keeps %d of %d; %d search launches"
          % (rel.max(), rel_thr, int(keep.sum()), len(rel), rounds))
    assert rel.max() <= 1e-12 and rel_thr <= 1e-12
    assert np.array_equal(keep.cpu().numpy(), r["keep"])
    assert rounds > 1
    keep2, avg2, threshold2 = statistical_outlier_mask(pts, fno.SCENE_K, fno.SCENE_STD_RATIO)
    assert torch.equal(avg, avg2) and threshold == threshold2 and torch.equal(keep, keep2)  # the same bits on a second run
    keep1, avg1, threshold1 = statistical_outlier_mask(pts, 1, fno.SCENE_STD_RATIO)
    assert not avg1.any() and threshold1 == 0.0 and not keep1.any()  # k = 1: only the point's own zero distance


def test_estimate_normals_on_the_scene(scene):
    from shine_mapping_amd.dataset import estimate_normals

    r, pts = scene
    p = r["points"]
    nrm = estimate_normals(pts, fno.SCENE_RADIUS, fno.SCENE_MAX_NN)
    torch.cuda.synchronize()
    assert nrm.shape == (len(p), 3) and nrm.dtype == torch.float64
    nrm = nrm.cpu().numpy()
    assert np.all(np.isfinite(nrm))
    unit = np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max()
    toward = (nrm * -p).sum(1)
    print("normals on the scene: max | |n| - 1 | = %.3e, min n . (0 - p) = %.3e" % (unit, toward.min()))
    assert unit <= 1e-12 and np.all(toward >= 0.0)
    fb = r["fallback"]
    want_fb = np.zeros((int(fb.sum()), 3))
    want_fb[:, 2] = np.where(p[fb, 2] > 0.0, -1.0, 1.0)  # exactly (0, 0, 1) before the flip
    assert np.array_equal(nrm[fb], want_fb)
    gap = fno.relative_gap(r["lam"])
    ok = ~fb & (gap >= 1e-3)
    excluded = 1.0 - ok[~fb].mean()
    sin = np.linalg.norm(np.cross(nrm[ok], r["normals"][ok]), axis=1)
    print("normals on the scene: max sin(angle to the oracle) = %.3e over %d points (%.2f %% excluded for a gap below 1e-3)"
          % (sin.max(), ok.sum(), 100 * excluded))
    assert excluded == 0.0  # (tests/test_frame_nn.py: the scene has no such point)
    assert sin.max() <= 1e-9
    decided = ok & (np.abs((r["normals"] * -p).sum(1)) > 1e-6)
    assert np.all((nrm[decided] * r["normals"][decided]).sum(1) > 0.0)  # the same side wherever the flip is not a coin toss
    # another viewpoint: the same lines, turned towards it
    vp = np.array([30.0, -40.0, 50.0])
    other = estimate_normals(pts, fno.SCENE_RADIUS, fno.SCENE_MAX_NN, viewpoint=vp).cpu().numpy()
    assert np.all((other * (vp - p)).sum(1) >= 0.0) and np.array_equal(np.abs(other), np.abs(nrm))


def test_collinear_neighbourhoods_give_finite_unit_normals():
    from shine_mapping_amd.dataset import estimate_normals

    t = np.arange(50, dtype=np.float64)[:, None] * 0.05
    for direction in ([1.0, 0.0, 0.0], [1.0, 2.0, -0.5]):
        d = np.asarray(direction) / np.linalg.norm(direction)
        p = np.array([3.0, -2.0, 1.0]) + t * d
        nrm = estimate_normals(torch.from_numpy(p).cuda(), 0.3, 20).cpu().numpy()
        print("line along %s: max | |n| - 1 | = %.3e, max |n . line| = %.3e"
              % (direction, np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max(), np.abs(nrm @ d).max()))
        assert np.all(np.isfinite(nrm)) and np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-12
        assert np.all((nrm * -p).sum(1) >= 0.0)


# ---- the datasets ---------------------------------------------------------------------------------------------------------------------
FRAMES = 4
OPTIONS = dict(estimate_normal=True, filter_noise=True, sor_nn=10, sor_std=2.0, normal_radius_m=1.0, normal_max_nn=20, vox_down_m=0.2)


@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    """a labelled drive whose scans carry 30 extra points each, uniform inside the crop box: the noise filter_noise is for"""
    from shine_mapping_amd import synth

    folder = str(tmp_path_factory.mktemp("nn_drive"))
    d = synth.write_kitti_drive(folder, synth.make_config("ncd", device="cuda"), frames=FRAMES, beams=32, azimuths=180,
                                device="cpu", labels=True)
    rng = np.random.default_rng(5)
    for f in range(FRAMES):
        scan = os.path.join(d.pc_path, "%06d.bin" % f)
        label = os.path.join(d.label_path, "%06d.label" % f)
        extra = np.zeros((30, 4), dtype=np.float32)
        extra[:, :3] = rng.uniform([-18.0, -18.0, -2.0], [18.0, 18.0, 12.0], (30, 3))
        np.concatenate([np.fromfile(scan, dtype=np.float32).reshape(-1, 4), extra]).tofile(scan)
        np.concatenate([np.fromfile(label, dtype=np.uint32), np.full(30, 40, dtype=np.uint32)]).tofile(label)
    return d


def _dataset(drive, with_octree=True, **over):
    from shine_mapping_amd import FeatureOctree, synth
    from shine_mapping_amd.dataset import LiDARDataset

    cfg = synth.dataset_config("ncd", drive, **dict(dict(pc_radius=20.0, min_range=2.5), **over))
    torch.manual_seed(1)
    octree = FeatureOctree(cfg) if with_octree else None
    return cfg, octree, LiDARDataset(cfg, octree)


def _rotate(normals, pose):
    """R n in fp64, products summed left to right, then the cast: what process_frame stores"""
    R = np.asarray(pose, dtype=np.float64)[:3, :3]
    x, y, z = normals[:, 0], normals[:, 1], normals[:, 2]
    return torch.stack([x * float(R[r, 0]) + y * float(R[r, 1]) + z * float(R[r, 2]) for r in range(3)], 1).float()


def _by_hand(ds, cfg, f):
    """the frame's points and normals in the sensor frame, assembled from the public pieces"""
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd.dataset import estimate_normals, frame_filter, statistical_outlier_mask

    raw = ds.read_point_cloud(os.path.join(cfg.pc_path, ds.pc_filenames[f]))
    pts = frame_filter(raw, cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius)
    nrm = estimate_normals(pts, cfg.normal_radius_m, cfg.normal_max_nn)
    down, mean = ev.voxel_down_sample(pts, cfg.vox_down_m, attrs=nrm)
    keep = statistical_outlier_mask(down, cfg.sor_nn, cfg.sor_std)[0]
    return down[keep], mean[keep], int(down.shape[0])


def test_frame_points_equal_the_pipeline_assembled_by_hand(drive):
    cfg, _, ds = _dataset(drive, with_octree=False, **OPTIONS)
    for f in range(2):
        want_pts, want_nrm, before = _by_hand(ds, cfg, f)
        got = ds.frame_points(f)
        print("frame %d: %d points after down-sampling, %d after filter_noise; mean |n| of the voxel means %.4f"
              % (f, before, got.shape[0], float(ds.cur_frame_normals.norm(dim=1).mean())))
        assert 1000 <= got.shape[0] < before  # (thousands of points, and the filter dropped some)
        assert torch.equal(got, want_pts) and torch.equal(ds.cur_frame_normals, want_nrm)
        assert float(ds.cur_frame_normals.norm(dim=1).max()) <= 1.0 + 1e-12  # means of unit vectors, NOT re-normalised
    # the seeded random subset takes the same rows of points and normals
    cfg_r, _, ds_r = _dataset(drive, with_octree=False, **dict(OPTIONS, rand_downsample=True, rand_down_r=0.3, filter_noise=False))
    from shine_mapping_amd.dataset import estimate_normals, frame_filter, random_subset

    raw = ds_r.read_point_cloud(os.path.join(cfg_r.pc_path, ds_r.pc_filenames[1]))
    pts = frame_filter(raw, cfg_r.min_z, cfg_r.max_z, cfg_r.min_range, cfg_r.pc_radius)
    sub = random_subset(int(pts.shape[0]), int(pts.shape[0] * 0.3), ds_r.seed, 1, pts.device)
    assert torch.equal(ds_r.frame_points(1), pts[sub])
    assert torch.equal(ds_r.cur_frame_normals, estimate_normals(pts, cfg_r.normal_radius_m, cfg_r.normal_max_nn)[sub])


def test_incremental_mode_replaces_the_normal_pool_with_the_rotated_normals(drive):
    cfg, octree, ds = _dataset(drive, **OPTIONS)
    S = ds.sampler.S
    for f in (0, 2):
        ds.process_frame(f, incremental_on=True)
        nrm = ds.cur_frame_normals
        m = int(nrm.shape[0])
        pool = ds.normal_label_pool
        assert pool.shape == (m * S, 3) == tuple(ds.coord_pool.shape) and pool.dtype == torch.float32 and pool.is_cuda
        want = _rotate(nrm, ds.poses_ref[f])
        assert torch.equal(pool.view(m, S, 3), want[:, None, :].expand(m, S, 3))  # row i * S + j: the normal of ray i
    assert not np.allclose(ds.poses_ref[2][:3, :3], np.eye(3))  # (the pose really turns them)
    assert not torch.equal(want, nrm.float())


@pytest.mark.parametrize("semantic", [False, True], ids=["plain", "semantic"])
def test_batch_mode_with_window_replay_keeps_the_normal_pool_aligned(drive, semantic):
    cfg, octree, ds = _dataset(drive, window_replay_on=True, window_radius=8.0, semantic_on=semantic, bs=48, **OPTIONS)
    S = ds.sampler.S
    want_nrm = torch.empty((0, 3), device="cuda")
    want_coord = torch.empty((0, 3), device="cuda")
    dropped = 0
    for f in range(FRAMES):
        prev = ds.coord_pool.clone()
        ds.process_frame(f)
        origin = torch.tensor((ds.poses_ref[f][:3, 3] * cfg.scale).astype(np.float32), device="cuda")
        mask = (prev - origin).norm(2, dim=-1) < cfg.window_radius * cfg.scale  # the reference's window, in torch
        dropped += int((~mask).sum())
        m = int(ds.cur_frame_normals.shape[0])
        rows = _rotate(ds.cur_frame_normals, ds.poses_ref[f])[:, None, :].expand(m, S, 3).reshape(m * S, 3)
        want_nrm = torch.cat([want_nrm[mask], rows])
        want_coord = torch.cat([want_coord[mask], ds.coord_pool[-m * S:]])
        assert ds.normal_label_pool.shape == ds.coord_pool.shape == want_nrm.shape
        assert torch.equal(ds.coord_pool, want_coord) and torch.equal(ds.normal_label_pool, want_nrm)
        if semantic:
            assert ds.sem_label_pool.shape[0] == ds.coord_pool.shape[0]
    print("window replay (%s): %d rows left the pool over %d frames, %d remain" % (
        "semantic" if semantic else "plain", dropped, FRAMES, ds.coord_pool.shape[0]))
    assert dropped > 0
    _check_batch_rows(cfg, ds, semantic)


def _check_batch_rows(cfg, ds, semantic, ray=False):
    """get_batch's normal_label (and sem_label) belong to the coord rows it returns"""
    batch = ds.get_batch()
    coord, normal_label, sem_label = batch[0], batch[3 if ray else 4], batch[4 if ray else 5]
    assert normal_label.shape == coord.shape and normal_label.dtype == torch.float32 and normal_label.is_cuda
    pool_coord, pool_nrm = ds.coord_pool.to(coord.device), ds.normal_label_pool.to(coord.device)
    row = torch.empty(coord.shape[0], dtype=torch.long, device=coord.device)
    for b in range(coord.shape[0]):  # (the first pool row with exactly this coordinate)
        hit = torch.nonzero((pool_coord == coord[b]).all(1))
        assert hit.numel() >= 1
        row[b] = hit[0, 0]
    assert torch.equal(normal_label, pool_nrm[row])
    if semantic:
        pool_sem = ds.sem_label_pool.to(coord.device).long()
        if ray:  # (one label per ray: that of the ray's first sample)
            R = ds.ray_sample_count
            assert torch.equal(sem_label, pool_sem[row[::R]])
        else:
            assert torch.equal(sem_label, pool_sem[row])
    else:
        assert sem_label is None
    return batch


@pytest.mark.parametrize("mode", ["point", "ray", "cpu_pool", "point_semantic", "ray_semantic"])
def test_get_batch_returns_the_normals_of_its_coord_rows(drive, mode):
    semantic, ray = mode.endswith("semantic"), mode.startswith("ray")
    over = dict(OPTIONS, bs=48, semantic_on=semantic, ray_loss=ray)
    if mode == "cpu_pool":
        over["pc_count_gpu_limit"] = 1
    cfg, octree, ds = _dataset(drive, **over)
    assert ds.to_cpu == (mode == "cpu_pool")
    S, rays = ds.sampler.S, 0
    for f in range(2):
        ds.process_frame(f)  # batch mode appends, in point mode and in ray mode, on the device and in the host pool
        rays += int(ds.cur_frame_normals.shape[0])
        assert ds.normal_label_pool.shape == (rays * S, 3) == tuple(ds.coord_pool.shape)
        assert ds.normal_label_pool.is_cuda == (mode != "cpu_pool")
    m = int(ds.cur_frame_normals.shape[0])
    want = _rotate(ds.cur_frame_normals, ds.poses_ref[1])[:, None, :].expand(m, S, 3).reshape(m * S, 3)
    assert torch.equal(ds.normal_label_pool[-m * S:].cuda(), want)
    batch = _check_batch_rows(cfg, ds, semantic, ray)
    assert batch[0].shape == ((48 * ds.ray_sample_count if ray else 48), 3)


def test_with_both_options_off_the_pools_are_those_of_the_unchanged_stages(drive):
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd.dataset import frame_filter, ray_sample, transform_points

    # (the parameters present, the options off: nothing of the new code may run)
    cfg, octree, ds = _dataset(drive, **dict(OPTIONS, estimate_normal=False, filter_noise=False))
    want = {n: [] for n in ("coord", "sdf_label", "weight", "origin", "time")}
    for f in range(3):
        ds.process_frame(f)
        raw = ds.read_point_cloud(os.path.join(cfg.pc_path, ds.pc_filenames[f]))
        pts = ev.voxel_down_sample(frame_filter(raw, cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius), cfg.vox_down_m)
        pts_s = (transform_points(pts, ds.poses_ref[f]) * cfg.scale).float()
        origin = (ds.poses_ref[f][:3, 3] * cfg.scale).astype(np.float32)
        res = ray_sample(pts_s, origin, ds.sampler, seed=ds.seed, stream_id=f, time_value=float(f), depths=False)
        for n in want:
            want[n].append(res[n])
        assert ds.normal_label_pool is None and ds.cur_frame_normals is None
    for n in want:
        assert torch.equal(getattr(ds, n + "_pool"), torch.cat(want[n])), n
    assert ds.get_batch()[4] is None


def test_a_frame_the_filter_empties_is_refused_by_name(drive):
    cfg, _, ds = _dataset(drive, with_octree=False, **dict(OPTIONS, sor_nn=1))  # k = 1: every mean distance is 0
    with pytest.raises(ValueError, match=r"no point passes filter_noise"):
        ds.frame_points(0)


def test_rgbd_dataset_filters_its_down_sampled_frame(tmp_path):
    from shine_mapping_amd import synth
    from shine_mapping_amd.dataset import statistical_outlier_mask
    from shine_mapping_amd.rgbd import RGBDDataset

    d = synth.write_rgbd_drive(str(tmp_path / "rgbd"), frames=2)
    over = dict(pc_radius=2.0, min_range=0.8, min_z=-3.5, max_z=1.0, vox_down_m=0.03)
    plain = RGBDDataset(synth.rgbd_config("rgbd", d, **over), None)
    cfg = synth.rgbd_config("rgbd", d, filter_noise=True, sor_nn=12, sor_std=1.0, **over)
    filtered = RGBDDataset(cfg, None)
    pts = plain.frame_points(1)
    keep = statistical_outlier_mask(pts, cfg.sor_nn, cfg.sor_std)[0]
    got = filtered.frame_points(1)
    print("RGB-D frame: %d points after down-sampling, %d after filter_noise" % (pts.shape[0], got.shape[0]))
    assert 0 < got.shape[0] < pts.shape[0] and torch.equal(got, pts[keep])
    filtered.process_frame(1)
    assert filtered.coord_pool.shape[0] == got.shape[0] * filtered.sampler.S and filtered.normal_label_pool is None
