"""GPU suite of the semantic frame front-end (shine_mapping_amd/dataset.py with semantic_on, csrc/shine_frame.hip's
shine_sem_frame_filter, csrc/shine_eval.hip's shine_voxel_down_attr):
  * the filter against the reference's own preprocess_sem_kitti (tests/golden/sem_frame.pt) and, with the crop box and the edge
    points, against the numpy fp64 oracle (tests/sem_frame_oracle.py) — exact;
  * voxel means with attributes against the oracle — exact, and the same points / keys as the call without attributes;
  * LiDARDataset on a labelled synthetic drive: the sem_label pool in every mode, get_batch, the coloured map cloud;
  * ingest -> Tier-A training with the semantic head -> a labelled, coloured mesh.
Comparisons are torch.equal / np.array_equal unless a line says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import frame_oracle as fo
import sem_frame_oracle as so
from conftest import load_golden

pytestmark = pytest.mark.gpu

HUGE = 1e30  # a crop box that holds everything: the golden records the label filters alone


class _Map:
    """what sem_frame_filter needs of a LabelMap, around a LUT array"""

    def __init__(self, lut):
        from shine_mapping_amd.semantic_kitti import LabelMap

        self._m = LabelMap({}, None, 20)
        self._m.lut = np.ascontiguousarray(lut, np.int32)
        self.device_lut = self._m.device_lut


def _layouts(p32):
    """the float32 [n,3] values as the three layouts the kernel reads"""
    n = len(p32)
    p4 = np.zeros((n, 4), np.float32)
    p4[:, :3] = p32
    p4[:, 3] = 0.5  # (an intensity the filter must not read as a coordinate)
    return dict(f32x4=torch.from_numpy(p4).cuda(), f32x3=torch.from_numpy(np.ascontiguousarray(p32)).cuda(),
                f64x3=torch.from_numpy(p32.astype(np.float64)).cuda())


def test_sem_frame_filter_equals_the_reference_on_its_golden():
    from shine_mapping_amd.dataset import sem_frame_filter

    fx = load_golden("sem_frame")
    lm = _Map(fx["lut"].numpy())
    for case in fx["cases"]:
        n = int(case["points"].shape[0])
        for name, pts in _layouts(case["points"].numpy()).items():
            got_p, got_c = sem_frame_filter(pts, case["labels"].cuda(), lm, case["min_range"], case["filter_moving"],
                                            case["filter_outlier"], -HUGE, HUGE, HUGE)
            print("n = %d %s moving %d outlier %d: kept %d (reference %d)" % (n, name, case["filter_moving"], case["filter_outlier"],
                                                                             got_p.shape[0], case["points_out"].shape[0]))
            assert got_p.dtype == torch.float64 and got_c.dtype == torch.int32
            assert torch.equal(got_p.cpu(), case["points_out"].double()) and torch.equal(got_c.cpu(), case["classes"])


def _edge_cloud(n, seed, R=25.0, min_z=-3.0, max_z=30.0, rmin=2.5):
    """a float32 cloud that straddles every bound, ids over a small map with 99 / 100 / 1 / 0; the first points are the edges"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.3, 1.3, size=(n, 3)) * np.array([R, R, 0.5 * (max_z - min_z)]) + np.array([0, 0, 0.5 * (max_z + min_z)])
    near = rng.normal(size=(n // 10, 3))
    p[: n // 10] = near / np.linalg.norm(near, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n // 10, 1)) * rmin
    p = p.astype(np.float32)
    ids = np.array([0, 1, 40, 44, 50, 99, 100, 252], np.uint32)[rng.integers(0, 8, n)]
    edges = [([R, 0, 0], 40), ([-R, R, 1.0], 40), ([3.0, 4.0, max_z], 40), ([5.0, 5.0, min_z], 40), ([0, -R, 0], 50),
             ([np.nextafter(np.float32(R), np.float32(1e9)), 0, 0], 40), ([0, 0, np.nextafter(np.float32(max_z), np.float32(1e9))], 40),
             ([0.6 * rmin, 0.8 * rmin, 0.0], 40), ([rmin, 0, 0], 50), ([np.nextafter(np.float32(rmin), np.float32(0)), 0, 0], 50),
             ([9.0, 0, 0], 99), ([9.0, 1, 0], 100), ([9.0, 2, 0], 1), ([9.0, 3, 0], 0)]
    for k, (xyz, s) in enumerate(edges[:n]):
        p[k], ids[k] = xyz, s
    words = ids | (rng.integers(1, 1 << 16, n).astype(np.uint32) << 16)
    lut = np.full(65536, -1, np.int32)
    lut[[0, 1, 40, 44, 50, 99, 100, 252]] = [0, 0, 2, 2, 3, 7, 5, 1]
    return p, words, lut


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 3 * 2048 + 5])
def test_sem_frame_filter_with_the_crop_equals_the_oracle(n):
    from shine_mapping_amd.dataset import sem_frame_filter

    R, min_z, max_z, rmin = 25.0, -3.0, 30.0, 2.5
    p, words, lut = _edge_cloud(n, n)
    lm = _Map(lut)
    labels = torch.from_numpy(words.view(np.int32).copy()).cuda()
    for moving in (True, False):
        for outlier in (True, False):
            idx, cls = so.sem_filter(p.astype(np.float64), words, lut, rmin, moving, outlier, min_z, max_z, R)
            for name, pts in _layouts(p).items():
                if name == "f32x3" and (moving != outlier):
                    continue  # (the two layouts the issue names, plus stride 3 on the diagonal)
                got_p, got_c = sem_frame_filter(pts, labels, lm, rmin, moving, outlier, min_z, max_z, R)
                assert np.array_equal(got_p.cpu().numpy(), p[idx].astype(np.float64)), (name, moving, outlier)
                assert np.array_equal(got_c.cpu().numpy(), cls)
            print("n = %d moving %d outlier %d: kept %d of %d" % (n, moving, outlier, len(idx), n))
    if n >= 2047:
        idx, _ = so.sem_filter(p.astype(np.float64), words, lut, rmin, True, True, min_z, max_z, R)
        assert {0, 1, 2, 3, 4, 7, 8, 10, 13} <= set(idx.tolist()) and not ({5, 6, 9, 11, 12} & set(idx.tolist()))  # the edge points


def test_sem_frame_filter_all_kept_none_kept_and_labels_given_as_uint32_values():
    from shine_mapping_amd.dataset import sem_frame_filter

    p, words, lut = _edge_cloud(2049, 3)
    lm = _Map(lut)
    pts = _layouts(p)["f32x4"]
    # all kept: no range cut, no label filter, a box that holds the cloud — in input order
    got_p, got_c = sem_frame_filter(pts, torch.from_numpy(words.astype(np.int64)).cuda(), lm, 0.0, False, False, -HUGE, HUGE, HUGE)
    assert np.array_equal(got_p.cpu().numpy(), p.astype(np.float64)) and np.array_equal(got_c.cpu().numpy(), lut[words & 0xFFFF])
    # the same labels as a numpy uint32 array
    again = sem_frame_filter(pts, words, lm, 0.0, False, False, -HUGE, HUGE, HUGE)
    assert torch.equal(again[0], got_p) and torch.equal(again[1], got_c)
    # none kept: a range no point reaches / a box beside the cloud
    for args in ((1e6, False, False, -HUGE, HUGE, HUGE), (0.0, False, False, 100.0, 101.0, HUGE)):
        none_p, none_c = sem_frame_filter(pts, words, lm, *args)
        assert none_p.shape == (0, 3) and none_c.shape == (0,) and none_c.dtype == torch.int32
    e = sem_frame_filter(torch.empty((0, 4), device="cuda"), np.zeros(0, np.uint32), lm, 0.0, True, True, -3.0, 30.0, 25.0)
    assert e[0].shape == (0, 3) and e[1].shape == (0,)
    with pytest.raises(ValueError, match="labels"):
        sem_frame_filter(pts, words[:-1], lm, 0.0, True, True, -3.0, 30.0, 25.0)


def test_unmapped_ids_raise_only_where_the_reference_looks_them_up():
    from shine_mapping_amd.dataset import sem_frame_filter

    p, words, lut = _edge_cloud(2049, 5)
    lm = _Map(lut)
    pts = _layouts(p)["f32x4"]
    args = (2.5, True, True, -3.0, 30.0, 25.0)
    bad = words.copy()
    bad[11] = 177 | (5 << 16)  # unmapped and >= 100: filter_moving removes it first
    ok = sem_frame_filter(pts, bad, lm, *args)
    want = so.sem_filter(p.astype(np.float64), bad, lut, *args)
    assert np.array_equal(ok[1].cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="177"):  # without filter_moving it is looked up
        sem_frame_filter(pts, bad, lm, 2.5, False, True, -3.0, 30.0, 25.0)
    bad = words.copy()
    bad[9] = 77  # unmapped, but inside range_min: dropped before the lookup
    assert sem_frame_filter(pts, bad, lm, *args)[0].shape[0] == ok[0].shape[0]
    bad[5] = 77  # unmapped on a point outside the crop box: the reference raises before it crops
    with pytest.raises(ValueError, match="77"):
        sem_frame_filter(pts, bad, lm, *args)
    with pytest.raises(KeyError):
        so.sem_filter(p.astype(np.float64), bad, lut, *args)


# ---- voxel means with attributes ----------------------------------------------------------------------------------------------------
def _voxel_clouds():
    rng = np.random.default_rng(9)
    out = {}
    out["one voxel"] = (rng.uniform(0.0, 0.04, size=(300, 3)), 0.1)
    out["own voxels"] = (np.stack(np.meshgrid(np.arange(7.0), np.arange(7.0), np.arange(7.0), indexing="ij"), -1).reshape(-1, 3)
                         + rng.uniform(0.0, 0.3, size=(343, 3)), 1.0)
    for n in (255, 256, 257):
        out["n = %d" % n] = (rng.uniform(-2.0, 2.0, size=(n, 3)), 0.5)
    # ~5000 points, tens per voxel in shuffled input order: the sorted runs are tens long and straddle the 256-thread workgroups
    centres = rng.integers(-3, 3, size=(125, 3)).astype(np.float64)
    out["long runs"] = ((centres[rng.integers(0, 125, 5003)] + rng.uniform(0.05, 0.95, size=(5003, 3))), 1.0)
    return out


@pytest.mark.parametrize("n_attr", [1, 3])
def test_voxel_down_sample_with_attrs_equals_the_oracle_and_leaves_points_and_keys_alone(n_attr):
    from shine_mapping_amd import evaluation as ev

    rng = np.random.default_rng(n_attr)
    for name, (pts, voxel) in _voxel_clouds().items():
        n = len(pts)
        attrs = rng.integers(0, 21, size=(n, n_attr)).astype(np.float64) / 255.0
        dev = torch.from_numpy(pts).cuda()
        plain, keys0 = ev.voxel_down_sample(dev, voxel, return_keys=True)
        a_in = torch.from_numpy(attrs[:, 0] if n_attr == 1 else attrs).cuda()
        got_p, got_k, got_a = ev.voxel_down_sample(dev, voxel, return_keys=True, attrs=a_in)
        assert torch.equal(got_p, plain) and torch.equal(got_k, keys0)
        only_p, only_a = ev.voxel_down_sample(dev, voxel, attrs=a_in)
        assert torch.equal(only_p, plain) and torch.equal(only_a, got_a)
        want_p, want_k, want_a = so.voxel_attr(pts, attrs, voxel)
        print("%s: %d points -> %d voxels, %d attribute column(s)" % (name, n, len(want_k), n_attr))
        assert np.array_equal(got_k.cpu().numpy(), want_k)
        assert got_a.shape == ((len(want_k),) if n_attr == 1 else (len(want_k), n_attr)) and got_a.dtype == torch.float64
        assert np.array_equal(got_a.cpu().numpy().reshape(len(want_k), n_attr), want_a)
        assert np.allclose(got_p.cpu().numpy(), want_p, rtol=1e-12, atol=0)  # (as tests/test_gpu_dataset.py holds the point means)
        if name == "one voxel":
            assert len(want_k) == 1
        if name == "own voxels":
            assert len(want_k) == n


def test_voxel_class_of_3_and_4_is_4_and_the_size_query_is_the_plain_one():
    from shine_mapping_amd import _lib
    from shine_mapping_amd import evaluation as ev

    pts = np.array([[0.0, 0, 0], [0.1, 0, 0], [2.0, 0, 0], [2.1, 0, 0], [2.2, 0, 0], [4.0, 0, 0]])
    cls = np.array([3, 4, 2, 9, 9, 20])
    _, mean = ev.voxel_down_sample(torch.from_numpy(pts).cuda(), 1.0, attrs=torch.from_numpy(cls / 255.0).cuda())
    got = torch.round(mean * 255.0).to(torch.int32).cpu().numpy()
    assert float(mean[0] * 255.0) == 3.5 and got.tolist() == [4, 7, 20] == so.voxel_classes(pts, cls, 1.0)[2].tolist()
    e = ev.voxel_down_sample(torch.empty((0, 3), dtype=torch.float64, device="cuda"), 1.0, attrs=torch.empty((0, 3), device="cuda"))
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3)
    with pytest.raises(ValueError, match="attrs"):
        ev.voxel_down_sample(torch.from_numpy(pts).cuda(), 1.0, attrs=torch.zeros((6, 5), device="cuda"))
    lib = _lib.lib()
    a, b = C.c_size_t(0), C.c_size_t(0)
    assert lib.shine_eval_voxel_down(None, 5000, None, 0.1, None, C.byref(a), None, None, None, None) == 0
    assert lib.shine_voxel_down_attr(None, None, 3, 5000, None, 0.1, None, C.byref(b), None, None, None, None, None) == 0
    assert a.value == b.value > 4 * 8 * 5000


# ---- the dataset on a labelled drive --------------------------------------------------------------------------------------------------
FRAMES = 4


@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    from shine_mapping_amd import synth

    folder = str(tmp_path_factory.mktemp("sem_drive"))
    cfg = synth.make_config("ncd", device="cuda")
    return synth.write_kitti_drive(folder, cfg, frames=FRAMES, beams=16, azimuths=90, device="cpu", labels=True)


def _dataset(drive, with_octree=True, **over):
    from shine_mapping_amd import FeatureOctree, synth
    from shine_mapping_amd.dataset import LiDARDataset

    # (a crop radius inside the scan's range.  At vox_down_m = 0.05 this sparse scan keeps one point per voxel, so a voxel's class
    # is its point's; voxels that mix classes are the subject of the voxel tests above, and the map copy's 0.2 m voxels mix colours)
    cfg = synth.dataset_config("ncd", drive, **dict(dict(pc_radius=20.0, min_range=2.5, semantic_on=True), **over))
    torch.manual_seed(1)
    octree = FeatureOctree(cfg) if with_octree else None
    return cfg, octree, LiDARDataset(cfg, octree)


@pytest.fixture(scope="module")
def oracle(drive):
    """the oracle's frames of the default semantic configuration, computed once"""
    cfg, _, ds = _dataset(drive, with_octree=False)
    lm = ds.label_map
    frames = []
    for f in range(FRAMES):
        name = ds.pc_filenames[f]
        frames.append(so.frame(fo.read_kitti_bin(os.path.join(cfg.pc_path, name)),
                               so.read_labels(os.path.join(cfg.label_path, name.replace("bin", "label"))), ds.poses_ref[f], cfg,
                               lm.lut, lm.colors))
    return frames


def _want_pool(ds, oracle, frames):
    return np.concatenate([so.sample_labels(oracle[f]["classes"], ds.sampler.ns, ds.sampler.S) for f in frames])


def test_frame_stages_with_labels_equal_the_oracle(drive, oracle):
    from shine_mapping_amd.dataset import transform_points

    cfg, _, ds = _dataset(drive, with_octree=False)
    assert cfg.min_z < 0 and cfg.min_range > 0 and cfg.filter_moving_object  # the quirk: no range cut, the outlier filter on
    for f in range(FRAMES):
        name = ds.pc_filenames[f]
        words = so.read_labels(os.path.join(cfg.label_path, name.replace("bin", "label")))
        want = oracle[f]
        assert 0 < len(want["kept"]) < len(words) and len(np.unique(want["classes"])) >= 4
        pts, classes = ds.sem_frame_points(f)
        assert classes.dtype == torch.int32 and np.array_equal(classes.cpu().numpy(), want["classes"])
        assert pts.shape == want["sensor"].shape and np.allclose(pts.cpu().numpy(), want["sensor"], rtol=1e-12, atol=0)
        ds.process_frame(f)
        # the map copy: the oracle on the device's own transformed points (a pose product may round differently on the host)
        world = transform_points(pts, ds.poses_ref[f]).cpu().numpy()
        cur, _, colors = so.voxel_attr(world, ds.label_map.colors[want["classes"]], cfg.map_vox_down_m)
        assert ds.cur_frame_pc.points.shape == cur.shape and np.allclose(ds.cur_frame_pc.points.cpu().numpy(), cur, rtol=1e-12, atol=1e-12)
        assert np.array_equal(ds.cur_frame_pc.colors.cpu().numpy(), colors) and colors.min() >= 0 and colors.max() <= 1
        mixed = int(((colors * 255.0 != np.rint(colors * 255.0)).any(1)).sum())
        print("frame %d: %d labelled points, %d kept, %d voxels, %d map voxels (%d with a mixed colour)"
              % (f, len(words), len(want["kept"]), len(want["classes"]), len(cur), mixed))
    assert len(ds.map_down_pc) == sum(len(o["cur"]) for o in oracle) == ds.map_down_pc.colors.shape[0]
    mixed = sum(int((np.abs(o["class_means"] - np.rint(o["class_means"])) > 1e-9).sum()) for o in oracle)
    print("voxels that hold several classes: %d" % mixed)


def test_rand_downsample_applies_one_subset_to_points_and_classes(drive, oracle):
    cfg, _, ds = _dataset(drive, with_octree=False, rand_downsample=True, rand_down_r=0.37)
    raw = fo.read_kitti_bin(os.path.join(cfg.pc_path, ds.pc_filenames[1])).astype(np.float64)
    kept, kept_cls = oracle[1]["kept"], oracle[1]["kept_classes"]
    pts, classes = ds.sem_frame_points(1)
    assert pts.shape == (int(len(kept) * 0.37), 3) and classes.shape == (pts.shape[0],)
    row_class = {raw[i].tobytes(): int(c) for i, c in zip(kept, kept_cls)}
    assert [row_class[r.tobytes()] for r in pts.cpu().numpy()] == classes.tolist()


def test_sem_label_pool_in_batch_and_incremental_mode(drive, oracle):
    cfg, octree, ds = _dataset(drive)
    for f in range(FRAMES):
        ds.process_frame(f, incremental_on=False)
        want = _want_pool(ds, oracle, range(f + 1))
        assert ds.sem_label_pool.dtype == torch.int32 and ds.sem_label_pool.is_cuda
        assert np.array_equal(ds.sem_label_pool.cpu().numpy(), want) and len(ds) == len(want) == ds.coord_pool.shape[0]
    assert torch.equal(ds.sem_label_pool > 0, (ds.weight_pool > 0) & (ds.sem_label_pool > 0)) and int((ds.sem_label_pool > 0).sum()) > 0
    batch_coord, batch_sem = ds.coord_pool.clone(), ds.sem_label_pool.clone()
    cfg, octree, inc = _dataset(drive)
    at = 0
    for f in range(FRAMES):
        inc.process_frame(f, incremental_on=True)
        want = _want_pool(inc, oracle, [f])
        assert np.array_equal(inc.sem_label_pool.cpu().numpy(), want) and inc.sem_label_pool.dtype == torch.int32
        assert torch.equal(inc.coord_pool, batch_coord[at:at + len(want)])  # the same samples as batch mode's slice
        at += len(want)
    assert inc.normal_label_pool is None


def test_sem_label_pool_with_host_pools_and_with_window_replay(drive, oracle):
    cfg, octree, ds = _dataset(drive)
    for f in range(FRAMES):
        ds.process_frame(f)
    full = {r.tobytes(): int(c) for r, c in zip(ds.coord_pool.cpu().numpy(), ds.sem_label_pool.cpu().numpy())}
    assert len(full) == len(ds)  # (coordinates are distinct: a row names its sample)
    # host pools
    cfg, octree, host = _dataset(drive, pc_count_gpu_limit=1)
    assert host.to_cpu
    for f in range(FRAMES):
        host.process_frame(f)
    assert not host.sem_label_pool.is_cuda and host.sem_label_pool.dtype == torch.int32
    assert torch.equal(host.sem_label_pool, ds.sem_label_pool.cpu()) and torch.equal(host.coord_pool, ds.coord_pool.cpu())
    coord, sdf_label, origin, ts, normal_label, sem_label, weight = host.get_batch()
    assert sem_label.dtype == torch.int64 and sem_label.is_cuda and sem_label.shape == (cfg.bs,)
    assert all(full[r.tobytes()] == int(c) for r, c in zip(coord.cpu().numpy(), sem_label.cpu().numpy()))
    # incremental mode with host pools replaces them
    host.process_frame(0, incremental_on=True)
    assert np.array_equal(host.sem_label_pool.numpy(), _want_pool(host, oracle, [0])) and not host.coord_pool.is_cuda
    # window replay: the label rows kept are the coordinate rows kept
    cfg, octree, win = _dataset(drive, window_replay_on=True, window_radius=6.0)
    for f in range(FRAMES):
        win.process_frame(f)
    print("window replay: %d of %d samples kept" % (len(win), len(ds)))
    assert 0 < len(win) < len(ds) and win.sem_label_pool.shape[0] == win.coord_pool.shape[0] == win.time_pool.shape[0]
    assert torch.unique(win.time_pool).numel() >= 2
    assert [full[r.tobytes()] for r in win.coord_pool.cpu().numpy()] == win.sem_label_pool.tolist()
    last = _want_pool(win, oracle, [FRAMES - 1])
    assert np.array_equal(win.sem_label_pool[-len(last):].cpu().numpy(), last)


def test_the_other_pools_do_not_depend_on_semantic_on(drive):
    # min_range = 0 switches the outlier filter off (the quirk) and the plain path's range cut too; without filter_moving_object
    # both paths keep exactly the crop box
    over = dict(min_range=0.0, filter_moving_object=False)
    _, _, sem = _dataset(drive, **over)
    _, _, plain = _dataset(drive, semantic_on=False, **over)
    for f in range(FRAMES):
        sem.process_frame(f)
        plain.process_frame(f)
    assert plain.sem_label_pool is None and not plain.semantic and plain.map_down_pc.colors is None
    for name in ("coord", "sdf_label", "weight", "origin", "time", "sample_depth", "ray_depth"):
        assert torch.equal(getattr(sem, name + "_pool"), getattr(plain, name + "_pool")), name
    assert torch.equal(sem.map_down_pc.points, plain.map_down_pc.points)
    assert sem.sem_label_pool.shape[0] == sem.coord_pool.shape[0]


def _rows(*tensors):
    cols = [t.detach().double().cpu().reshape(t.shape[0], -1) for t in tensors]
    return np.ascontiguousarray(torch.cat(cols, 1).numpy())


def test_get_batch_returns_rows_of_the_pools_with_int64_labels(drive):
    cfg, octree, ds = _dataset(drive, bs=2048)
    for f in range(FRAMES):
        ds.process_frame(f)
    pool = {r.tobytes() for r in _rows(ds.coord_pool, ds.sdf_label_pool, ds.origin_pool, ds.time_pool, ds.sem_label_pool, ds.weight_pool)}
    for _ in range(2):  # through the sorted pool (the octree's node order)
        coord, sdf_label, origin, ts, normal_label, sem_label, weight = ds.get_batch()
        assert sem_label.dtype == torch.int64 and sem_label.shape == (cfg.bs,) and sem_label.is_cuda and normal_label is None
        batch = _rows(coord, sdf_label, origin, ts, sem_label, weight)
        assert all(r.tobytes() in pool for r in batch)
        assert int((sem_label > 0).sum()) > 0 and bool((sem_label[weight < 0] == 0).all())
    # without an octree: the plain draw
    cfg, _, flat = _dataset(drive, with_octree=False, bs=512)
    flat.process_frame(0)
    coord, sdf_label, origin, ts, _, sem_label, weight = flat.get_batch()
    pool0 = {r.tobytes() for r in _rows(flat.coord_pool, flat.sdf_label_pool, flat.sem_label_pool)}
    assert sem_label.dtype == torch.int64 and all(r.tobytes() in pool0 for r in _rows(coord, sdf_label, sem_label))


def test_ray_mode_gives_one_label_per_ray(drive, oracle):
    cfg, octree, ds = _dataset(drive, ray_loss=True, bs=64)
    for f in range(2):
        ds.process_frame(f)
    R = ds.ray_sample_count
    assert R == ds.sampler.S and np.array_equal(ds.sem_label_pool.cpu().numpy(), _want_pool(ds, oracle, range(2)))
    n_ray = ds.ray_depth_pool.shape[0]
    assert ds.sem_label_pool.shape[0] == n_ray * R
    torch.manual_seed(5)
    coord, sample_depth, ray_depth, normal_label, sem_label, weight = ds.get_batch()
    torch.manual_seed(5)
    ray_index = torch.randint(0, n_ray, (cfg.bs,), device="cuda")  # (get_batch's own draw)
    assert torch.equal(ray_depth, ds.ray_depth_pool[ray_index])
    classes = torch.from_numpy(np.concatenate([oracle[f]["classes"] for f in range(2)])).cuda()
    assert sem_label.dtype == torch.int64 and sem_label.shape == (cfg.bs,) and torch.equal(sem_label, classes[ray_index].long())


def test_write_merged_pc_round_trips_the_class_colours(drive, oracle, tmp_path):
    from shine_mapping_amd.evaluation import read_ply

    cfg, _, ds = _dataset(drive, with_octree=False)
    for f in range(FRAMES):
        ds.process_frame(f)
    ds.write_merged_pc(str(tmp_path / "merged.ply"))
    back = read_ply(str(tmp_path / "merged.ply"))
    colors = ds.map_down_pc.colors.cpu().numpy()
    assert back["vertices"].shape == (len(ds.map_down_pc), 3) and back["red"].dtype == np.uint8
    rgb = np.stack([back["red"], back["green"], back["blue"]], 1)
    assert np.array_equal(rgb, np.clip(np.rint(colors * 255.0), 0, 255).astype(np.uint8))
    # ... which are the oracle's: allclose here (its map voxels come from a host pose product), exact in the stage test above
    want = np.concatenate([o["cur_colors"] for o in oracle])
    assert want.shape == colors.shape and np.allclose(colors, want, rtol=0, atol=1e-12)
    assert len(np.unique(rgb, axis=0)) >= 4
    # a map without colours gives a cloud without colours
    _, _, plain = _dataset(drive, with_octree=False, semantic_on=False)
    plain.process_frame(0)
    plain.write_merged_pc(str(tmp_path / "plain.ply"))
    assert "red" not in read_ply(str(tmp_path / "plain.ply"))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_ingest_train_the_semantic_head_and_mesh_with_labels(drive, tmp_path, monkeypatch):
    import sys

    from shine_mapping_amd import Decoder, optim, sdf_bce_loss
    from shine_mapping_amd.mesher import Mesher, query_labels_device

    monkeypatch.setitem(sys.modules, "utils.semantic_kitti_utils", None)  # (the colours below are the config's, wherever this runs)
    cfg, octree, ds = _dataset(drive, bs=4096)
    for f in range(FRAMES):
        ds.process_frame(f)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio, cfg.weight_s = 0.01, 1e-15, True, 1.0, 1.0
    torch.manual_seed(3)
    geo, sem = Decoder(cfg).cuda(), Decoder(cfg, is_geo_encoder=False).cuda()
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), list(geo.parameters()), list(sem.parameters()), None)
    nll = []
    for it in range(100):  # shine_batch.py:119-209 with semantic_on, on get_batch's labels
        coord, sdf_label, origin, ts, _, sem_label, weight = ds.get_batch()
        feature = octree.query_feature(coord)
        loss = sdf_bce_loss(geo.sdf(feature), sdf_label, cfg.sigma_sigmoid, torch.abs(weight), False, "mean")
        sem_loss = torch.nn.NLLLoss(reduction="mean")(sem.sem_label_prob(feature), sem_label)
        opt.zero_grad(set_to_none=True)
        (loss + cfg.weight_s * sem_loss).backward()
        opt.step()
        nll.append(float(sem_loss.detach()))
    first, last = float(np.mean(nll[:10])), float(np.mean(nll[-10:]))
    print("semantic NLL: mean of the first 10 iterations %.4f, of the last 10 %.4f" % (first, last))
    assert np.isfinite(nll).all() and last < first
    surf = ds.sem_label_pool > 0
    pred = query_labels_device(octree, sem, ds.coord_pool[surf])
    print("surface samples whose predicted class matches: %.4f of %d" % (float((pred == ds.sem_label_pool[surf].long()).double().mean()),
                                                                         int(surf.sum())))
    cfg.min_cluster_vertices = 10
    m = Mesher(cfg, octree, geo, sem)
    top = octree.max_level - octree.featured_level_num + 1
    mesh = m.recon_octree_mesh(top, 0.2, str(tmp_path / "sem.ply"), None, estimate_sem=True, estimate_normal=False,
                               filter_isolated_mesh=False)
    labels, colors = np.asarray(mesh.vertex_labels), np.asarray(mesh.vertex_colors)
    print("mesh: %d vertices, %d triangles, classes %s" % (len(labels), len(np.asarray(mesh.triangles)), np.unique(labels).tolist()))
    assert len(labels) > 0 and len(np.asarray(mesh.triangles)) > 0 and bool((labels > 0).all())
    table = np.zeros((cfg.sem_class_count + 1, 3))
    for k, c in cfg.sem_color_map.items():
        table[k] = np.asarray(c, np.float64) / 255.0
    assert np.array_equal(colors, table[labels])
