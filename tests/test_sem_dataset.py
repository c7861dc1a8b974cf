"""CPU suite of the semantic frame front-end: the numpy oracle (tests/sem_frame_oracle.py) against the reference's own
preprocess_sem_kitti (tests/golden/sem_frame.pt, written by tools/make_sem_frame_golden.py), semantic_kitti.LabelMap, the host logic
of LiDARDataset with semantic_on (refusal rule, file checks), the labelled synthetic drive, and the argument checks of
shine_sem_frame_filter / shine_voxel_down_attr.  Nothing here needs a GPU; the device stages are in tests/test_gpu_sem_dataset.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sem_frame_oracle as so
from conftest import load_golden
from test_dataset import make_cfg


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_the_reference_preprocess_exactly():
    fx = load_golden("sem_frame")
    lut = fx["lut"].numpy()
    assert lut.shape == (65536,) and lut.dtype == np.int32 and lut[40] == 9 and lut[252] == 1 and lut[2] == -1
    assert fx["colors"].shape == (21, 3) and float(fx["colors"].max()) == 1.0
    seen = set()
    for case in fx["cases"]:
        p = case["points"].double().numpy()
        words = case["labels"].numpy().view(np.uint32)
        assert int((words >> 16).max()) > 0 or len(words) == 1  # (instance ids in the upper half)
        idx, cls = so.sem_filter(p, words, lut, case["min_range"], case["filter_moving"], case["filter_outlier"])
        assert np.array_equal(p[idx], case["points_out"].double().numpy())
        assert np.array_equal(cls, case["classes"].numpy()) and cls.dtype == np.int32
        seen.add((case["filter_moving"], case["filter_outlier"]))
        if len(p) > 8:
            assert 0 < len(idx) < len(p)
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    sizes = sorted({int(c["points"].shape[0]) for c in fx["cases"]})
    assert all(n in sizes for n in (1, 2047, 2048, 2049, 3 * 2048 + 5))


def test_oracle_edges_crop_faces_range_and_label_thresholds():
    lut = np.full(65536, -1, np.int32)
    lut[[0, 1, 40, 99, 100]] = [0, 0, 2, 7, 5]
    R, min_z, max_z, rmin = 25.0, -3.0, 30.0, 2.5
    pts = np.array([[25.0, 0, 0], [-25.0, 25.0, 1.0], [3.0, 4.0, 30.0], [5.0, 5.0, -3.0], [25.000001, 0, 0], [0, 0, 30.5],
                    [1.5, 2.0, 0.0], [2.4999, 0, 0], [9.0, 0, 0], [9.0, 1, 0], [9.0, 2, 0], [9.0, 3, 0]])
    ids = np.array([40, 40, 40, 40, 40, 40, 40, 40, 99, 100, 1, 0], np.uint32) | np.uint32(7 << 16)
    idx, cls = so.sem_filter(pts, ids, lut, rmin, True, True, min_z, max_z, R)
    # faces kept (z == min_z too: the semantic path has no strict z test), outside dropped, r == range_min kept, 99 kept, 100 / 1 dropped
    assert idx.tolist() == [0, 1, 2, 3, 6, 8, 11] and cls.tolist() == [2, 2, 2, 2, 2, 7, 0]
    idx, cls = so.sem_filter(pts, ids, lut, rmin, False, False, min_z, max_z, R)
    assert idx.tolist() == [0, 1, 2, 3, 6, 8, 9, 10, 11] and cls.tolist() == [2, 2, 2, 2, 2, 7, 5, 0, 0]
    bad = ids.copy()
    bad[9] = 177  # unmapped and moving: removed by filter_moving before the lookup ...
    assert len(so.sem_filter(pts, bad, lut, rmin, True, True, min_z, max_z, R)[0]) == 7
    with pytest.raises(KeyError):  # ... and looked up without it, even though it is outside nothing
        so.sem_filter(pts, bad, lut, rmin, False, True, min_z, max_z, R)
    bad[9], bad[4] = 100, 77  # unmapped on a point the CROP would drop: the reference looks it up before it crops
    with pytest.raises(KeyError):
        so.sem_filter(pts, bad, lut, rmin, True, True, min_z, max_z, R)


def test_oracle_voxel_classes_round_the_mean_half_to_even():
    pts = np.array([[0.0, 0, 0], [0.1, 0, 0], [2.0, 0, 0], [2.1, 0, 0], [2.2, 0, 0], [4.0, 0, 0]])
    means, keys, cls = so.voxel_classes(pts, [3, 4, 2, 9, 9, 20], 1.0)
    assert ((3 / 255.0 + 4 / 255.0) / 2) * 255.0 == 3.5  # (the tie is exact in fp64)
    assert cls.tolist() == [4, 7, 20] and len(keys) == 3 and np.allclose(means[:, 0], [0.05, 2.1, 4.0])
    m2, k2, a2 = so.voxel_attr(pts, np.arange(18.0).reshape(6, 3), 1.0)
    assert np.array_equal(m2, means) and np.array_equal(a2[0], [1.5, 2.5, 3.5]) and np.array_equal(a2[2], [15.0, 16.0, 17.0])
    assert so.sample_labels([5, 0, 2], 2, 5).tolist() == [5, 5, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 0, 0, 0]


# ---- LabelMap ------------------------------------------------------------------------------------------------------------------------
def test_label_map_from_dicts_and_from_a_yaml_with_bgr_colours(tmp_path):
    from types import SimpleNamespace

    from shine_mapping_amd.semantic_kitti import LabelMap

    cfg = SimpleNamespace(sem_class_count=20, sem_label_map={0: 0, 40: 9, 252: 1}, sem_color_map={9: (255, 0, 255), 1: (100, 150, 245)})
    m = LabelMap.from_config(cfg)
    assert m.n_class == 21 and m.lut.dtype == np.int32 and m.lut.shape == (65536,)
    assert m.lut[40] == 9 and m.lut[252] == 1 and m.lut[0] == 0 and m.lut[41] == -1 and int((m.lut >= 0).sum()) == 3
    assert m.colors.shape == (21, 3) and m.colors.dtype == np.float64
    assert np.array_equal(m.colors[1], np.array([100, 150, 245]) / 255.0) and np.array_equal(m.colors[2], [0, 0, 0])
    assert LabelMap.from_config(SimpleNamespace(sem_class_count=20, sem_label_map={40: 9})).colors is None
    path = tmp_path / "labels.yaml"
    path.write_text("labels:\n  0: unlabeled\n  40: road\n  10: car\n"
                    "color_map: # bgr\n  0: [0, 0, 0]\n  10: [245, 150, 100]\n  40: [255, 0, 255]\n  44: [255, 150, 255]\n"
                    "learning_map:\n  0: 0\n  10: 1\n  40: 2\n  44: 2\n  252: 1\n"
                    "learning_map_inv:\n  0: 0\n  1: 10\n  2: 40\n")
    y = LabelMap.from_config(SimpleNamespace(sem_class_count=2, label_map_path=str(path)))
    assert y.n_class == 3 and y.lut[44] == 2 and y.lut[252] == 1 and y.lut[41] == -1
    assert np.allclose(y.colors * 255.0, [[0, 0, 0], [100, 150, 245], [255, 0, 255]], rtol=0, atol=1e-12)  # (BGR in the file, RGB here)
    # the dict wins over the yaml
    both = LabelMap.from_config(SimpleNamespace(sem_class_count=2, label_map_path=str(path), sem_label_map={7: 1}))
    assert both.lut[7] == 1 and both.lut[40] == -1


def test_label_map_errors_name_the_sources_and_the_class_range(tmp_path, monkeypatch):
    import sys
    from types import SimpleNamespace

    from shine_mapping_amd.semantic_kitti import LabelMap

    monkeypatch.setitem(sys.modules, "utils.semantic_kitti_utils", None)  # (the import fails, whatever else is on the path)
    with pytest.raises(ValueError) as e:
        LabelMap.from_config(SimpleNamespace(sem_class_count=20))
    for word in ("sem_label_map", "label_map_path", "utils.semantic_kitti_utils"):
        assert word in str(e.value)
    with pytest.raises(ValueError, match="sem_class_count"):
        LabelMap.from_config(SimpleNamespace(sem_class_count=20, sem_label_map={40: 21}))
    with pytest.raises(ValueError, match="sem_class_count"):
        LabelMap.from_config(SimpleNamespace(sem_class_count=20, sem_label_map={40: -1}))
    assert LabelMap.from_config(SimpleNamespace(sem_class_count=20, sem_label_map={40: 20})).lut[40] == 20  # (inclusive)
    path = tmp_path / "bad.yaml"
    path.write_text("learning_map:\n  40: 3\n")
    with pytest.raises(ValueError, match="sem_class_count"):
        LabelMap.from_config(SimpleNamespace(sem_class_count=2, label_map_path=str(path)))


def test_mesher_colour_map_falls_back_to_the_config(monkeypatch):
    import sys
    from types import SimpleNamespace

    from shine_mapping_amd.mesher import _sem_color_map

    monkeypatch.setitem(sys.modules, "utils.semantic_kitti_utils", None)
    assert _sem_color_map(SimpleNamespace()) is None and _sem_color_map() is None
    assert _sem_color_map(SimpleNamespace(sem_color_map={1: (1, 2, 3)})) == {1: (1, 2, 3)}


# ---- LiDARDataset's host logic ------------------------------------------------------------------------------------------------------
def _sem_cfg(tmp_path, **over):
    labels = tmp_path / "labels"
    labels.mkdir(exist_ok=True)
    return make_cfg(tmp_path, **dict(dict(semantic_on=True, label_path=str(labels), sem_class_count=20,
                                          sem_label_map={0: 0, 40: 9}, filter_moving_object=True), **over))


def test_semantic_on_needs_a_label_path(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset

    for path in (None, "", 5):
        with pytest.raises(NotImplementedError, match="semantic_on"):
            LiDARDataset(_sem_cfg(tmp_path, label_path=path))
    cfg = _sem_cfg(tmp_path)
    del cfg.label_path
    with pytest.raises(NotImplementedError, match="semantic_on"):
        LiDARDataset(cfg)
    ds = LiDARDataset(_sem_cfg(tmp_path))
    assert ds.semantic and ds.label_map.lut[40] == 9
    assert ds.sem_label_pool.dtype == torch.int32 and ds.sem_label_pool.shape == (0,)
    assert ds._kept_pools() == ("coord", "weight", "sdf_label", "origin", "time", "sem_label")
    off = LiDARDataset(_sem_cfg(tmp_path, semantic_on=False))
    assert not off.semantic and off.label_map is None and "sem_label" not in off._pools
    with pytest.raises(ValueError, match="sem_label_map"):  # semantic, but no label definition anywhere
        LiDARDataset(_sem_cfg(tmp_path, sem_label_map=None))


def test_semantic_mode_reads_bin_only_and_checks_the_label_count(tmp_path):
    from shine_mapping_amd.dataset import LiDARDataset

    ds = LiDARDataset(_sem_cfg(tmp_path))
    with pytest.raises(ValueError, match="bin"):
        ds.read_semantic_point_label(str(tmp_path / "scan.ply"), str(tmp_path / "labels" / "scan.label"))
    scan, lab = tmp_path / "velodyne" / "0.bin", tmp_path / "labels" / "0.label"
    np.zeros((5, 4), np.float32).tofile(str(scan))
    np.zeros(4, np.uint32).tofile(str(lab))
    with pytest.raises(ValueError, match="0.label") as e:
        ds.read_semantic_point_label(str(scan), str(lab))
    assert "4 labels" in str(e.value) and "5 points" in str(e.value)
    with pytest.raises(ValueError, match="label"):
        ds.read_semantic_point_label(str(scan), str(tmp_path / "labels" / "0.txt"))
    scan.write_bytes(b"")


# ---- the labelled drive ----------------------------------------------------------------------------------------------------------------
def test_labelled_drive_writes_one_uint32_per_point_with_instance_bits(tmp_path):
    import hashlib

    from shine_mapping_amd import synth

    cfg = synth.make_config("ncd", device="cuda")
    plain = synth.write_kitti_drive(str(tmp_path / "a"), cfg, frames=3, beams=8, azimuths=60, device="cpu")
    drive = synth.write_kitti_drive(str(tmp_path / "b"), cfg, frames=3, beams=8, azimuths=60, device="cpu", labels=True)
    assert not hasattr(plain, "label_path") and not os.path.exists(str(tmp_path / "a" / "labels"))
    assert sorted(os.listdir(drive.label_path)) == ["000000.label", "000001.label", "000002.label"]
    known = set(drive.label_map)
    ids_seen = set()
    for f in range(3):
        a, b = (open(os.path.join(d.pc_path, "%06d.bin" % f), "rb").read() for d in (plain, drive))
        assert hashlib.sha256(a).digest() == hashlib.sha256(b).digest()  # the scans do not depend on `labels`
        words = so.read_labels(os.path.join(drive.label_path, "%06d.label" % f))
        assert words.dtype == np.uint32 and len(words) == len(b) // 16
        assert int((words >> 16).min()) >= 1  # every point carries an instance id
        ids_seen |= set((words & 0xFFFF).tolist())
    assert ids_seen <= known and {40, 50, 10} <= ids_seen and 1 in ids_seen and any(i >= 100 for i in ids_seen)
    assert synth.DRIVE_UNMAPPED_ID not in known
    assert open(plain.pose_path).read() == open(drive.pose_path).read()
    odd = synth.write_kitti_drive(str(tmp_path / "c"), cfg, frames=1, beams=8, azimuths=60, device="cpu", labels=True, unmapped=3)
    words = so.read_labels(os.path.join(odd.label_path, "000000.label"))
    assert int(((words & 0xFFFF) == synth.DRIVE_UNMAPPED_ID).sum()) == 3
    c = synth.dataset_config("ncd", drive, semantic_on=True)
    assert c.label_path == drive.label_path and c.sem_label_map == drive.label_map and c.sem_color_map == drive.color_map
    assert max(c.sem_label_map.values()) <= c.sem_class_count and not hasattr(synth.dataset_config("ncd", plain), "label_path")


# ---- the C ABI's argument checks (no device is touched) ------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    INVALID = -1
    host = (C.c_char * 4096)()  # stands in for device memory: every call below returns before anything would touch it
    p = C.cast(host, C.c_void_p)
    need, big, small = C.c_size_t(0), C.c_size_t(1 << 30), C.c_size_t(8)
    kept, unknown = C.c_int64(-7), C.c_int64(-7)

    def sem(points, n, stride, labels, lut, ws, ws_bytes, out, cls, n_out, n_unknown, radius=25.0):
        return lib.shine_sem_frame_filter(points, n, 0, stride, labels, lut, 2.5, 1, 1, -3.0, 30.0, radius, ws, ws_bytes, out, cls,
                                          n_out, n_unknown, None)

    assert sem(None, 1000, 4, None, None, None, C.byref(need), None, None, None, None) == 0
    assert need.value >= 256 + 8  # the chain's head and one state word
    one_tile = need.value
    assert sem(None, 2049, 4, None, None, None, C.byref(need), None, None, None, None) == 0 and need.value >= one_tile
    assert sem(None, 1000, 4, None, None, None, None, None, None, None, None) == INVALID
    assert b"shine_sem_frame_filter" in lib.shine_error_string(INVALID)
    assert sem(None, 1 << 31, 4, None, None, None, C.byref(need), None, None, None, None) == INVALID
    assert sem(None, -1, 4, None, None, None, C.byref(need), None, None, None, None) == INVALID
    assert sem(None, 1000, 5, None, None, None, C.byref(need), None, None, None, None) == INVALID
    full = (p, 1000, 4, p, p, p, C.byref(big), p, p, C.byref(kept), C.byref(unknown))
    for at in (0, 3, 4, 7, 8, 9, 10):  # null points / labels / lut / points_out / class_out / n_out / n_unknown_out
        args = list(full)
        args[at] = None
        assert sem(*args) == INVALID, at
    assert sem(*full[:6], C.byref(small), *full[7:]) == INVALID
    assert sem(*full, radius=-1.0) == INVALID
    assert sem(None, 0, 4, None, None, p, C.byref(big), None, None, C.byref(kept), C.byref(unknown)) == 0
    assert (kept.value, unknown.value) == (0, 0)

    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)

    def vox(points, attrs, n_attr, n, origin, ws, ws_bytes, out, aout, n_out, voxel=0.1):
        return lib.shine_voxel_down_attr(points, attrs, n_attr, n, origin, voxel, ws, ws_bytes, out, aout, None, n_out, None)

    # the size query asks rocPRIM for its scratch, which asks for the device's architecture: host arithmetic for
    # shine_sem_frame_filter above, but here it answers what shine_eval_voxel_down's query answers on this machine (0 and the same
    # size with a GPU, the same HIP error without one; tests/test_gpu_sem_dataset.py checks the size on the device)
    plain, need = C.c_size_t(0), C.c_size_t(0)
    rc = lib.shine_eval_voxel_down(None, 1000, None, 0.1, None, C.byref(plain), None, None, None, None)
    assert vox(None, None, 3, 1000, None, None, C.byref(need), None, None, None) == rc and need.value == plain.value
    assert rc != INVALID and (rc != 0 or need.value > 4 * 8 * 1000)
    assert vox(None, None, 3, 1000, None, None, None, None, None, None) == INVALID
    assert b"shine_voxel_down_attr" in lib.shine_error_string(INVALID)
    for bad in (0, 5, -1):
        assert vox(None, None, bad, 1000, None, None, C.byref(need), None, None, None) == INVALID
    assert vox(None, None, 1, 1 << 31, None, None, C.byref(need), None, None, None) == INVALID
    assert vox(p, p, 1, 1000, o3, p, C.byref(big), p, p, None) == INVALID
    assert vox(p, p, 1, 1000, o3, p, C.byref(big), p, p, C.byref(kept), voxel=0.0) == INVALID
    assert vox(p, None, 1, 1000, o3, p, C.byref(big), p, p, C.byref(kept)) == INVALID
    assert vox(p, p, 1, 1000, o3, p, C.byref(big), p, None, C.byref(kept)) == INVALID
