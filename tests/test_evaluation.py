"""CPU: the evaluation module's host side (PLY reader, argument handling, the metrics dict, the CLI) and self-checks of the
numpy oracle (tests/eval_oracle.py) that the GPU tests compare the device with."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_oracle as eo
from conftest import ROOT
from shine_mapping_amd import evaluation as ev
from shine_mapping_amd.mesher import write_ply

ELEVEN = ["MAE_accuracy (m)", "MAE_completeness (m)", "Chamfer_L1 (m)", "Chamfer_L2 (m)", "Precision [Accuracy] (%)",
          "Recall [Completeness] (%)", "F-score (%)", "Spacing (m)", "Inlier_threshold (m)", "Outlier_truncation_acc (m)",
          "Outlier_truncation_com (m)"]


# ------------------------------------------------------------------------------------------------ read_ply
def test_read_ply_round_trips_a_mesh_with_normals_and_colours(tmp_path):
    rng = np.random.default_rng(1)
    v = rng.normal(size=(50, 3)) * 100.0
    nrm = rng.normal(size=(50, 3))
    rgb = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    f = rng.integers(0, 50, size=(80, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    write_ply(p, [("x", v[:, 0], "double"), ("y", v[:, 1], "double"), ("z", v[:, 2], "double"),
                  ("nx", nrm[:, 0], "double"), ("ny", nrm[:, 1], "double"), ("nz", nrm[:, 2], "double"),
                  ("red", rgb[:, 0], "uchar"), ("green", rgb[:, 1], "uchar"), ("blue", rgb[:, 2], "uchar")], f)
    d = ev.read_ply(p)
    assert d["vertices"].dtype == np.float64 and np.array_equal(d["vertices"], v)
    assert d["faces"].dtype == np.int32 and np.array_equal(d["faces"], f)
    assert np.array_equal(np.stack([d["nx"], d["ny"], d["nz"]], 1), nrm)
    assert np.array_equal(np.stack([d["red"], d["green"], d["blue"]], 1), rgb)


def test_read_ply_round_trips_a_cloud_float_vertices_and_zero_vertices(tmp_path):
    rng = np.random.default_rng(2)
    v = rng.normal(size=(33, 3))
    p = str(tmp_path / "c.ply")
    write_ply(p, [("x", v[:, 0], "double"), ("y", v[:, 1], "double"), ("z", v[:, 2], "double")])
    d = ev.read_ply(p)
    assert d["faces"] is None and np.array_equal(d["vertices"], v)
    write_ply(p, [("x", v[:, 0], "float"), ("y", v[:, 1], "float"), ("z", v[:, 2], "float"), ("label", np.arange(33), "int")])
    d = ev.read_ply(p)
    assert np.array_equal(d["vertices"], v.astype(np.float32).astype(np.float64)) and np.array_equal(d["label"], np.arange(33))
    z = np.zeros(0)
    write_ply(p, [("x", z, "double"), ("y", z, "double"), ("z", z, "double")], np.zeros((0, 3), np.int32))
    d = ev.read_ply(p)
    assert d["vertices"].shape == (0, 3) and d["faces"].shape == (0, 3)
    write_ply(p, [("x", z, "double"), ("y", z, "double"), ("z", z, "double")])
    d = ev.read_ply(p)
    assert d["vertices"].shape == (0, 3) and d["faces"] is None


def test_read_ply_parses_a_hand_written_ascii_file(tmp_path):
    p = tmp_path / "a.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nelement face 2\nproperty list uchar uint vertex_indices\nend_header\n"
                 "0 0 0 255\n1 0 0 0\n0 1.5 0 7\n0 0 -2e1 9\n3 0 1 2\n3 0 2 3\n")
    d = ev.read_ply(str(p))
    assert np.array_equal(d["vertices"], np.array([[0, 0, 0], [1, 0, 0], [0, 1.5, 0], [0, 0, -20.0]]))
    assert np.array_equal(d["faces"], np.array([[0, 1, 2], [0, 2, 3]], np.int32)) and d["faces"].dtype == np.int32
    assert np.array_equal(d["red"], np.array([255, 0, 7, 9], np.uint8))
    with pytest.raises(ValueError):
        q = tmp_path / "b.ply"
        q.write_text("not a ply\n")
        ev.read_ply(str(q))


# ------------------------------------------------------------------------------------------------ arguments, dict, CLI
def test_metric_dict_has_the_eleven_keys_in_order_and_nan_rules():
    assert ev.METRIC_KEYS == ELEVEN and eo.METRIC_KEYS == ELEVEN
    m = ev.metrics_from_sums([3.0, 5.0, 2.0, 8.0, 20.0, 1.0, 4.0, 4.0], 0.02, 0.05, 0.2, 2.0)
    assert list(m) == ELEVEN
    assert m["MAE_accuracy (m)"] == 0.75 and m["MAE_completeness (m)"] == 2.0 and m["Chamfer_L1 (m)"] == 1.375
    assert m["Chamfer_L2 (m)"] == np.sqrt(0.5 * (1.25 + 5.0))
    assert m["Precision [Accuracy] (%)"] == 50.0 and m["Recall [Completeness] (%)"] == 25.0
    assert m["F-score (%)"] == 2 * 50.0 * 25.0 / 75.0
    assert [m[k] for k in ELEVEN[7:]] == [0.02, 0.05, 0.2, 2.0]
    # empty arrays: NaN where numpy's mean of nothing is NaN, no exception; F-score NaN when precision + recall is 0
    e = ev.metrics_from_sums([0, 0, 0, 0, 0, 0, 0, 0], 0.02, 0.05, 0.2, 2.0)
    o = eo.metrics(np.zeros(0), np.zeros(0), 0.02, 0.05, 0.2, 2.0)
    assert list(o) == ELEVEN
    for k in ELEVEN[:7]:
        assert np.isnan(e[k]) and np.isnan(o[k])
    z = ev.metrics_from_sums([1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 2.0, 2.0], 0.02, 0.05, 0.2, 2.0)
    assert z["Precision [Accuracy] (%)"] == 0.0 and z["Recall [Completeness] (%)"] == 0.0 and np.isnan(z["F-score (%)"])
    assert np.isnan(eo.metrics(np.ones(2), np.ones(2), 0.02, 0.05, 0.2, 2.0)["F-score (%)"])
    # the oracle's dict and the module's agree on ordinary numbers
    dp, dr = np.array([0.01, 0.04, 0.3]), np.array([0.02, 0.06])
    sums = [dp.sum(), (dp ** 2).sum(), 2, dr.sum(), (dr ** 2).sum(), 1, 3, 2]
    a, b = ev.metrics_from_sums(sums, 0.02, 0.05, 0.2, 2.0), eo.metrics(dp, dr, 0.02, 0.05, 0.2, 2.0)
    for k in ELEVEN:
        assert a[k] == pytest.approx(b[k], rel=1e-15)


def test_voxel_down_sample_refuses_more_than_21_bit_indices():
    pts = np.array([[0.0, 0.0, 0.0], [0.0, 30000.0, 0.0]])
    with pytest.raises(ValueError, match="21-bit"):
        ev.voxel_down_sample(pts, 0.01)  # 3 * 10^6 voxels along y > 2^21
    with pytest.raises(ValueError):
        ev.voxel_down_sample(pts, 0.0)


def test_argument_errors_need_no_gpu():
    from shine_mapping_amd import _lib
    import ctypes as C

    lib = _lib.lib()
    assert lib.shine_eval_fine_per_coarse() == ev.FINE_PER_COARSE
    need = C.c_size_t(0)
    assert lib.shine_eval_bounds(None, 1 << 31, None, C.byref(need), None, None) == -1
    assert lib.shine_eval_metrics(None, 10, None, 10, 0.05, None, C.byref(need), None, None) == 0 and need.value > 0
    assert lib.shine_eval_grid_count(None, 0, None, 0.1, None, C.byref(need), None, None) == -1
    assert lib.shine_eval_grid_emit(None, 10, None, 0, 20, 1, None, C.byref(need), None) == -1  # more fine cells than points
    assert lib.shine_eval_grid_emit(None, 10, None, 0, 5, 2, None, C.byref(need), None) == 0 and need.value >= 10 * 28
    with pytest.raises(ValueError):
        ev._load_mesh(os.path.join(ROOT, "README.md"))
    with pytest.raises(TypeError):
        ev._load_mesh(3)


def test_cli_help_runs_in_a_child_process():
    r = subprocess.run([sys.executable, "-m", "shine_mapping_amd.evaluation", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--spacing", "--threshold", "--trunc-acc", "--trunc-com", "--no-bbx-mask", "--samples", "--seed", "--csv"):
        assert flag in r.stdout


def test_csv_has_the_evaluators_columns(tmp_path):
    m = ev.metrics_from_sums([3.0, 5.0, 2.0, 8.0, 20.0, 1.0, 4.0, 4.0], 0.02, 0.05, 0.2, 2.0)
    p = str(tmp_path / "e.csv")
    ev.write_csv(p, m)
    lines = open(p).read().splitlines()
    assert lines[0] == ",".join(ELEVEN) and len(lines) == 2 and lines[1].split(",")[0] == "0.75"


def test_package_exports_eval_mesh():
    import shine_mapping_amd

    assert shine_mapping_amd.eval_mesh is ev.eval_mesh and "eval_mesh" in shine_mapping_amd.__all__


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_brute_force_equals_the_tree():
    if not eo.have_scipy():
        pytest.skip("scipy does not import: nothing to compare the brute force with")
    rng = np.random.default_rng(5)
    ref = rng.normal(size=(20000, 3)) + np.array([50.0, -20.0, 3.0])
    qry = rng.normal(size=(5000, 3)) + np.array([50.0, -20.0, 3.0])
    ib, db, sb = eo.nn_brute(ref, qry, second=True)
    it, dt, st = eo.nn_tree(ref, qry, second=True)
    assert np.array_equal(db, dt)
    tie = db == sb
    assert np.array_equal(ib[~tie], it[~tie])
    assert np.allclose(sb, st, rtol=1e-14, atol=0)


def test_oracle_crop_sample_and_voxel_rules():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 2, 2]])
    f = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4]])
    cv, cf = eo.crop_mesh(v, f, [0, 0, 0], [1, 1, 0])  # points on the bounds are kept
    assert np.array_equal(cv, v[:4]) and np.array_equal(cf, f[:2])
    # a zero-area triangle between two unit-area halves is never chosen; u0 = 0.5 falls to the triangle after it
    v2 = np.array([[0.0, 0, 0], [2, 0, 0], [0, 1, 0], [5, 5, 5], [0, 0, 1]])
    f2 = np.array([[0, 1, 2], [3, 3, 3], [0, 1, 4]])
    u = np.array([[0.0, 0.25, 0.5], [0.49, 0.0, 0.0], [0.5, 1.0 - 2 ** -53, 0.0], [0.99, 0.25, 1.0 - 2 ** -53]])
    pts, tri, cdf = eo.sample_points(v2, f2, u)
    assert tri.tolist() == [0, 0, 2, 2] and cdf.tolist() == [0.5, 0.5, 1.0]
    assert np.allclose(pts[1], v2[0]) and np.allclose(pts[0], 0.5 * v2[0] + 0.25 * v2[1] + 0.25 * v2[2])
    # voxel means: the grid starts half a voxel below the minimum, keys ascend
    p = np.array([[0.0, 0, 0], [0.4, 0, 0], [0.6, 0, 0], [-0.0, 0.9, 0], [0.1, 0.1, 0.1]])
    m, k = eo.voxel_down_sample(p, 1.0)
    assert k.tolist() == [0, 1 << 21, 1 << 42]
    assert np.allclose(m, [[0.5 / 3, 0.1 / 3, 0.1 / 3], [0, 0.9, 0], [0.6, 0, 0]])


def test_oracle_on_concentric_spheres_stays_inside_the_derived_band():
    """Two Fibonacci spheres of radii 1.00 and 1.03 m, 2 * 10^6 points each (dense against the voxel), down-sampled at s = 0.02:
    every nearest-neighbour distance, both ways, lies in [0.03 - 3 s^2 / (8 r), 0.03 + 3 s^2 / (8 r) + sqrt(3) s] — a voxel mean
    sits at most the sagitta of a voxel-diagonal chord inside its sphere, and the radial projection of any point falls in an
    occupied voxel whose mean is within one diagonal of it."""
    s, r = 0.02, 1.0
    centre = np.array([50.0, -20.0, 3.0])
    a = eo.voxel_down_sample(eo.fibonacci_sphere(2000000, 1.00, centre), s)[0]
    b = eo.voxel_down_sample(eo.fibonacci_sphere(2000000, 1.03, centre), s)[0]
    lo, hi = 0.03 - 3 * s * s / (8 * r), 0.03 + 3 * s * s / (8 * r) + np.sqrt(3.0) * s
    rng = np.random.default_rng(11)
    for ref, qry in ((a, b), (b, a)):
        if eo.have_scipy():
            d = eo.nn_tree(ref, qry)[1]
        else:
            d = eo.nn_brute(ref, qry[rng.choice(len(qry), 4096, replace=False)])[1]
        print("nn distances %.6f .. %.6f (band %.6f .. %.6f), %d queries" % (d.min(), d.max(), lo, hi, len(d)))
        assert lo <= d.min() and d.max() <= hi
