"""GPU: every stage of shine_mapping_amd.evaluation against the numpy oracle (tests/eval_oracle.py).

Exactness: distances, means and Chamfer values at rtol 1e-9 (d^2 = dx^2 + dy^2 + dz^2 in fp64 with or without FMA contraction
carries <= ~4 ulp, sqrt one more, a mean over n <= 2 * 10^6 non-negative terms in any order <= n * 2^-53 ~ 2e-10); counts
(precision, recall, kept / dropped) must be EQUAL, which is fair because every test first asserts on the ORACLE's distances that
none lies within 1e-9 * max(1, value) of the threshold or of a truncation.  Nearest indices must be equal wherever the oracle's
best and second-best distances differ by more than 1e-9 relative; the share excused by that clause is asserted < 0.1 %."""
import math
import os
import time

import numpy as np
import pytest
import torch

import eval_oracle as eo
from shine_mapping_amd import evaluation as ev
from shine_mapping_amd import mesher
from shine_mapping_amd.mesher import write_ply

pytestmark = pytest.mark.gpu

CENTRES = [(50.0, -20.0, 3.0), (1500.0, -900.0, 40.0)]
RTOL = 1e-9


def noisy_sphere(n, radius, centre, sigma, seed):
    rng = np.random.default_rng(seed)
    return eo.fibonacci_sphere(n, radius, centre) + rng.normal(scale=sigma, size=(n, 3))


def assert_clear_of(dist, *values):
    """the guard: no oracle distance within 1e-9 * max(1, value) of a threshold / truncation (it may exclude ZERO cases)"""
    for v in values:
        gap = np.abs(np.asarray(dist) - v).min() if len(dist) else np.inf
        print("closest approach of a distance to %g: %.3e" % (v, gap))
        assert gap > 1e-9 * max(1.0, v)


def check_nn(res_index, res_dist, res_keep, ref, qry, truncation, oracle):
    """device per-query results against the oracle's (index, distance, second-best distance)"""
    oi, od, o2 = oracle
    d2 = ((qry - ref[oi]) ** 2).sum(-1)
    assert_clear_of(np.sqrt(d2), truncation)
    keep = d2 < truncation ** 2
    gi, gd, gk = res_index.cpu().numpy(), res_dist.cpu().numpy(), res_keep.cpu().numpy()
    assert np.array_equal(gk, keep)
    assert np.allclose(gd[keep], np.sqrt(d2[keep]), rtol=RTOL, atol=0)
    assert np.all(gd[~keep] == truncation) and np.all(gi[~keep] == -1)
    decided = keep & (o2 - od > RTOL * od)
    excused = keep & ~decided
    share = excused.sum() / max(int(keep.sum()), 1)
    print("queries %d, kept %d, excused ties %d (%.4f %%)" % (len(qry), keep.sum(), excused.sum(), 100 * share))
    assert share < 1e-3
    assert np.array_equal(gi[decided], oi[decided])
    # an excused query still names a point at the same distance
    ex = np.flatnonzero(excused)
    assert np.allclose(np.sqrt(((qry[ex] - ref[gi[ex]]) ** 2).sum(-1)), gd[ex], rtol=RTOL, atol=0)
    return keep


# ------------------------------------------------------------------------------------------------ crop
@pytest.mark.parametrize("centre", CENTRES)
def test_crop_mesh_equals_the_oracle(centre):
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, size=(5000, 3)) + np.asarray(centre)
    lo, hi = np.asarray(centre) - 0.5, np.asarray(centre) + 0.5
    v[:40] = np.where(rng.random((40, 3)) < 0.5, np.where(rng.random((40, 3)) < 0.5, lo, hi), v[:40])  # on the bounds
    v[0], v[1] = lo, hi
    f = rng.integers(0, len(v), size=(20000, 3)).astype(np.int32)
    f[:20] = rng.integers(0, 40, size=(20, 3))
    gv, gf = ev.crop_mesh(v, f, lo, hi)
    ov, of = eo.crop_mesh(v, f, lo, hi)
    assert gv.dtype == torch.float64 and gf.dtype == torch.int32 and gv.is_cuda
    assert len(ov) > 100 and len(of) > 20 and np.all(ov[0] == lo) and np.all(ov[1] == hi)
    assert np.array_equal(gv.cpu().numpy(), ov) and np.array_equal(gf.cpu().numpy(), of)
    ev_, ef = ev.crop_mesh(v, f, hi + 1, hi + 2)  # nothing inside
    assert ev_.shape == (0, 3) and ef.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ sampling
def skewed_mesh(centre):
    """one triangle with 90 % of the area, zero-area triangles (repeated vertex, collinear), 40 small ones"""
    rng = np.random.default_rng(7)
    small_v = rng.uniform(-1, 1, size=(120, 3))
    small_f = np.arange(120).reshape(40, 3)
    small_area = eo.triangle_areas(small_v, small_f).sum()
    big_area = 9.0 * small_area
    side = math.sqrt(2.0 * big_area)
    big_v = np.array([[3.0, 0, 0], [3.0 + side, 0, 0], [3.0, side, 0]])
    v = np.concatenate([small_v, big_v, [[0.0, 0, 5], [1.0, 0, 5], [2.0, 0, 5]]]) + np.asarray(centre)
    f = np.concatenate([[[120, 120, 121]], small_f[:20], [[123, 124, 125]], [[120, 121, 122]], small_f[20:], [[7, 7, 7]]]).astype(np.int32)
    return v, f


@pytest.mark.parametrize("centre", CENTRES)
def test_sampling_with_injected_uniforms_equals_the_oracle(centre):
    v, f = skewed_mesh(centre)
    areas = eo.triangle_areas(v, f)
    assert (areas == 0).sum() >= 3 and abs(areas.max() / areas.sum() - 0.9) < 1e-6
    n = 200000
    u = np.random.default_rng(8).random((n, 3))
    opts, otri, cdf = eo.sample_points(v, f, u)
    gap = np.abs(u[:, :1] - cdf[None, :]).min()
    print("closest u0 to a cumulative boundary: %.3e" % gap)
    assert gap > 1e-12  # the guard: excludes nothing
    gpts, gtri = ev.sample_points_uniformly(v, f, n, uniforms=u, return_triangles=True)
    assert np.array_equal(gtri.cpu().numpy(), otri)
    assert not np.isin(otri, np.flatnonzero(areas == 0)).any()
    assert np.allclose(gpts.cpu().numpy(), opts, rtol=1e-12, atol=0)


def test_sampling_with_a_seed_is_deterministic_uniform_and_on_the_mesh():
    rng = np.random.default_rng(9)
    v = rng.uniform(-2, 2, size=(150, 3))  # (around the origin: the checks below are then exact to ~1e-14; offsets: the test above)
    f = np.arange(150).reshape(50, 3).astype(np.int32)
    assert eo.triangle_areas(v, f).min() > 0.05
    n = 1000000
    a, tri = ev.sample_points_uniformly(v, f, n, seed=5, return_triangles=True)
    b = ev.sample_points_uniformly(v, f, n, seed=5)
    c = ev.sample_points_uniformly(v, f, n, seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # a prefix is the same whatever the launch size: samples are keyed by (seed, i)
    assert torch.equal(ev.sample_points_uniformly(v, f, 1000, seed=5), a[:1000])
    p, t = a.cpu().numpy(), tri.cpu().numpy()
    share = eo.triangle_areas(v, f)
    share = share / share.sum()
    counts = np.bincount(t, minlength=50)
    sd = np.sqrt(n * share * (1 - share))  # binomial
    z = np.abs(counts - n * share) / sd
    print("largest deviation of a triangle's sample count: %.2f sd" % z.max())
    assert np.all(z < 5.0)
    v0, v1, v2 = (v[f[t, k]] for k in range(3))
    nrm = np.cross(v1 - v0, v2 - v0)
    nn_ = np.linalg.norm(nrm, axis=1)
    assert np.abs(((p - v0) * nrm).sum(1) / nn_).max() < 1e-9
    # barycentrics in the triangle's own frame
    b1 = (np.cross(p - v0, v2 - v0) * nrm).sum(1) / nn_ ** 2
    b2 = (np.cross(v1 - v0, p - v0) * nrm).sum(1) / nn_ ** 2
    b0 = 1.0 - b1 - b2
    print("smallest barycentric coordinate: %.3e" % min(b0.min(), b1.min(), b2.min()))
    assert min(b0.min(), b1.min(), b2.min()) >= -1e-12


# ------------------------------------------------------------------------------------------------ voxel down-sampling
def check_voxel(points, voxel):
    g1, k1 = ev.voxel_down_sample(points, voxel, return_keys=True)
    g2, k2 = ev.voxel_down_sample(torch.as_tensor(points).cuda(), voxel, return_keys=True)  # device input: device bounds
    om, ok = eo.voxel_down_sample(points, voxel)
    assert torch.equal(g1, g2) and torch.equal(k1, k2)  # bit-identical across two runs
    k = k1.cpu().numpy()
    assert np.array_equal(k, ok) and np.all(np.diff(k) > 0)
    assert np.allclose(g1.cpu().numpy(), om, rtol=1e-12, atol=0)
    return len(ok)


@pytest.mark.parametrize("centre", CENTRES)
def test_voxel_down_sample_equals_the_oracle(centre):
    pts = noisy_sphere(1000000, 1.0, centre, 0.002, 21)
    m = check_voxel(pts, 0.02)
    assert 20000 < m < 200000
    assert check_voxel(pts[:5000], 0.5) < 200  # hundreds of points per voxel


def test_voxel_down_sample_small_and_negative_clouds():
    rng = np.random.default_rng(22)
    check_voxel(rng.uniform(-3, -1, size=(20000, 3)), 0.1)
    check_voxel(rng.uniform(-1, 1, size=(20000, 3)), 0.07)
    assert check_voxel(np.array([[-4.0, 2.5, 1e3]]), 0.02) == 1
    assert check_voxel(np.repeat(np.array([[1.0, 2.0, 3.0]]), 100, 0), 0.02) == 1
    assert ev.voxel_down_sample(np.zeros((0, 3)), 0.02).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ nearest neighbour
@pytest.mark.parametrize("centre", CENTRES)
def test_nn_correspondence_equals_brute_force(centre):
    c = np.asarray(centre)
    rng = np.random.default_rng(31)
    n, blob = 50000, 2000
    ref = np.concatenate([noisy_sphere(n - blob, 1.00, c, 0.002, 32), c + [9.0, 0, 0] + rng.normal(scale=0.1, size=(blob, 3))])
    qry = np.concatenate([noisy_sphere(n - blob, 1.03, c, 0.002, 33), c + [0, -7.0, 1.0] + rng.normal(scale=0.1, size=(blob, 3))])
    qry = qry[rng.permutation(n)]  # the caller's order is arbitrary
    truncation = 0.2
    oracle = eo.nn_brute(ref, qry, second=True)
    res = ev.nn_correspondence(ref, qry, truncation, True)
    keep = check_nn(res.index, res.dist, res.keep, ref, qry, truncation, oracle)
    assert (~keep).sum() > 0 and keep.sum() > 0  # the dropped and the kept branch
    oi, od, ok = eo.nn_correspondence(ref, qry, truncation, True, nearest=oracle[:2])
    assert len(res.distances) == keep.sum() and np.allclose(res.distances.cpu().numpy(), od, rtol=RTOL, atol=0)
    assert np.array_equal(res.indices.cpu().numpy(), res.index.cpu().numpy()[keep])
    # clamped instead of dropped
    res2 = ev.nn_correspondence(ref, qry, truncation, False)
    oi2, od2, ok2 = eo.nn_correspondence(ref, qry, truncation, False, nearest=oracle[:2])
    assert (od2 == truncation).sum() == (~keep).sum() > 0
    assert len(res2.distances) == n and np.allclose(res2.distances.cpu().numpy(), od2, rtol=RTOL, atol=0)
    assert torch.equal(res2.dist, res.dist) and torch.equal(res2.index, res.index)
    # another cell size, same answer (the grid is an accelerator, not part of the result)
    res3 = ev.nn_correspondence(ref, qry, truncation, True, cell=0.31)
    assert torch.equal(res3.dist, res.dist) and torch.equal(res3.keep, res.keep)


def test_nn_correspondence_edge_cases():
    rng = np.random.default_rng(41)
    c = np.asarray(CENTRES[0])
    ref = rng.normal(size=(3000, 3)) + c
    qry = rng.normal(size=(1000, 3)) + c
    for r, q in ((np.zeros((0, 3)), qry), (ref, np.zeros((0, 3)))):  # either set empty: empty result
        e = ev.nn_correspondence(r, q, 0.5)
        assert len(e.indices) == 0 and len(e.distances) == 0 and len(e.keep) == 0
    # all queries identical
    same = np.repeat(qry[:1], 777, 0)
    s = ev.nn_correspondence(ref, same, 10.0)
    oi, od = eo.nn_brute(ref, same)
    assert np.all(s.index.cpu().numpy() == oi) and np.allclose(s.dist.cpu().numpy(), od, rtol=RTOL, atol=0)
    # a reference of one point
    one = ev.nn_correspondence(ref[:1], qry, 100.0)
    assert np.all(one.index.cpu().numpy() == 0)
    assert np.allclose(one.dist.cpu().numpy(), np.sqrt(((qry - ref[0]) ** 2).sum(-1)), rtol=RTOL, atol=0)
    # duplicated reference points: any of the duplicates, same distance
    dup = np.concatenate([ref, ref[:500], ref[:500]])
    d = ev.nn_correspondence(dup, qry, 100.0)
    oi, od = eo.nn_brute(ref, qry)
    gi = d.index.cpu().numpy()
    assert np.allclose(d.dist.cpu().numpy(), od, rtol=RTOL, atol=0)
    assert np.array_equal(np.where(gi >= len(ref), (gi - len(ref)) % 500, gi), oi)
    # a query exactly `truncation` away is dropped (strict <); axis-aligned so that the distance is exact
    r2 = np.array([[64.0, -32.0, 4.0], [80.0, -32.0, 4.0]])
    q2 = np.array([[64.5, -32.0, 4.0], [64.0, -32.25, 4.0], [64.0, -32.0, 4.5 - 2.0 ** -40], [80.0, -31.5, 4.0]])
    t = ev.nn_correspondence(r2, q2, 0.5, False)
    assert t.keep.cpu().tolist() == [False, True, True, False]
    assert t.dist.cpu().tolist() == pytest.approx([0.5, 0.25, 0.5 - 2.0 ** -40, 0.5], rel=1e-15) and t.index.cpu().tolist() == [-1, 0, 0, -1]
    assert t.dist.cpu().tolist()[0] == 0.5 and t.dist.cpu().tolist()[2] < 0.5
    assert len(ev.nn_correspondence(r2, q2, 0.5, True).distances) == 2
    # queries far outside the reference's box, and without any truncation to speak of
    far = np.array([[1e4, 0, 0], [c[0], c[1], c[2] + 50.0]])
    g = ev.nn_correspondence(ref, far, 1e6)
    oi, od = eo.nn_brute(ref, far)
    assert np.array_equal(g.index.cpu().numpy(), oi) and np.allclose(g.dist.cpu().numpy(), od, rtol=RTOL, atol=0)


def big_pair(outliers):
    """two surface-like clouds 3 cm apart, 2 * 10^6 points each at ~0.02 m spacing (spheres of 8 m); with `outliers`, 5 % of the
    queries are farther than 2 m from every reference point: half deep inside the sphere, half in a far box"""
    c = np.asarray(CENTRES[1])
    n = 2000000
    ref = noisy_sphere(n, 8.00, c, 0.002, 51)
    qry = noisy_sphere(n, 8.03, c, 0.002, 52)
    if outliers:
        rng = np.random.default_rng(53)
        k = n // 20
        where = rng.choice(n, k, replace=False)
        inside = rng.normal(size=(k // 2, 3))
        inside *= (rng.random((k // 2, 1)) ** (1 / 3) * 5.0) / np.linalg.norm(inside, axis=1, keepdims=True)
        qry[where[:k // 2]] = c + inside
        qry[where[k // 2:]] = c + [30.0, 10.0, -5.0] + rng.uniform(-5, 5, size=(k - k // 2, 3))
    return ref, qry


def oracle_at_size(ref, qry):
    """(rows checked, their (index, distance, second-best)): the tree on everything when scipy imports, else brute force on
    4096 randomly chosen queries"""
    if eo.have_scipy():
        print("oracle: cKDTree on all %d queries" % len(qry))
        return np.arange(len(qry)), eo.nn_tree(ref, qry, second=True)
    rows = np.random.default_rng(54).choice(len(qry), 4096, replace=False)
    print("oracle: brute force on 4096 randomly chosen queries (scipy does not import)")
    return rows, eo.nn_brute(ref, qry[rows], second=True)


def test_nn_correspondence_at_size():
    ref, qry = big_pair(False)
    rows, oracle = oracle_at_size(ref, qry)
    res = ev.nn_correspondence(ref, qry, 0.2, True, spacing=0.02)
    check_nn(res.index[rows], res.dist[rows], res.keep[rows], ref, qry[rows], 0.2, oracle)


def test_nn_correspondence_outliers_are_bounded_and_not_slower_than_the_tree():
    ref, qry = big_pair(True)
    truncation, spacing = 2.0, 0.02
    rows, oracle = oracle_at_size(ref, qry)
    r_dev, q_dev = torch.as_tensor(ref).cuda(), torch.as_tensor(qry).cuda()
    res = ev.nn_correspondence(r_dev, q_dev, truncation, False, spacing=spacing, stats=True)
    keep = check_nn(res.index[rows], res.dist[rows], res.keep[rows], ref, qry[rows], truncation, oracle)
    assert (~keep).sum() >= (0.049 * len(qry) if len(rows) == len(qry) else 1)
    # (i) structure: the bound of the documented layout, from the parameters the module exposes
    coarse = res.cell * ev.FINE_PER_COARSE
    assert res.cell == ev.CELL_FACTOR * spacing
    max_coarse = (2 * math.ceil(truncation / coarse) + 1) ** 3
    max_fine = ev.FINE_PER_COARSE ** 3 * max_coarse
    print("cells visited by one query at most: %d coarse (bound %d), %d fine (bound %d)"
          % (res.max_coarse_cells, max_coarse, res.max_fine_cells, max_fine))
    assert 0 < res.max_coarse_cells <= max_coarse and 0 < res.max_fine_cells <= max_fine
    # (ii) against the reference's method: the warm device call (grid build included) must not be slower than the tree's query
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res2 = ev.nn_correspondence(r_dev, q_dev, truncation, False, spacing=spacing)
    b.record()
    torch.cuda.synchronize()
    dev_s = a.elapsed_time(b) * 1e-3
    assert torch.equal(res2.dist, res.dist)
    if not eo.have_scipy():
        print("device %.4f s; scipy does not import: no tree to compare with" % dev_s)
        return
    from scipy.spatial import cKDTree

    tree = cKDTree(ref)
    t0 = time.perf_counter()
    tree.query(qry, k=1, workers=16)
    cpu_s = time.perf_counter() - t0
    print("2e6 x 2e6 with 5 %% outliers: device %.4f s (%.3g queries/s), cKDTree.query(workers=16) %.3f s" % (dev_s, len(qry) / dev_s, cpu_s))
    assert dev_s <= cpu_s


# ------------------------------------------------------------------------------------------------ metrics, eval_mesh
def test_distance_sums_equal_numpy():
    rng = np.random.default_rng(61)
    # (n_p, n_r); the longer one sets the grid: one workgroup of 256, two, exactly the 256 workgroups of the reduction without
    # and with a strided tail, and many strides
    for n_p, n_r in ((1234567, 54321), (1, 1), (256, 100), (100, 257), (65536, 3), (1000, 65537)):
        dp, dr = rng.random(n_p) * 0.2, rng.random(n_r) * 2.0
        s = ev.distance_sums(torch.as_tensor(dp).cuda(), torch.as_tensor(dr).cuda(), 0.05)
        want = [dp.sum(), (dp ** 2).sum(), (dp < 0.05).sum(), dr.sum(), (dr ** 2).sum(), (dr < 0.05).sum(), len(dp), len(dr)]
        assert np.allclose(s, want, rtol=RTOL, atol=0) and s[2] == want[2] and s[5] == want[5], (n_p, n_r)
        s2 = ev.distance_sums(torch.as_tensor(dp).cuda(), torch.as_tensor(dr).cuda(), 0.05)
        assert np.array_equal(s, s2), (n_p, n_r)
    e = ev.distance_sums(torch.zeros(0, dtype=torch.float64).cuda(), torch.as_tensor(dr).cuda(), 0.05)
    assert e[:3].tolist() == [0, 0, 0] and e[6] == 0 and e[7] == len(dr)
    m = ev.metrics_from_sums(e, 0.02, 0.05, 0.2, 2.0)
    assert np.isnan(m["MAE_accuracy (m)"]) and np.isnan(m["F-score (%)"]) and not np.isnan(m["MAE_completeness (m)"])


def sphere_mesh(centre, radius=1.0, voxel=0.05, half=1.6):
    n = int(round(2 * half / voxel)) + 1
    ax = torch.arange(n, dtype=torch.float64, device="cuda") * voxel - half
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    sdf = (torch.sqrt(x * x + y * y + z * z) - radius).float().contiguous()
    verts, faces = mesher.marching_cubes(sdf)
    v = verts.double() * voxel - half + torch.as_tensor(np.asarray(centre), device="cuda")
    return v.contiguous(), faces


def compare_dicts(got, want, dist_p, dist_r, threshold, tacc, tcom):
    assert list(got) == eo.METRIC_KEYS
    assert_clear_of(dist_p, threshold, tacc)
    assert_clear_of(dist_r[dist_r < tcom], threshold, tcom)  # (a clamped distance IS the truncation: the guard is on the rest)
    for k in eo.METRIC_KEYS[:4]:
        assert got[k] == pytest.approx(want[k], rel=RTOL, abs=0), k
    for k in eo.METRIC_KEYS[4:6] + eo.METRIC_KEYS[7:]:
        assert got[k] == want[k], k
    assert got["F-score (%)"] == pytest.approx(want["F-score (%)"], rel=1e-14)
    print({k: got[k] for k in eo.METRIC_KEYS[:7]})


@pytest.mark.parametrize("centre", CENTRES)
def test_eval_mesh_end_to_end_equals_the_oracle(centre, tmp_path):
    v, f = sphere_mesh(centre)
    trgt = noisy_sphere(400000, 1.03, centre, 0.002, 71)
    kw = dict(down_sample_res=0.02, threshold=0.031, truncation_acc=0.2, truncation_com=2.0)
    n = 2000000
    got = ev.eval_mesh((v, f), trgt, mesh_sample_point=n, seed=3, gt_bbx_mask_on=False, **kw)
    sampled = ev.sample_points_uniformly(v, f, n, seed=3).cpu().numpy()  # the device's own stream, shared with the oracle
    want, dp, dr = eo.eval_mesh_from_points(sampled, trgt, return_distances=True, **kw)
    compare_dicts(got, want, dp, dr, 0.031, 0.2, 2.0)
    assert 0.0 < got["Precision [Accuracy] (%)"] < 100.0 and 0.0 < got["Recall [Completeness] (%)"] < 100.0
    # through files: the same dict
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    pm, pc = str(tmp_path / "mesh.ply"), str(tmp_path / "gt.ply")
    write_ply(pm, [("x", vn[:, 0], "double"), ("y", vn[:, 1], "double"), ("z", vn[:, 2], "double")], fn)
    write_ply(pc, [("x", trgt[:, 0], "double"), ("y", trgt[:, 1], "double"), ("z", trgt[:, 2], "double")])
    from_files = ev.eval_mesh(pm, pc, mesh_sample_point=n, seed=3, gt_bbx_mask_on=False, **kw)
    assert from_files == got
    assert ev.eval_mesh(mesher.TriangleMesh(vn, fn), torch.as_tensor(trgt), mesh_sample_point=n, seed=3, gt_bbx_mask_on=False, **kw) == got


def test_eval_mesh_bbx_mask_crops_a_mesh_that_sticks_out():
    centre = CENTRES[0]
    v, f = sphere_mesh(centre)
    full = noisy_sphere(400000, 1.03, centre, 0.002, 72)
    trgt = full[full[:, 2] < centre[2] + 0.4]  # the target's box ends below the top of the mesh
    kw = dict(down_sample_res=0.02, threshold=0.031, truncation_acc=0.2, truncation_com=2.0)
    n = 2000000
    lo, hi = trgt.min(0), trgt.max(0)
    lo[2] -= 0.02
    hi[2] += 0.02
    cv, cf = eo.crop_mesh(v.cpu().numpy(), f.cpu().numpy(), lo, hi)
    assert 0 < len(cf) < len(f)
    on = ev.eval_mesh((v, f), trgt, mesh_sample_point=n, seed=4, gt_bbx_mask_on=True, **kw)
    sampled = ev.sample_points_uniformly(cv, cf, n, seed=4).cpu().numpy()
    want, dp, dr = eo.eval_mesh_from_points(sampled, trgt, return_distances=True, **kw)
    compare_dicts(on, want, dp, dr, 0.031, 0.2, 2.0)
    off = ev.eval_mesh((v, f), trgt, mesh_sample_point=n, seed=4, gt_bbx_mask_on=False, **kw)
    sampled = ev.sample_points_uniformly(v, f, n, seed=4).cpu().numpy()
    want_off, dp, dr = eo.eval_mesh_from_points(sampled, trgt, return_distances=True, **kw)
    compare_dicts(off, want_off, dp, dr, 0.031, 0.2, 2.0)
    # the part of the mesh above the target's box has no target nearby: it costs accuracy only when it is not cropped
    assert off["MAE_accuracy (m)"] > on["MAE_accuracy (m)"]
    # no down-sampling at all (the reference fails there)
    raw = ev.eval_mesh((v, f), trgt[:50000], mesh_sample_point=100000, seed=4, gt_bbx_mask_on=True, down_sample_res=0, threshold=0.031,
                       truncation_acc=0.2, truncation_com=2.0)
    assert raw["Spacing (m)"] == 0 and np.isfinite(raw["Chamfer_L1 (m)"])


def test_crop_intersection_writes_the_filtered_cloud(tmp_path):
    centre = CENTRES[0]
    v, f = sphere_mesh(centre)
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    half = fn[vn[fn].mean(1)[:, 0] > centre[0]]  # a second prediction that covers half of the sphere
    gt = noisy_sphere(30000, 1.02, centre, 0.01, 81)  # (sizes a brute-force oracle can take when scipy does not import)
    p1, p2, pg, out = (str(tmp_path / s) for s in ("a.ply", "b.ply", "gt.ply", "crop.ply"))
    for p, ff in ((p1, fn), (p2, half)):
        write_ply(p, [("x", vn[:, 0], "double"), ("y", vn[:, 1], "double"), ("z", vn[:, 2], "double")], ff)
    write_ply(pg, [("x", gt[:, 0], "double"), ("y", gt[:, 1], "double"), ("z", gt[:, 2], "double")])
    ev.crop_intersection(pg, [p1, p2], out, dist_thre=0.03, mesh_sample_point=100000, seed=2)
    want = gt
    for ff in (fn, half):
        s = ev.sample_points_uniformly(vn, ff, 100000, seed=2).cpu().numpy()
        _, d = eo.nn(s, want)[:2]
        assert_clear_of(d, 0.03)
        want = want[d * d < 0.03 ** 2]
    got = ev.read_ply(out)
    assert got["faces"] is None and 0 < len(want) < len(gt)
    assert np.array_equal(got["vertices"], want)


def test_cli_prints_the_dict_and_writes_the_csv(tmp_path):
    import subprocess
    import sys

    from conftest import ROOT

    centre = CENTRES[0]
    v, f = sphere_mesh(centre)
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    gt = noisy_sphere(50000, 1.03, centre, 0.002, 91)
    pm, pc, out = (str(tmp_path / s) for s in ("mesh.ply", "gt.ply", "e.csv"))
    write_ply(pm, [("x", vn[:, 0], "double"), ("y", vn[:, 1], "double"), ("z", vn[:, 2], "double")], fn)
    write_ply(pc, [("x", gt[:, 0], "double"), ("y", gt[:, 1], "double"), ("z", gt[:, 2], "double")])
    r = subprocess.run([sys.executable, "-m", "shine_mapping_amd.evaluation", pm, pc, "--spacing", "0.02", "--threshold", "0.031",
                        "--trunc-acc", "0.2", "--trunc-com", "2.0", "--samples", "300000", "--seed", "6", "--csv", out],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    want = ev.eval_mesh(pm, pc, down_sample_res=0.02, threshold=0.031, truncation_acc=0.2, truncation_com=2.0,
                        mesh_sample_point=300000, seed=6)
    assert repr(want) in r.stdout
    lines = open(out).read().splitlines()
    assert lines[0] == ",".join(eo.METRIC_KEYS) and [float(x) for x in lines[1].split(",")] == [want[k] for k in eo.METRIC_KEYS]
