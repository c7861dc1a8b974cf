"""GPU suite of the frame front-end (shine_mapping_amd/dataset.py, csrc/shine_frame.hip):
  * shine_ray_sample with injected uniforms against the reference's own dataSampler.sample (tests/golden/frame_sampler.pt, written by
    tools/make_frame_golden.py): per tensor max|device - ref64| <= 4 x e_ref, e_ref = the reference's own fp32-vs-fp64 distance;
  * its generator: reproducible, keyed by the frame id, label ranges, a 64-bin uniformity test sized from the sample count;
  * filter, voxel means, boxes, random subset and the window filter against the numpy fp64 oracle (tests/frame_oracle.py);
  * LiDARDataset end to end on a synthetic KITTI-format drive: batch, incremental, window replay, training and meshing.
Every comparison prints its figures before it asserts."""
import math
import os

import numpy as np
import pytest
import torch

import frame_oracle as fo
from conftest import load_golden

pytestmark = pytest.mark.gpu

BOUND_FACTOR = 4.0  # x e_ref: two correct fp32 evaluations in different operation orders each sit within ~e_ref of exact


def _params(case):
    from types import SimpleNamespace

    from shine_mapping_amd.dataset import SamplerParams

    return SamplerParams(SimpleNamespace(
        scale=case["scale"], surface_sample_n=case["ns"], clearance_sample_n=case["nc"], free_sample_n=case["nf"],
        surface_sample_range_m=case["surface_sample_range_m"], clearance_dist_m=case["clearance_dist_m"],
        free_sample_begin_ratio=case["free_sample_begin_ratio"], free_sample_end_dist_m=case["free_sample_end_dist_m"]))


def test_ray_sample_matches_the_reference_sampler_on_its_own_uniforms():
    from shine_mapping_amd.dataset import ray_sample

    fx = load_golden("frame_sampler")
    e_ref = fx["e_ref"]
    assert e_ref["weight"] == 0.0 and all(e_ref[k] > 0 for k in ("coord", "sdf_label", "sample_depth", "ray_depth"))
    worst = {k: 0.0 for k in ("coord", "sdf_label", "sample_depth", "ray_depth")}
    for ci, case in enumerate(fx["cases"]):
        p = _params(case)
        m, S = case["points"].shape[0], p.S
        out = ray_sample(case["points"].cuda(), case["origin"].tolist(), p, uniforms=case["uniforms"].cuda(),
                         labels=case["labels"].cuda() if case["labels"] is not None else None, time_value=7.0 + ci)
        torch.cuda.synchronize()
        for k in worst:
            d = float((out[k].double().cpu() - case[k]).abs().max())
            worst[k] = max(worst[k], d)
            print("case %d (%d, %d, %d) m=%d  %-12s max|device - ref64| = %.3e   e_ref = %.3e   bound = %.3e"
                  % (ci, case["ns"], case["nc"], case["nf"], m, k, d, e_ref[k], BOUND_FACTOR * e_ref[k]))
        # exact: weight (and with it the ray-major order: ns surface samples first in every ray), labels, time, origin rows
        assert torch.equal(out["weight"].cpu(), case["weight"].float())
        want_w = torch.tensor([1.0] * case["ns"] + [-1.0] * (case["nc"] + case["nf"])).repeat(m)
        assert torch.equal(out["weight"].cpu(), want_w)
        if case["labels"] is not None:
            assert out["sem_label"].dtype == torch.int32 and torch.equal(out["sem_label"].cpu(), case["sem_label"])
            assert torch.equal(out["sem_label"].cpu().view(m, S)[:, 0], case["labels"])
        else:
            assert "sem_label" not in out
        assert torch.equal(out["time"].cpu(), torch.full((m * S,), 7.0 + ci))
        assert torch.equal(out["origin"].cpu(), case["origin"].repeat(m * S, 1))
        assert out["coord"].shape == (m * S, 3) and out["ray_depth"].shape == (m,)
    for k, d in worst.items():
        assert d <= BOUND_FACTOR * e_ref[k], (k, d, e_ref[k])


def test_ray_sample_with_no_rays_and_with_skipped_outputs():
    from shine_mapping_amd.dataset import ray_sample

    fx = load_golden("frame_sampler")
    case = fx["cases"][0]
    p = _params(case)
    out = ray_sample(torch.empty((0, 3), device="cuda"), [0.0, 0.0, 0.0], p)
    assert out["coord"].shape == (0, 3) and out["sdf_label"].shape == (0,) and out["ray_depth"].shape == (0,)
    # null depth / origin / time pointers: the other outputs are what the full call writes
    pts, u = case["points"].cuda(), case["uniforms"].cuda()
    full = ray_sample(pts, case["origin"].tolist(), p, uniforms=u)
    part = ray_sample(pts, case["origin"].tolist(), p, uniforms=u, depths=False, origin_time=False)
    assert sorted(part) == ["coord", "sdf_label", "weight"]
    for k in part:
        assert torch.equal(part[k], full[k])
    # written straight into caller's buffers (the pools' tails)
    m, S = pts.shape[0], p.S
    buf = torch.zeros((m * S + 5, 3), device="cuda")
    got = ray_sample(pts, case["origin"].tolist(), p, uniforms=u, out={"coord": buf[2:2 + m * S]}, depths=False, origin_time=False)
    assert got["coord"].data_ptr() == buf[2:].data_ptr() and torch.equal(buf[2:2 + m * S], full["coord"])
    assert float(buf[:2].abs().max()) == 0.0 and float(buf[2 + m * S:].abs().max()) == 0.0


def test_ray_sample_generator_is_reproducible_in_range_and_uniform():
    from types import SimpleNamespace

    from shine_mapping_amd.dataset import SamplerParams, ray_sample

    cfg = SimpleNamespace(scale=0.02, surface_sample_n=4, clearance_sample_n=1, free_sample_n=1, surface_sample_range_m=0.3,
                          clearance_dist_m=0.25, free_sample_begin_ratio=0.3, free_sample_end_dist_m=0.8)
    p = SamplerParams(cfg)
    m, S, ns = 1 << 20, p.S, p.ns
    g = torch.Generator(device="cuda").manual_seed(5)
    d = torch.randn((m, 3), device="cuda", generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    origin = [0.05, -0.02, 0.01]
    pts = torch.tensor(origin, device="cuda") + d * ((3.0 + 47.0 * torch.rand((m, 1), device="cuda", generator=g)) * cfg.scale)
    a = ray_sample(pts, origin, p, seed=42, stream_id=3)
    b = ray_sample(pts, origin, p, seed=42, stream_id=3)
    c = ray_sample(pts, origin, p, seed=42, stream_id=4)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["sdf_label"], c["sdf_label"]) and not torch.equal(a["coord"], c["coord"])
    # r and c as the reference defines them: the double products surface_sample_range_m * scale and clearance_dist_m * scale
    # (utils/data_sampler.py:27,33).  Their fp32 roundings are NOT the interval's ends: with the largest 24-bit uniform the
    # reference's own fp32 expression -u * c - r returns -(fl32(r) + fl32(c)) exactly (checked with the real dataSampler on the
    # CPU), so an open end computed from the rounded constants is reached by the reference itself.
    r, cl = p.surface_range, p.clearance_dist
    lab = a["sdf_label"].view(m, S).double()
    surf, clear = lab[:, :ns], lab[:, ns:ns + 1]
    print("surface labels in [%.9g, %.9g], r = %.9g" % (float(surf.min()), float(surf.max()), float(r)))
    assert float(surf.min()) >= -float(r) and float(surf.max()) < float(r)
    print("clearance labels in [%.9g, %.9g], -(r + c) = %.9g" % (float(clear.min()), float(clear.max()), -(float(r) + float(cl))))
    assert float(clear.max()) <= -float(r) and float(clear.min()) > -(float(r) + float(cl))
    # free space: ratio = depth / ray depth in [lo, end / dist + 1] up to the fp32 rounding of that quotient (4 ulp)
    ratio = (a["sample_depth"].view(m, S)[:, S - 1] / a["ray_depth"]).double()
    dist = a["ray_depth"].double() * cfg.scale
    hi = p.free_end_dist / dist + 1.0
    ulp4 = 4 * 2.0 ** -23
    print("free ratio - lo >= %.3e, hi - ratio >= %.3e" % (float((ratio - p.free_begin_ratio).min()), float((hi - ratio).min())))
    assert bool((ratio >= p.free_begin_ratio * (1 - ulp4)).all()) and bool((ratio <= hi * (1 + ulp4)).all())
    assert bool((a["sdf_label"].view(m, S)[:, S - 1] < 0).any()) and bool((a["sdf_label"].view(m, S)[:, S - 1] > 0).any())
    # uniformity: the uniforms recovered from n >= 2^22 surface labels, 64 equal bins, binomial expectation +- 5 sigma
    n = m * ns
    assert n >= 1 << 22
    u = surf.reshape(-1) / (2.0 * float(r)) + 0.5
    counts = torch.bincount(torch.clamp((u * 64).long(), 0, 63), minlength=64).double().cpu().numpy()
    sigma = math.sqrt(n * (1 / 64) * (63 / 64))
    dev = np.abs(counts - n / 64).max()
    print("n = %d, bins within %.2f sigma (bound 5)" % (n, dev / sigma))
    assert dev <= 5 * sigma
    # and the samples of one ray do not share their uniform
    assert float((surf[:, 0] - surf[:, 1]).abs().min()) >= 0.0 and float((surf[:, 0] - surf[:, 1]).abs().mean()) > 0.1 * float(r)


def _cloud(n, seed, radius=25.0, min_z=-3.0, max_z=30.0, min_range=2.5):
    """random float32 cloud that straddles every bound, with points exactly on the crop faces, at min_range and at min_z"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.3, 1.3, size=(n, 3)) * np.array([radius, radius, 0.5 * (max_z - min_z)]) + np.array([0, 0, 0.5 * (max_z + min_z)])
    near = rng.normal(size=(n // 10, 3))
    p[: n // 10] = near / np.linalg.norm(near, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n // 10, 1)) * min_range
    p = p.astype(np.float32)
    k = n // 3
    p[k] = [radius, 0.0, 0.0]
    p[k + 1] = [-radius, radius, 1.0]
    p[k + 2] = [3.0, 4.0, max_z]
    p[k + 3] = [min_range, 0.0, 0.0]
    p[k + 4] = [5.0, 5.0, min_z]
    p[k + 5] = [0.6 * min_range, 0.8 * min_range, 0.0]
    return p


@pytest.mark.parametrize("n", [1, 777, 2048, 2049, 130000, 1 << 21])
def test_frame_filter_keeps_exactly_the_oracle_set(n):
    """the larger sizes are 64 and 1024 tiles: the chained prefix looks back over more than one wave of tiles"""
    from shine_mapping_amd.dataset import frame_filter

    R, min_z, max_z, min_range = 25.0, -3.0, 30.0, 2.5
    p = _cloud(max(n, 16), 100 + n % 97)[:n]
    keep = fo.filter_mask(p, min_z, max_z, min_range, R)
    want = p[keep].astype(np.float64)
    print("n = %d, oracle keeps %d" % (n, keep.sum()))
    if n >= 16:
        assert 0 < keep.sum() < n
    got3 = frame_filter(torch.from_numpy(np.ascontiguousarray(p)).cuda(), min_z, max_z, min_range, R)
    p4 = np.zeros((n, 4), np.float32)
    p4[:, :3] = p
    p4[:, 3] = 0.5
    got4 = frame_filter(torch.from_numpy(p4).cuda(), min_z, max_z, min_range, R)
    got64 = frame_filter(torch.from_numpy(p.astype(np.float64)).cuda(), min_z, max_z, min_range, R)
    for got in (got3, got4, got64):
        assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)  # the same points in the same order


def test_frame_filter_special_points():
    from shine_mapping_amd.dataset import frame_filter

    pts = np.array([[25.0, 0.0, 0.0], [-25.0, 25.0, 1.0], [3.0, 4.0, 30.0], [25.000002, 0.0, 0.0], [2.5, 0.0, 0.0],
                    [1.5, 2.0, 0.0], [2.4999, 0.0, 0.0], [5.0, 5.0, -3.0], [5.0, 5.0, -2.999], [0.0, 0.0, 31.0]], np.float32)
    got = frame_filter(torch.from_numpy(pts).cuda(), -3.0, 30.0, 2.5, 25.0).cpu().numpy()
    assert np.array_equal(got, pts[[0, 1, 2, 4, 5, 8]].astype(np.float64))
    assert frame_filter(torch.empty((0, 4), device="cuda"), -3.0, 30.0, 2.5, 25.0).shape == (0, 3)


@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    from shine_mapping_amd import synth

    folder = str(tmp_path_factory.mktemp("drive"))
    cfg = synth.make_config("ncd", device="cuda")
    return synth.write_kitti_drive(folder, cfg, frames=6, beams=32, azimuths=180, device="cpu")


def _dataset(drive, with_octree=True, **over):
    from shine_mapping_amd import FeatureOctree, synth
    from shine_mapping_amd.dataset import LiDARDataset

    # (a crop radius and a minimum range inside the scan's 1.5-25 m, so that the filter really drops points)
    cfg = synth.dataset_config("ncd", drive, **dict(dict(pc_radius=20.0, min_range=2.5), **over))
    torch.manual_seed(1)
    octree = FeatureOctree(cfg) if with_octree else None
    return cfg, octree, LiDARDataset(cfg, octree)


def _oracle_frames(drive, cfg, ds):
    return [fo.frame(fo.read_kitti_bin(os.path.join(cfg.pc_path, ds.pc_filenames[f])), ds.poses_ref[f], cfg)
            for f in range(drive.frames)]


def test_frame_stages_equal_the_oracle(drive):
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd.dataset import frame_filter

    cfg, _, ds = _dataset(drive, with_octree=False)
    lo_all, hi_all = None, None
    for f in range(3):
        raw = fo.read_kitti_bin(os.path.join(cfg.pc_path, ds.pc_filenames[f]))
        want = fo.frame(raw, ds.poses_ref[f], cfg)
        kept = frame_filter(ds.read_point_cloud(os.path.join(cfg.pc_path, ds.pc_filenames[f])), cfg.min_z, cfg.max_z, cfg.min_range,
                            cfg.pc_radius)
        assert np.array_equal(kept.cpu().numpy(), raw[want["kept"]].astype(np.float64))
        means, keys = ev.voxel_down_sample(kept, cfg.vox_down_m, return_keys=True)
        assert np.array_equal(keys.cpu().numpy(), want["sensor_keys"])
        assert np.allclose(means.cpu().numpy(), want["sensor"], rtol=1e-12, atol=0)
        assert torch.equal(ds.frame_points(f), means)
        ds.process_frame(f)
        cur = ds.cur_frame_pc.points.cpu().numpy()
        print("frame %d: %d raw, %d kept, %d down-sampled, %d in the map copy" % (f, len(raw), len(want["kept"]), len(means), len(cur)))
        assert cur.shape == want["cur"].shape and np.allclose(cur, want["cur"], rtol=1e-12, atol=1e-12)
        assert np.allclose(ds.cur_bbx.get_min_bound(), want["lo"], rtol=1e-12, atol=1e-12)
        assert np.allclose(ds.cur_bbx.get_max_bound(), want["hi"], rtol=1e-12, atol=1e-12)
        lo_all = want["lo"] if lo_all is None else np.minimum(lo_all, want["lo"])
        hi_all = want["hi"] if hi_all is None else np.maximum(hi_all, want["hi"])
    assert np.allclose(ds.map_bbx.get_min_bound(), lo_all, rtol=1e-12, atol=1e-12)
    assert np.allclose(ds.map_bbx.get_max_bound(), hi_all, rtol=1e-12, atol=1e-12)
    merged = ds.map_down_pc.points.cpu().numpy()
    assert len(ds.map_down_pc) == len(merged) and np.allclose(merged.min(0), lo_all, rtol=1e-12, atol=1e-12)


def test_rand_downsample_keeps_exactly_int_n_r_input_points(drive):
    cfg, _, ds = _dataset(drive, with_octree=False, rand_downsample=True, rand_down_r=0.37)
    raw = fo.read_kitti_bin(os.path.join(cfg.pc_path, ds.pc_filenames[2]))
    kept = raw[fo.filter_mask(raw, cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius)].astype(np.float64)
    a = ds.frame_points(2).cpu().numpy()
    assert a.shape == (int(len(kept) * 0.37), 3)
    rows = {r.tobytes() for r in kept}
    assert all(r.tobytes() in rows for r in a) and len({r.tobytes() for r in a}) == len(a)  # distinct input points
    assert np.array_equal(a, ds.frame_points(2).cpu().numpy())  # reproducible
    assert not np.array_equal(a[:50], ds.frame_points(3).cpu().numpy()[:50])
    ds.process_frame(2)
    assert len(ds) == len(a) * ds.sampler.S


@pytest.mark.parametrize("n", [1, 1000, 1024, 70000, 3000000])
def test_pool_window_filter_equals_the_torch_expression_and_keeps_six_arrays_aligned(n):
    from shine_mapping_amd.dataset import pool_window_filter

    g = torch.Generator(device="cuda").manual_seed(n)
    origin = torch.tensor([0.11, -0.07, 0.02], device="cuda")
    radius = float(np.float32(0.25))
    coord = origin + (torch.rand((2 * n + 64, 3), device="cuda", generator=g) - 0.5) * 0.7
    dist = (coord - origin).norm(2, dim=-1)
    coord = coord[(dist - radius).abs() >= 1e-5][:n].contiguous()  # no sample within 1e-5 (scaled) of the radius ...
    assert coord.shape[0] == n
    dist = (coord - origin).norm(2, dim=-1)
    assert float((dist - radius).abs().min()) >= 1e-5  # ... asserted on the inputs the filter sees
    mask = dist < radius
    idx = torch.arange(n, device="cuda")
    arrays = [coord, torch.rand(n, device="cuda", generator=g), torch.rand(n, device="cuda", generator=g),
              torch.rand((n, 3), device="cuda", generator=g), idx.float() if n < (1 << 24) else idx.int(),
              idx.int()]
    outs, kept = pool_window_filter(coord, origin.tolist(), radius, arrays)
    print("n = %d: kept %d, torch keeps %d" % (n, kept, int(mask.sum())))
    assert kept == int(mask.sum())
    for a, o in zip(arrays, outs):
        assert o.shape == a.shape and torch.equal(o[:kept], a[mask])
    if n >= 1000:
        assert 0 < kept < n
    # the numpy oracle agrees with the torch expression on these inputs
    assert np.array_equal(fo.window_mask(coord.cpu().numpy(), origin.cpu().numpy(), radius)[0], mask.cpu().numpy())


def _rows(*tensors):
    cols = [t.detach().float().cpu().reshape(t.shape[0], -1) for t in tensors]
    return np.ascontiguousarray(torch.cat(cols, 1).numpy())


def _check_batch(cfg, ds):
    coord, sdf_label, origin, ts, normal_label, sem_label, weight = ds.get_batch()
    bs = cfg.bs
    assert coord.shape == (bs, 3) and sdf_label.shape == (bs,) and origin.shape == (bs, 3) and ts.shape == (bs,)
    assert weight.shape == (bs,) and normal_label is None and sem_label is None
    assert all(t.dtype == torch.float32 and t.is_cuda for t in (coord, sdf_label, origin, ts, weight))
    pool = {r.tobytes() for r in _rows(ds.coord_pool, ds.sdf_label_pool, ds.origin_pool, ds.time_pool, ds.weight_pool)}
    batch = _rows(coord, sdf_label, origin, ts, weight)
    assert all(r.tobytes() in pool for r in batch)
    assert len({r.tobytes() for r in batch}) > bs // 2  # (a draw with replacement from a pool much larger than the batch)


def _check_surface_samples(cfg, ds, frames, want, e_coord):
    """every coord[weight > 0] lies within surface_sample_range_m * scale (+ the sampler's fp32 distance and the fp32 cast of the
    point) of the down-sampled point of its ray — sample i * S + j belongs to point i of its frame"""
    S, ns = ds.sampler.S, ds.sampler.ns
    coord, weight, time = ds.coord_pool.double().cpu().numpy(), ds.weight_pool.cpu().numpy(), ds.time_pool.cpu().numpy()
    at = 0
    for f in frames:
        pts = want[f]["world"] * cfg.scale
        m = len(pts)
        c = coord[at:at + m * S].reshape(m, S, 3)
        assert np.all(time[at:at + m * S] == f) and np.all(weight[at:at + m * S].reshape(m, S)[:, :ns] > 0)
        assert np.all(weight[at:at + m * S].reshape(m, S)[:, ns:] < 0)
        d = np.linalg.norm(c[:, :ns] - pts[:, None, :], axis=2).max()
        bound = cfg.surface_sample_range_m * cfg.scale + e_coord + 2.0 ** -23
        print("frame %d: surface samples within %.6e of their points (bound %.6e)" % (f, d, bound))
        assert d <= bound
        at += m * S
    assert at == len(coord)


def test_batch_mode_end_to_end_trains_and_meshes(drive, tmp_path):
    from shine_mapping_amd import Decoder, StepOptions
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.mesher import Mesher
    from shine_mapping_amd.optim import setup_optimizer

    e_coord = BOUND_FACTOR * load_golden("frame_sampler")["e_ref"]["coord"]
    cfg, octree, ds = _dataset(drive)
    want = _oracle_frames(drive, cfg, ds)
    S = ds.sampler.S
    total = 0
    for f in range(drive.frames):
        ds.process_frame(f, incremental_on=False)
        total += S * len(want[f]["sensor"])
        assert len(ds) == total == ds.coord_pool.shape[0] == ds.weight_pool.shape[0] == ds.origin_pool.shape[0]
    print("batch mode: %d samples from %d frames" % (total, drive.frames))
    assert ds.sample_depth_pool.shape[0] == 0 and ds.ray_depth_pool.shape[0] == 0  # (kept only with ray_loss)
    assert len(octree.hier_features) == cfg.tree_level_feat and all(p.shape[0] > 100 for p in octree.hier_features)
    _check_surface_samples(cfg, ds, range(drive.frames), want, e_coord)
    _check_batch(cfg, ds)
    # 200 steps of the fused loop on the dataset's sorted pool
    torch.manual_seed(2)
    dec = Decoder(cfg).cuda()
    opt = setup_optimizer(cfg, list(octree.parameters()), dec.fused_params())
    pool = ds.sorted_pool()
    assert pool is ds.sorted_pool() and pool.size == total
    it = GraphedIteration(octree, dec, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid, loss_reduction="mean"), cfg.bs)
    losses = [float(it()) for _ in range(200)]
    torch.cuda.synchronize()
    print("fused loop: loss %.5f -> %.5f" % (losses[0], losses[-1]))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    cfg.min_cluster_vertices = 10
    mesh = Mesher(cfg, octree, dec).recon_bbx_mesh(ds.map_bbx, 0.4, str(tmp_path / "mesh.ply"), None, estimate_normal=False,
                                                   filter_isolated_mesh=False)
    print("mesh: %d vertices, %d triangles" % (len(np.asarray(mesh.vertices)), len(np.asarray(mesh.triangles))))
    assert len(np.asarray(mesh.triangles)) > 0 and os.path.getsize(str(tmp_path / "mesh.ply")) > 0
    ds.write_merged_pc(str(tmp_path / "merged.ply"))
    from shine_mapping_amd.evaluation import read_ply

    assert read_ply(str(tmp_path / "merged.ply"))["vertices"].shape == (len(ds.map_down_pc), 3)


def test_incremental_mode_end_to_end(drive):
    from shine_mapping_amd import Decoder, StepOptions
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.optim import setup_optimizer

    e_coord = BOUND_FACTOR * load_golden("frame_sampler")["e_ref"]["coord"]
    cfg, octree, ds = _dataset(drive, loss_reduction="mean", lambda_forget=0.0)
    want = _oracle_frames(drive, cfg, ds)
    S = ds.sampler.S
    rows = []
    for f in range(drive.frames):
        ds.process_frame(f, incremental_on=True)
        assert len(ds) == S * len(want[f]["sensor"]) == ds.coord_pool.shape[0] == ds.time_pool.shape[0]  # the last frame only
        rows.append(sum(int(p.shape[0]) for p in octree.hier_features))
        _check_surface_samples(cfg, ds, [f], want, e_coord)
    print("incremental mode: feature rows per frame", rows)
    assert rows[-1] > rows[0] > 0
    _check_batch(cfg, ds)
    torch.manual_seed(2)
    dec = Decoder(cfg).cuda()
    opt = setup_optimizer(cfg, list(octree.parameters()), dec.fused_params())
    it = GraphedIteration(octree, dec, ds.sorted_pool(), opt, StepOptions(sigma=cfg.sigma_sigmoid, loss_reduction="mean"), cfg.bs)
    losses = [float(it()) for _ in range(200)]
    print("fused loop on the last frame: loss %.5f -> %.5f" % (losses[0], losses[-1]))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


def test_window_replay_keeps_only_samples_inside_the_window(drive):
    cfg, octree, ds = _dataset(drive, window_replay_on=True, window_radius=12.0)
    want = _oracle_frames(drive, cfg, ds)
    S = ds.sampler.S
    for f in range(drive.frames):
        ds.process_frame(f)
    last = drive.frames - 1
    n_all = S * sum(len(w["sensor"]) for w in want)
    coord, time = ds.coord_pool, ds.time_pool
    assert len(ds) == coord.shape[0] == ds.sdf_label_pool.shape[0] == ds.weight_pool.shape[0] == ds.origin_pool.shape[0]
    print("window replay: %d of %d samples kept; frames present %s" % (len(ds), n_all, torch.unique(time).tolist()))
    assert len(ds) < n_all and int((time == last).sum()) == S * len(want[last]["sensor"])
    assert torch.unique(time).numel() >= 2  # the drive is longer than the window, but neighbouring frames overlap
    origin_last = torch.tensor((ds.poses_ref[last][:3, 3] * cfg.scale).astype(np.float32), device="cuda")
    old = time < last
    assert bool(((coord[old] - origin_last).norm(2, dim=-1) < cfg.window_radius * cfg.scale).all())
    # the arrays stayed aligned: every sample still carries the origin of its own frame, and its label sign matches its weight slot
    for f in torch.unique(time).tolist():
        o = torch.tensor((ds.poses_ref[int(f)][:3, 3] * cfg.scale).astype(np.float32), device="cuda")
        assert bool((ds.origin_pool[time == f] == o).all())
    surf = ds.weight_pool > 0
    assert float(ds.sdf_label_pool[surf].abs().max()) <= cfg.surface_sample_range_m * cfg.scale * (1 + 1e-6)
    # and something the window dropped really was outside
    assert int((time == 0).sum()) < S * len(want[0]["sensor"])


def test_ray_mode_pools_and_batches(drive):
    cfg, octree, ds = _dataset(drive, ray_loss=True, bs=128)
    want = _oracle_frames(drive, cfg, ds)
    S = ds.sampler.S
    for f in range(2):
        ds.process_frame(f)
    rays = len(want[0]["sensor"]) + len(want[1]["sensor"])
    assert len(ds) == rays == ds.ray_depth_pool.shape[0] and ds.sample_depth_pool.shape[0] == rays * S == ds.coord_pool.shape[0]
    assert ds.sdf_label_pool.shape[0] == 0 and ds.origin_pool.shape[0] == 0
    coord, sample_depth, ray_depth, normal_label, sem_label, weight = ds.get_batch()
    R = ds.ray_sample_count
    assert coord.shape == (128 * R, 3) and sample_depth.shape == (128 * R,) and ray_depth.shape == (128,) and weight.shape == (128 * R,)
    assert normal_label is None and sem_label is None
    # a ray's samples: depth of the surface samples within the sampling range of the ray's depth
    d = sample_depth.view(128, R)[:, :ds.sampler.ns] - ray_depth[:, None]
    assert float(d.abs().max()) <= cfg.surface_sample_range_m * (1 + 1e-4)
