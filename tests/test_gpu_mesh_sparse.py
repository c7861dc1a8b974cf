"""GPU: marching cubes over a brick set (csrc/shine_mc_sparse.hip) against the dense marching cubes on the dense grid the bricks
stand for — bit for bit, in the same order — and the Mesher's brick routes (recon_octree_mesh / recon_bbx_mesh with sparse=True)
against its dense routes, up to a map that spans the world cube."""
import numpy as np
import pytest
import torch

import mc_sparse_oracle as so
from test_gpu_mesh import _Box, _cross_zero, _mesher, _smooth, _T, _tiny

pytestmark = pytest.mark.gpu


def _sparse(values, mask, origins, shape, level=0.0):
    from shine_mapping_amd.mesher import marching_cubes_sparse

    v, f = marching_cubes_sparse(torch.as_tensor(values).cuda(), None if mask is None else torch.as_tensor(mask).cuda(), origins,
                                 shape, level)
    torch.cuda.synchronize()
    return v, f


def _dense(sdf, mask, level=0.0):
    from shine_mapping_amd.mesher import marching_cubes

    return marching_cubes(torch.as_tensor(sdf).cuda(), None if mask is None else torch.as_tensor(mask).cuda(), level)


def _equals_the_dense_twin(values, mask, origins, shape, level=0.0):
    sdf, msk = so.dense_twin(values, mask, origins, shape)
    v, f = _sparse(values, mask, origins, shape, level)
    dv, df = _dense(sdf, msk, level)
    print("%d bricks of %d^3 in %s, level %g: %d vertices, %d faces (dense twin: %d, %d)"
          % (len(origins), values.shape[1], tuple(shape), level, len(v), len(f), len(dv), len(df)))
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    assert torch.equal(f, df)
    assert torch.equal(v, dv)
    v2, f2 = _sparse(values, mask, origins, shape, level)
    assert torch.equal(v, v2) and torch.equal(f, f2), "two runs must be bit-identical"
    return v, f


@pytest.mark.parametrize("B", [1, 3, 8, 12])
@pytest.mark.parametrize("shape", [(96, 80, 72), (61, 45, 50)])
def test_random_smooth_fields_with_dropped_bricks_equal_the_dense_twin(shape, B):
    sdf = _smooth(shape, sum(shape) + B)
    rng = np.random.default_rng(B)
    values, _, origins = so.cut(sdf, None, B, keep_fraction=0.6, seed=B)
    v, f = _equals_the_dense_twin(values, None, origins, shape)  # no mask: every cube a brick covers
    assert len(f) > 100
    _equals_the_dense_twin(values, None, origins, shape, level=0.13)  # (uncovered points are 0: out, and not on the level)
    _equals_the_dense_twin(values, None, origins, shape, level=-0.2)  # (uncovered points are in)
    mask = rng.random(shape) < 0.7
    values, bmask, origins = so.cut(sdf, mask, B, keep_fraction=0.6, seed=B + 100)
    v, f = _equals_the_dense_twin(values, bmask, origins, shape)
    assert len(f) > 100
    _equals_the_dense_twin(values, bmask, origins, shape, level=0.13)


def test_the_largest_brick_edge():
    shape = (70, 64, 40)
    sdf = _smooth(shape, 11)
    values, bmask, origins = so.cut(sdf, np.random.default_rng(3).random(shape) < 0.8, 32, keep_fraction=0.7, seed=4)
    assert 2 <= len(origins) < 12
    v, f = _equals_the_dense_twin(values, bmask, origins, shape)
    assert len(f) > 100
    _equals_the_dense_twin(values, None, origins, shape, level=0.1)


def test_values_on_the_level_at_brick_faces_and_corner_vertices_of_uncovered_points():
    """a field quantised to quarters has whole sheets of exact zeros; with bricks dropped next to them, edges collapse onto
    corner vertices that belong to points NO brick covers (their value 0 is the level)"""
    shape, B = (40, 36, 44), 4
    sdf = np.round(_smooth(shape, 4) * 4).astype(np.float32) / 4
    assert (sdf == 0).sum() > 100
    for ax in range(3):  # exact zeros ON brick faces
        sl = [slice(None)] * 3
        sl[ax] = slice(0, None, B)
        assert (sdf[tuple(sl)] == 0).sum() > 10
    values, _, origins = so.cut(sdf, None, B, keep_fraction=0.6, seed=2)
    v, f = _equals_the_dense_twin(values, None, origins, shape)
    fn = f.cpu().numpy()
    assert ((fn[:, 0] != fn[:, 1]) & (fn[:, 1] != fn[:, 2]) & (fn[:, 0] != fn[:, 2])).all()
    vn = v.cpu().numpy()
    assert len(np.unique(vn, axis=0)) == len(vn)
    whole = vn[(vn == np.round(vn)).all(1)].astype(np.int64)  # corner vertices
    _, covered = so.dense_twin(values, None, origins, shape)
    outside = ~covered[whole[:, 0], whole[:, 1], whole[:, 2]]
    print("%d corner vertices, %d of them at points no brick covers" % (len(whole), outside.sum()))
    assert outside.sum() > 0
    mask = np.random.default_rng(5).random(shape) < 0.7
    values, bmask, origins = so.cut(sdf, mask, B, keep_fraction=0.6, seed=3)
    _equals_the_dense_twin(values, bmask, origins, shape)


@pytest.mark.parametrize("B", [1, 3])
def test_the_two_cube_grid_as_bricks(B):
    """test_gpu_mesh's (2, 2, 3) grid with every cube processed: as twelve bricks of one point each, where every value a cube
    reads besides its lowest corner comes from the apron, and as one brick of 3^3 that reaches beyond the grid on x and y"""
    shape = (2, 2, 3)
    values, bmask, origins = so.cut(_tiny(shape), np.ones(shape, bool), B)
    assert len(origins) == (12 if B == 1 else 1)
    v, f = _equals_the_dense_twin(values, bmask, origins, shape)
    assert (len(v), len(f)) == (12, 8)


def test_empty_surface_single_brick_and_no_bricks():
    from shine_mapping_amd.mesher import marching_cubes_sparse

    shape, B = (30, 30, 30), 12
    ones, _, origins = so.cut(np.ones(shape, np.float32), None, B)
    # (level 2: the uncovered zeros and the ones are all out; at level 0 the rim of the brick set is a surface)
    v, f = _sparse(ones, None, origins, shape, level=2.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = _sparse(ones, np.zeros(ones.shape, bool), origins, shape)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = marching_cubes_sparse(torch.zeros((0, B, B, B), device="cuda"), None, np.zeros((0, 3), np.int64), shape)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.is_cuda
    # a single brick: alone in its grid, and inside a larger one (where its upper faces meet uncovered zeros)
    sdf = _smooth((B, B, B), 8)
    one = sdf[None]
    v, f = _equals_the_dense_twin(one, None, np.array([[0, 0, 0]]), (B, B, B))
    assert len(f) > 20
    assert torch.equal(v, _dense(sdf, None)[0])
    _equals_the_dense_twin(one, None, np.array([[12, 12, 0]]), shape)
    _equals_the_dense_twin(one, None, np.array([[24, 12, 24]]), shape, level=0.05)  # (reaches beyond the grid on x and z)


# ---------------------------------------------------------------------------------------------------------------- the Mesher
def _mesh_arrays(mesh):
    return np.asarray(mesh.triangles), np.asarray(mesh.vertices), np.asarray(mesh.vertex_normals)


def _routes_agree(call, tmp_path, tag):
    """call(sparse, path) -> mesh: the brick route and the dense route give the same arrays and the same file"""
    pd, ps = str(tmp_path / (tag + "_dense.ply")), str(tmp_path / (tag + "_sparse.ply"))
    dense = _mesh_arrays(call(False, pd))
    sparse = _mesh_arrays(call(True, ps))
    print("%s: %d triangles, %d vertices" % (tag, len(dense[0]), len(dense[1])))
    for a, b in zip(dense, sparse):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert open(pd, "rb").read() == open(ps, "rb").read()
    return dense


def test_recon_octree_mesh_brick_route_equals_the_dense_route_on_a_fixture(tmp_path):
    fx, m = _mesher("mesh_query_L3")
    coord, _, _ = m.get_query_from_bbx(_Box(fx["lo"], fx["hi"]), fx["voxel"])
    _cross_zero(m, coord)
    m.global_transform = _T()
    top = m.octree.max_level - m.octree.featured_level_num + 1
    for level, res in ((top, 0.1), (top, 0.07), (m.octree.max_level, 0.1)):
        for filt in (False, True):
            tri, _, nrm = _routes_agree(lambda sp, path: m.recon_octree_mesh(level, res, path, None, filter_isolated_mesh=filt,
                                                                             sparse=sp), tmp_path, "o%d_%g_%d" % (level, res, filt))
            assert len(nrm) > 0 and (filt or len(tri) > 0)
    tri, _, _ = _routes_agree(lambda sp, path: m.recon_octree_mesh(top, 0.1, path, None, estimate_normal=False,
                                                                   filter_isolated_mesh=False, sparse=sp), tmp_path, "plain")
    assert len(tri) > 0


@pytest.mark.parametrize("name", ["mesh_query_L3", "mesh_query_L4"])
def test_recon_bbx_mesh_brick_route_equals_the_dense_route_on_a_fixture(name, tmp_path):
    fx, m = _mesher(name)
    box, vox = _Box(fx["lo"], fx["hi"]), fx["voxel"]
    coord, _, _ = m.get_query_from_bbx(box, vox)
    _cross_zero(m, coord)
    m.global_transform = _T()
    for filt in (False, True):
        tri, _, nrm = _routes_agree(lambda sp, path: m.recon_bbx_mesh(box, vox, path, None, filter_isolated_mesh=filt, sparse=sp),
                                    tmp_path, "b%d" % filt)
        assert len(nrm) > 0 and (filt or len(tri) > 0)
    _routes_agree(lambda sp, path: m.recon_bbx_mesh(box, vox * 0.5, path, None, filter_isolated_mesh=False, sparse=sp), tmp_path, "half")
    # what the brick route cannot do
    with pytest.raises(ValueError, match="save_map.*sparse"):
        m.recon_bbx_mesh(box, vox, str(tmp_path / "x.ply"), str(tmp_path / "map.ply"), save_map=True, sparse=True)
    m.config.mc_mask_on = False
    with pytest.raises(ValueError, match="mc_mask_on"):
        m.recon_bbx_mesh(box, vox, str(tmp_path / "x.ply"), None, sparse=True)
    m.recon_bbx_mesh(box, vox, str(tmp_path / "x.ply"), None)  # (None stays dense there)


def test_both_routes_on_a_trained_synthetic_maicity_map(tmp_path):
    from shine_mapping_amd import Decoder, FeatureOctree, StepOptions, synth
    from shine_mapping_amd.dataset import LiDARDataset
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.mesher import Mesher
    from shine_mapping_amd.optim import setup_optimizer

    drive = synth.write_kitti_drive(str(tmp_path / "drive"), synth.make_config("maicity", device="cuda"), frames=6, beams=32,
                                    azimuths=180, device="cpu")
    cfg = synth.dataset_config("maicity", drive)
    torch.manual_seed(1)
    octree = FeatureOctree(cfg)
    ds = LiDARDataset(cfg, octree)
    for f in range(drive.frames):
        ds.process_frame(f, incremental_on=False)
    torch.manual_seed(2)
    dec = Decoder(cfg).cuda()
    opt = setup_optimizer(cfg, list(octree.parameters()), dec.fused_params())
    it = GraphedIteration(octree, dec, ds.sorted_pool(), opt, StepOptions(sigma=cfg.sigma_sigmoid, loss_reduction="mean"), cfg.bs)
    for _ in range(300):
        it()
    torch.cuda.synchronize()
    cfg.mc_mask_on = True
    cfg.min_cluster_vertices = 50
    m = Mesher(cfg, octree, dec)
    top = octree.max_level - octree.featured_level_num + 1
    for filt in (False, True):
        tri, _, _ = _routes_agree(lambda sp, path: m.recon_octree_mesh(top, 0.1, path, None, filter_isolated_mesh=filt, sparse=sp),
                                  tmp_path, "oct%d" % filt)
        assert filt or len(tri) > 1000
        tri, _, _ = _routes_agree(lambda sp, path: m.recon_bbx_mesh(ds.map_bbx, 0.2, path, None, filter_isolated_mesh=filt, sparse=sp),
                                  tmp_path, "box%d" % filt)
        assert filt or len(tri) > 1000


def _two_patch_map():
    from shine_mapping_amd import Decoder, FeatureOctree, synth
    from shine_mapping_amd.mesher import Mesher

    cfg = synth.make_config("maicity", device="cuda")
    assert cfg.tree_level_world == 12
    cfg.mc_mask_on = True
    torch.manual_seed(3)
    octree = FeatureOctree(cfg)
    dec = Decoder(cfg).cuda()
    g = torch.Generator().manual_seed(5)
    half = torch.tensor([0.012, 0.012, 0.004])  # ~ 10 m x 10 m x 3 m at this scale

    def patch(centre):
        return (torch.rand(4000, 3, generator=g) * 2 - 1) * half + torch.tensor(centre)

    pts = torch.cat([patch([-0.97, -0.96, -0.95]), patch([0.96, 0.95, 0.97])]).float().cuda()
    octree.update(pts, False)
    return cfg, octree, dec, Mesher(cfg, octree, dec)


def test_a_map_that_spans_the_world_cube(tmp_path):
    """two small patches near opposite corners of the world cube: the dense grid over their bounding box takes terabytes, the
    bricks a few MB, and the mesh is patch A's dense mesh followed by patch B's (they are separated in x)"""
    from shine_mapping_amd.mesher import dense_grid_bytes, marching_cubes, marching_cubes_sparse

    cfg, octree, dec, m = _two_patch_map()
    level, res = octree.max_level - octree.featured_level_num + 1, 0.1
    lay = m.octree_grid_layout(level, res)
    assert dense_grid_bytes(lay[4]) > 1e12, lay[4]
    values, mask, _, _, _, _ = m.octree_bricks_device(level, res)
    with torch.no_grad():  # (as _cross_zero: the untrained decoder's level 0 must cross the masked points)
        dec.fused_params()[5].add_(float(values[mask.bool()].median()))
    with pytest.raises(MemoryError):
        m.recon_octree_mesh(level, res, str(tmp_path / "d.ply"), None, sparse=False)
    values, mask, origins, shape, voxel, origin = m.octree_bricks_device(level, res)
    B = values.shape[1]
    print("%d bricks of %d^3 in a virtual grid %s" % (len(origins), B, shape))
    assert 200 <= len(origins) <= 4000 and tuple(shape) == tuple(int(v) for v in lay[4])

    # the expected mesh: dense marching cubes of a window around each patch (a margin of one cell where the grid goes on)
    vn, mn = values.cpu().numpy(), mask.cpu().numpy().astype(bool)
    in_a = origins[:, 0] < shape[0] // 2
    assert 0 < in_a.sum() < len(origins)
    assert origins[in_a, 0].max() + B + 1 < origins[~in_a, 0].min()  # separated in x: A's rows come first in the dense order
    ev, ef, base = [], [], 0
    for sel in (in_a, ~in_a):
        lo = np.maximum(origins[sel].min(0) - 1, 0)
        hi = np.minimum(origins[sel].max(0) + B + 1, np.asarray(shape))
        sdf, msk = so.dense_twin(vn[sel], mn[sel], origins[sel] - lo, hi - lo)
        wv, wf = marching_cubes(torch.as_tensor(sdf).cuda(), torch.as_tensor(msk).cuda(), 0.0)
        assert len(wf) > 100
        ev.append(wv + torch.as_tensor(lo, dtype=torch.float32, device="cuda"))
        ef.append(wf + base)
        base += len(wv)
    ev, ef = torch.cat(ev), torch.cat(ef)
    v, f = marching_cubes_sparse(values, mask, origins, shape, 0.0)
    assert torch.equal(f, ef)
    # fl(x + t) against fl(fl(x_window + t) + offset): one ulp of the largest coordinate (fp32)
    ulp = float(np.spacing(np.float32(max(shape))))
    err = (v - ev).abs().max().item()
    print("vertices: max |sparse - (window + offset)| = %.3e index units (bound: one fp32 ulp at %d = %.3e)" % (err, max(shape), ulp))
    assert v.shape == ev.shape and err <= ulp

    # the drivers' call (no keyword) and sparse=True: the same mesh, within 1 GiB
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    mesh = m.recon_octree_mesh(level, res, str(tmp_path / "n.ply"), None, estimate_normal=False, filter_isolated_mesh=False)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("peak device memory over recon_octree_mesh: %.1f MB" % (peak / 1e6))
    assert peak < 2 ** 30
    assert np.array_equal(np.asarray(mesh.triangles), f.cpu().numpy())
    want = np.asarray(origin, np.float64) + v.double().cpu().numpy() * voxel
    assert np.abs(np.asarray(mesh.vertices) - want).max() <= 1e-9
    full = m.recon_octree_mesh(level, res, str(tmp_path / "n2.ply"), None)
    forced = m.recon_octree_mesh(level, res, str(tmp_path / "s.ply"), None, sparse=True)
    for a, b in zip(_mesh_arrays(full), _mesh_arrays(forced)):
        assert np.array_equal(a, b)
    assert open(str(tmp_path / "n2.ply"), "rb").read() == open(str(tmp_path / "s.ply"), "rb").read()
    assert len(np.asarray(full.vertex_normals)) == len(want)


def test_default_stays_on_the_dense_route_where_it_fits(tmp_path, monkeypatch):
    from shine_mapping_amd import _lib

    fx, m = _mesher("mesh_query_L3")
    box, vox = _Box(fx["lo"], fx["hi"]), fx["voxel"]
    coord, _, _ = m.get_query_from_bbx(box, vox)
    _cross_zero(m, coord)
    lib = _lib.lib()
    calls = {"count": 0, "emit": 0}
    real_count, real_emit = lib.shine_mc_sparse_count, lib.shine_mc_sparse_emit

    def count(*a):
        calls["count"] += 1
        return real_count(*a)

    def emit(*a):
        calls["emit"] += 1
        return real_emit(*a)

    monkeypatch.setattr(lib, "shine_mc_sparse_count", count)
    monkeypatch.setattr(lib, "shine_mc_sparse_emit", emit)
    level = m.octree.max_level - m.octree.featured_level_num + 1
    runs = {}
    for key, kw in (("default", {}), ("none", {"sparse": None}), ("dense", {"sparse": False})):
        po, pb = str(tmp_path / (key + "_o.ply")), str(tmp_path / (key + "_b.ply"))
        o = m.recon_octree_mesh(level, 0.1, po, None, **kw)
        b = m.recon_bbx_mesh(box, vox, pb, str(tmp_path / (key + "_map.ply")), save_map=True, **kw)
        runs[key] = (_mesh_arrays(o), _mesh_arrays(b), open(po, "rb").read(), open(pb, "rb").read(),
                     open(str(tmp_path / (key + "_map.ply")), "rb").read())
    assert calls == {"count": 0, "emit": 0}
    for key in ("default", "none"):
        for a, b in zip(runs[key][0] + runs[key][1], runs["dense"][0] + runs["dense"][1]):
            assert np.array_equal(a, b)
        assert runs[key][2:] == runs["dense"][2:]
    assert len(runs["dense"][0][0]) > 0 and len(runs["dense"][1][0]) > 0
    m.recon_octree_mesh(level, 0.1, str(tmp_path / "s.ply"), None, sparse=True)
    assert calls["count"] == 2 and calls["emit"] == 2  # (each: the size query, then the call)
