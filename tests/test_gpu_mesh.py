"""GPU: device marching cubes (csrc/shine_mc.hip) against the numpy oracle with the same rules (tests/mc_oracle.py), analytic
surfaces at 256^3, determinism, 64-bit grid indexing, vertex normals and the cluster filter (csrc/shine_mesh.hip), and the
Mesher's recon_bbx_mesh / recon_octree_mesh / estimate_sem on fixture and synthetic maps."""
import numpy as np
import pytest
import torch

import mc_oracle as mo
import mesh_post_cases as mp
from conftest import load_golden, product_from_golden

pytestmark = pytest.mark.gpu


def _mc(sdf, mask=None, level=0.0):
    from shine_mapping_amd.mesher import marching_cubes

    v, f = marching_cubes(torch.as_tensor(sdf).cuda(), None if mask is None else torch.as_tensor(mask).cuda(), level)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


def _same(sdf, mask=None, level=0.0):
    v, f = _mc(sdf, mask, level)
    rv, rf = mo.marching_cubes(sdf, mask, level)
    assert f.shape == rf.shape and np.array_equal(f, rf)
    assert v.shape == rv.shape and (len(v) == 0 or np.abs(v - rv).max() <= 1e-6)
    return v, f


def _smooth(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, 1) + tuple(s // 4 + 2 for s in shape), generator=g)
    return torch.nn.functional.interpolate(x, size=shape, mode="trilinear", align_corners=True)[0, 0].numpy().astype(np.float32)


@pytest.mark.parametrize("shape", [(17, 23, 29), (40, 33, 70), (3, 64, 1030)])
def test_random_smooth_fields_match_the_oracle(shape):
    sdf = _smooth(shape, sum(shape))
    v, f = _same(sdf)
    assert len(f) > 100
    _same(sdf, level=0.13)


def test_exact_zeros_match_the_oracle_without_degenerate_faces():
    X, Y, Z = 19, 21, 40
    z = np.arange(Z, dtype=np.float32)
    for k in (0, 7, 39):
        sdf = np.broadcast_to(np.float32(k) - z, (X, Y, Z)).copy()
        v, f = _same(sdf)
        assert len(np.unique(v, axis=0)) == len(v)
        assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    # zeros scattered over a rough field: collapsed corners of every kind
    rng = np.random.default_rng(1)
    sdf = np.round(_smooth((30, 31, 45), 4) * 4).astype(np.float32) / 4
    assert (sdf == 0).sum() > 100
    v, f = _same(sdf)
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    assert len(np.unique(v, axis=0)) == len(v)
    del rng


def test_masks_match_the_oracle():
    shape = (36, 41, 67)
    sdf = _smooth(shape, 9)
    rng = np.random.default_rng(2)
    _same(sdf, rng.random(shape) < 0.6)
    v, f = _same(sdf, np.zeros(shape, bool))
    assert len(v) == 0 and len(f) == 0
    half = np.zeros(shape, bool)
    half[:, :, :30] = True
    _same(sdf, half)


def _tiny(shape):
    return np.random.default_rng(0).standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("shape,counts", [((2, 2, 2), (6, 4)), ((2, 2, 3), (12, 8)), ((1, 7, 7), (0, 0)), ((5, 1, 9), (0, 0)),
                                          ((2, 3, 1), (0, 0))])
def test_smallest_extents_match_the_oracle(shape, counts):
    """one cube, two cubes, and grids too thin to hold a cube, every cube processed: each point lies on the grid's border, so the
    only thing that keeps the classify rules from reading a neighbour outside the grid is that no processed cube lies there"""
    v, f = _same(_tiny(shape), np.ones(shape, bool))
    assert (len(v), len(f)) == counts


def test_empty_surface_and_out_of_range_level():
    sdf = _smooth((20, 20, 20), 5)
    for lev in (float(sdf.max()) + 1, float(sdf.min()) - 1):
        v, f = _mc(sdf, level=lev)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = _mc(np.ones((8, 8, 8), np.float32))
    assert v.shape == (0, 3) and f.shape == (0, 3)


def _analytic(kind, n=256):
    ax = torch.arange(n, dtype=torch.float64, device="cuda")
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    s = n / 256.0  # (the surfaces are laid out for 256^3 and shrink with a smaller grid: the same numbers at n = 256)
    c = (127.3 * s, 128.6 * s, 126.9 * s)
    if kind == "sphere":
        r = 100.0 * s
        d = torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        return (r - d).float(), r
    R, r = 80.0 * s, 30.0 * s
    q = torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R
    return (r - torch.sqrt(q ** 2 + (z - c[2]) ** 2)).float(), (R, r)


def _topology(f):
    f = f.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    kd = d[:, 0] * (1 << 31) + d[:, 1]
    ku = np.minimum(d[:, 0], d[:, 1]) * (1 << 31) + np.maximum(d[:, 0], d[:, 1])
    _, cu = np.unique(ku, return_counts=True)
    _, cd = np.unique(kd, return_counts=True)
    return cu, cd, len(np.unique(f)) - len(cu) + len(f)


@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_analytic_surfaces_at_256(kind):
    from shine_mapping_amd.mesher import marching_cubes

    sdf, par = _analytic(kind)
    v, f = marching_cubes(sdf)
    v2, f2 = marching_cubes(sdf)
    assert torch.equal(v, v2) and torch.equal(f, f2), "two runs must be bit-identical"
    v, f = v.cpu().numpy().astype(np.float64), f.cpu().numpy()
    cu, cd, chi = _topology(f)
    assert (cu == 2).all() and cd.max() == 1, "watertight and consistently oriented"
    c = np.array([127.3, 128.6, 126.9])
    if kind == "sphere":
        assert chi == 2
        vol = np.einsum("ij,ij->i", v[f[:, 0]] - c, np.cross(v[f[:, 1]] - c, v[f[:, 2]] - c)).sum() / 6
        assert vol > 0 and abs(vol / (4 / 3 * np.pi * par ** 3) - 1) <= 0.01, vol
        err = np.abs(np.linalg.norm(v - c, axis=1) - par).max()
    else:
        assert chi == 0
        R, r = par
        q = np.sqrt((v[:, 0] - c[0]) ** 2 + (v[:, 1] - c[1]) ** 2) - R
        err = np.abs(np.sqrt(q ** 2 + (v[:, 2] - c[2]) ** 2) - r).max()
    assert err <= 0.02, err


def test_grid_beyond_2_to_the_31_points():
    from shine_mapping_amd.mesher import marching_cubes

    n, b = 1300, 25
    o = n - b
    ax = torch.arange(b, dtype=torch.float32, device="cuda")
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    small = (8.0 - torch.sqrt((x - 12.2) ** 2 + (y - 11.7) ** 2 + (z - 12.4) ** 2)).contiguous()
    vs, fs = marching_cubes(small)
    big = torch.full((n, n, n), -5.0, dtype=torch.float32, device="cuda")
    assert big.numel() > 2 ** 31
    big[o:, o:, o:] = small
    vb, fb = marching_cubes(big)
    del big
    assert len(fs) > 500 and torch.equal(fb, fs)
    assert (vb - (vs + o)).abs().max().item() <= 2e-4


def test_vertex_normals_match_the_area_weighted_oracle():
    from shine_mapping_amd.mesher import marching_cubes, vertex_normals_device

    sdf, _ = _analytic("torus", 96)
    v, f = marching_cubes(sdf)
    assert len(f) > 10000  # (the whole torus lies inside the grid)
    vw = v.double() * 0.1 + torch.tensor([3.0, -2.0, 1.0], dtype=torch.float64, device="cuda")
    vw = torch.cat([vw, torch.zeros(1, 3, dtype=torch.float64, device="cuda")])  # one vertex without faces: normal 0
    n = vertex_normals_device(vw, f)
    # |n - n_ref| <= 8 (k_v + 8) 2^-53 cond_v against the 80-bit oracle (mesh_post_cases.check_normals); the vertex without faces
    # is the only one the bound does not cover, and it must be exactly zero
    ref, kv, cond = mo.vertex_normals_ext(vw.cpu().numpy(), f.cpu().numpy())
    ratio = mp.check_normals(n.cpu().numpy(), ref, kv, cond, cancel=(len(vw) - 1,))
    print("torus: max |n - n_ref| / bound = %.3g" % ratio)
    assert (n[-1] == 0).all()
    assert torch.equal(n, vertex_normals_device(vw, f))


def test_cluster_filter_keeps_the_large_component():
    from shine_mapping_amd.mesher import cluster_filter_device, marching_cubes

    n = 64
    ax = torch.arange(n, dtype=torch.float32, device="cuda")
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    big = 20.0 - torch.sqrt((x - 30.3) ** 2 + (y - 31.1) ** 2 + (z - 30.7) ** 2)
    tiny = 1.6 - torch.sqrt((x - 58.2) ** 2 + (y - 57.6) ** 2 + (z - 58.4) ** 2)
    mid = 4.0 - torch.sqrt((x - 6.4) ** 2 + (y - 6.3) ** 2 + (z - 57.5) ** 2)
    v, f = marching_cubes(torch.maximum(torch.maximum(big, tiny), mid))
    fn = f.cpu().numpy()
    cid, cnt = mo.triangle_clusters(fn)
    assert len(cnt) == 3 and cnt.min() < 300 <= cnt.max()
    kept, clusters = cluster_filter_device(f, 300, return_clusters=True)
    assert np.array_equal(clusters.cpu().numpy(), cid)
    assert np.array_equal(kept.cpu().numpy(), fn[cnt[cid] >= 300])
    thr = int(np.sort(cnt)[1])
    assert np.array_equal(cluster_filter_device(f, thr).cpu().numpy(), fn[cnt[cid] >= thr])
    assert cluster_filter_device(f, 1).shape == f.shape


# ---------------------------------------------------------------------------------------------------------------- the Mesher
class _Box:
    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def get_min_bound(self):
        return np.asarray(self.lo, dtype=np.float64)

    def get_max_bound(self):
        return np.asarray(self.hi, dtype=np.float64)


def _mesher(fx_name):
    from shine_mapping_amd.mesher import Mesher

    fx = load_golden(fx_name)
    cfg, octree, dec = product_from_golden(load_golden(fx["source"]))
    cfg.mc_vis_level = fx["mc_vis_level"]
    cfg.pad_voxel = fx["pad_voxel"]
    cfg.mc_mask_on = True
    cfg.min_cluster_vertices = 20
    return fx, Mesher(cfg, octree, dec.cuda(), None)


def _cross_zero(m, coord):
    """Shift the decoder's output bias so that the mesher's (negated) SDF changes sign inside the queried region: the fixture
    and synthetic decoders are barely trained, and their level 0 may not cross the masked points at all."""
    sdf, _, mask = m.query_points(coord, coord.shape[0] + 1, True, False, True)
    med = float(np.median(sdf[mask.astype(bool)]))
    with torch.no_grad():
        m.geo_decoder.fused_params()[5].add_(med)  # sdf = -decoder: the bias moves it by -med


def _T():
    T = np.eye(4)
    a = 0.3
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [10.0, -4.0, 2.5]
    return T


@pytest.mark.parametrize("name", ["mesh_query_L3", "mesh_query_L4"])
def test_recon_bbx_mesh_matches_the_oracle(name, tmp_path):
    fx, m = _mesher(name)
    box = _Box(fx["lo"], fx["hi"])
    vox = fx["voxel"]
    coord, num, origin = m.get_query_from_bbx(box, vox)
    _cross_zero(m, coord)
    sdf, _, mask = m.query_points(coord, fx["bs"], True, False, True)
    sdf, _, mask = m.assign_to_bbx(sdf, None, mask, num)
    rv, rf = mo.marching_cubes(sdf.astype(np.float32), mask)
    assert len(rf) > 0
    m.global_transform = _T()
    path = str(tmp_path / "mesh.ply")
    mesh = m.recon_bbx_mesh(box, vox, path, None, estimate_normal=True, filter_isolated_mesh=False)
    assert np.array_equal(np.asarray(mesh.triangles), rf)
    world = origin + rv.astype(np.float64) * vox
    T = m.global_transform
    want = world @ T[:3, :3].T + T[:3, 3]
    assert np.abs(np.asarray(mesh.vertices) - want).max() <= 1e-6 * vox + 1e-9
    nrm = mo.vertex_normals(world, rf) @ T[:3, :3].T
    assert np.abs(np.asarray(mesh.vertex_normals) - nrm).max() <= 1e-5
    ply = mo.read_ply(path)
    assert np.array_equal(np.stack([ply["vertex"][k] for k in "xyz"], 1), np.asarray(mesh.vertices))
    assert np.array_equal(np.stack([ply["vertex"][k] for k in ("nx", "ny", "nz")], 1), np.asarray(mesh.vertex_normals))
    assert np.array_equal(ply["face"]["vertex_indices"], rf)
    # with the cluster filter (config.min_cluster_vertices) and the sdf map
    mesh2 = m.recon_bbx_mesh(box, vox, path, str(tmp_path / "map.ply"), save_map=True)
    cid, cnt = mo.triangle_clusters(rf)
    assert np.array_equal(np.asarray(mesh2.triangles), rf[cnt[cid] >= 20])
    mp = mo.read_ply(str(tmp_path / "map.ply"))
    assert len(mp["vertex"]["x"]) == coord.shape[0] and np.array_equal(mp["vertex"]["labels"], mask.reshape(-1).astype(np.int32))


def test_recon_octree_mesh_grid_matches_the_reference_loop(tmp_path):
    fx, m = _mesher("mesh_query_L3")
    octree = m.octree
    level = octree.max_level - octree.featured_level_num + 1  # the top featured level: the fewest nodes
    mc_res_m = 0.1
    sdf, mask, voxel, origin = m.octree_grid_device(level, mc_res_m)
    # utils/mesher.py:297-337 as written: one query per node into a float16 numpy grid
    nodes = octree.get_octree_nodes(level)
    min_nodes = np.min(nodes, 0)
    max_nodes = np.max(nodes, 0)
    node_res = 2 ** (1 - level)
    k = np.ceil(node_res / m.world_scale / mc_res_m).astype(dtype=int)
    ax = torch.arange(k, dtype=torch.int16, device="cuda")
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    coord = torch.stack((x.flatten(), y.flatten(), z.flatten())).transpose(0, 1).float()
    mc_res = node_res / k
    coord *= mc_res
    count = ((max_nodes - min_nodes) / mc_res + k).astype(int)
    grid = np.zeros(tuple(count), dtype=np.float16)
    gmask = np.zeros(tuple(count), dtype=bool)
    for i in range(nodes.shape[0]):
        cur = coord.clone()
        cur += torch.tensor(nodes[i] - 0.5 * (node_res - mc_res), device="cuda")
        s, _, mk = m.query_points(cur, 4096, True, False, True)
        s, _, mk = m.assign_to_bbx(s, None, mk, np.ones(3, int) * k)
        sh = ((nodes[i] - min_nodes) / node_res * k).astype(int)
        grid[sh[0]:sh[0] + k, sh[1]:sh[1] + k, sh[2]:sh[2] + k] = s
        gmask[sh[0]:sh[0] + k, sh[1]:sh[1] + k, sh[2]:sh[2] + k] = mk
    assert np.array_equal(sdf.cpu().numpy(), grid.astype(np.float32))
    assert np.array_equal(mask.cpu().numpy(), gmask)
    assert np.isclose(voxel, mc_res / m.world_scale)
    assert np.allclose(origin, (min_nodes - 0.5 * (node_res - mc_res)) / m.world_scale)
    rv, rf = mo.marching_cubes(grid.astype(np.float32), gmask)
    assert len(rf) > 0
    mesh = m.recon_octree_mesh(level, mc_res_m, str(tmp_path / "o.ply"), None, filter_isolated_mesh=False, estimate_normal=False)
    assert np.array_equal(np.asarray(mesh.triangles), rf)
    assert np.abs(np.asarray(mesh.vertices) - (origin + rv.astype(np.float64) * voxel)).max() <= 1e-9


def test_estimate_sem_labels_and_free_space_removal(tmp_path):
    import copy

    from shine_mapping_amd import Decoder, synth
    from shine_mapping_amd.mesher import Mesher, marching_cubes, query_labels_device

    wl = synth.build_workload("maicity", frames=12, beams=32, azimuths=180, device="cuda", seed=7)
    torch.manual_seed(1)
    sem = Decoder(wl.cfg, is_geo_encoder=False)
    sem = copy.deepcopy(sem)
    with torch.no_grad():  # (spread the logits of the untrained head, as tests/test_gpu_semantic.py does)
        sem.layers[0].weight.mul_(100.0)
        sem.nclass_out.weight.mul_(10.0)
    cfg = wl.cfg
    cfg.mc_mask_on = True
    m = Mesher(cfg, wl.octree, wl.decoder, sem)
    lo = (wl.pool.coord.min(0).values / cfg.scale).cpu().numpy()
    hi = (wl.pool.coord.max(0).values / cfg.scale).cpu().numpy()
    box, vox = _Box(lo, hi), 0.4
    coord, num, origin = m.get_query_from_bbx(box, vox)
    _cross_zero(m, coord)
    sdf, mask = m._fill_grid(coord, tuple(int(v) for v in num), m._check_level(), True)
    v, f = marching_cubes(sdf, mask)
    assert len(f) > 100
    vw = torch.as_tensor(origin, device="cuda") + v.double() * vox
    with torch.no_grad():  # raise class 0 (free space) until it wins on about half of the vertices
        logp = sem._sem_composite(wl.octree.query_feature((vw * cfg.scale).float(), True))
        margin = logp.max(1).values - logp[:, 0]
        sem.nclass_out.bias[0] += float(margin.median()) + 1e-4
    labels = query_labels_device(wl.octree, sem, (vw * cfg.scale).float()).cpu().numpy()
    assert len(np.unique(labels)) > 1 and 0 < (labels <= 0).sum() < len(labels)
    rv, rf, rl = mo.remove_vertices_by_mask(vw.cpu().numpy(), f.cpu().numpy(), labels <= 0, labels)
    mesh = m.recon_bbx_mesh(box, vox, str(tmp_path / "s.ply"), None, estimate_sem=True, estimate_normal=False,
                            filter_isolated_mesh=False)
    assert np.array_equal(np.asarray(mesh.triangles), rf)
    assert np.array_equal(np.asarray(mesh.vertices), rv)
    if hasattr(mesh, "vertex_labels") and mesh.vertex_labels is not None:
        assert np.array_equal(mesh.vertex_labels, rl)
