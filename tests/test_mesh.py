"""CPU: the marching-cubes table (csrc/shine_mc_tables.hpp) is complete, crack-free and consistently oriented; the numpy
oracle (tests/mc_oracle.py) makes closed meshes of the right topology; the PLY writer round-trips; the mesher's host logic
(octree grid layout, memory refusal, empty results); the post-processing oracles agree with each other and with the bound the
kernels are held to, on the hand-built meshes of tests/mesh_post_cases.py; shine_mesh.hip's size checks."""
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mc_oracle as mo
import mesh_post_cases as mp
from conftest import ROOT


def _corner_in(case, c):
    return (case >> c) & 1


def _boundary(tris):
    """directed edges of the cube's triangles that no other triangle of the cube uses (in either direction)"""
    und = {}
    for t in tris:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            und.setdefault((min(a, b), max(a, b)), []).append((a, b))
    return [d[0] for d in und.values() if len(d) == 1]


def _face_edges(a, s):
    return {e for e in range(12) if all(((c >> a) & 1) == s for c in mo.edge_corners(e))}


def test_generated_header_is_up_to_date():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_tables.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_table_uses_exactly_the_crossing_edges():
    for case in range(256):
        crossing = {e for e in range(12) if _corner_in(case, mo.edge_corners(e)[0]) != _corner_in(case, mo.edge_corners(e)[1])}
        used = {e for t in mo.TRI[case] for e in t}
        assert used == crossing, case
        for t in mo.TRI[case]:
            assert len(set(t)) == 3, (case, t)


def test_table_is_crack_free_and_consistently_oriented_across_faces():
    """Every boundary segment of a case lies on one cube face; for each face and every pair of configurations that agree on it,
    the two cubes put the same segments there, in opposite directions."""
    segs = {}
    for case in range(256):
        bd = _boundary(mo.TRI[case])
        per = {}
        for a, s in itertools.product(range(3), range(2)):
            fe = _face_edges(a, s)
            per[(a, s)] = sorted(d for d in bd if d[0] in fe and d[1] in fe)
        assert sum(len(v) for v in per.values()) == len(bd), case  # (no boundary segment crosses the cube's interior)
        segs[case] = per
    for a in range(3):
        hi_corners = [c for c in range(8) if (c >> a) & 1]
        lo_corners = [c for c in range(8) if not (c >> a) & 1]

        def mirror(e):
            c0, c1 = mo.edge_corners(e)
            c0, c1 = c0 ^ (1 << a), c1 ^ (1 << a)
            return [x for x in range(12) if set(mo.edge_corners(x)) == {c0, c1}][0]

        for ca in range(256):
            for free in range(16):
                cb = 0
                for c in hi_corners:  # B's low face = A's high face
                    cb |= _corner_in(ca, c) << (c ^ (1 << a))
                for k, c in enumerate(hi_corners):  # B's own far corners: any
                    cb |= ((free >> k) & 1) << c
                got_a = sorted((mirror(y), mirror(x)) for x, y in segs[ca][(a, 1)])  # reversed, in B's edge names
                assert got_a == segs[cb][(a, 0)], (a, ca, cb)
        assert lo_corners


def _topology(verts, faces):
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(d, 1)
    _, cu = np.unique(und, axis=0, return_counts=True)
    _, cd = np.unique(d, axis=0, return_counts=True)
    used = len(np.unique(f))
    return cu, cd, used - len(cu) + len(f)


def _sphere(n, c, r):
    g = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    return (r - np.sqrt(((g - np.asarray(c, np.float64).reshape(3, 1, 1, 1)) ** 2).sum(0))).astype(np.float32)


def _torus(n, c, R, r):
    g = np.mgrid[0:n, 0:n, 0:n].astype(np.float64) - np.asarray(c, np.float64).reshape(3, 1, 1, 1)
    q = np.sqrt(g[0] ** 2 + g[1] ** 2) - R
    return (r - np.sqrt(q ** 2 + g[2] ** 2)).astype(np.float32)


@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_oracle_mesh_is_closed_oriented_with_the_right_euler_characteristic(kind):
    sdf = _sphere(40, (19.3, 20.1, 18.7), 13.0) if kind == "sphere" else _torus(48, (23.6, 24.2, 23.9), 13.0, 5.5)
    verts, faces = mo.marching_cubes(sdf)
    cu, cd, chi = _topology(verts, faces)
    assert len(faces) > 1000
    assert (cu == 2).all() and cd.max() == 1
    assert chi == (2 if kind == "sphere" else 0)
    v = verts.astype(np.float64)
    vol = np.einsum("ij,ij->i", v[faces[:, 0]], np.cross(v[faces[:, 1]], v[faces[:, 2]])).sum() / 6
    assert vol > 0


def test_oracle_exact_zeros_give_no_degenerate_faces():
    z = np.arange(12, dtype=np.float32)
    sdf = np.broadcast_to(5.0 - z, (9, 10, 12)).copy()  # the plane z = 5 through grid points
    verts, faces = mo.marching_cubes(sdf)
    assert len(faces) == 2 * 8 * 9
    assert len(np.unique(verts, axis=0)) == len(verts) == 9 * 10
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()


def test_oracle_empty_surface_and_out_of_range_level():
    sdf = _sphere(10, (4.5, 4.5, 4.5), 3.0)
    for lev in (10.0, -100.0):
        v, f = mo.marching_cubes(sdf, level=lev)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = mo.marching_cubes(sdf, mask=np.zeros(sdf.shape, bool))
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_ply_round_trip(tmp_path):
    from shine_mapping_amd.mesher import write_ply

    rng = np.random.default_rng(0)
    v = rng.normal(size=(50, 3))
    n = rng.normal(size=(50, 3))
    rgb = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    f = rng.integers(0, 50, size=(70, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    write_ply(p, [("x", v[:, 0], "double"), ("y", v[:, 1], "double"), ("z", v[:, 2], "double"), ("nx", n[:, 0], "double"),
                  ("ny", n[:, 1], "double"), ("nz", n[:, 2], "double"), ("red", rgb[:, 0], "uchar"),
                  ("green", rgb[:, 1], "uchar"), ("blue", rgb[:, 2], "uchar")], f)
    got = mo.read_ply(p)
    assert np.array_equal(np.stack([got["vertex"][k] for k in "xyz"], 1), v)
    assert np.array_equal(np.stack([got["vertex"][k] for k in ("nx", "ny", "nz")], 1), n)
    assert np.array_equal(np.stack([got["vertex"][k] for k in ("red", "green", "blue")], 1), rgb)
    assert np.array_equal(got["face"]["vertex_indices"], f)
    # the sdf-map form: float positions, intensities, int labels, no faces
    p2 = str(tmp_path / "map.ply")
    write_ply(p2, [("x", v[:, 0], "float"), ("intensities", n[:, 0], "float"), ("labels", rgb[:, 0].astype(np.int32), "int")])
    got = mo.read_ply(p2)
    assert np.array_equal(got["vertex"]["x"], v[:, 0].astype(np.float32)) and "face" not in got
    assert np.array_equal(got["vertex"]["labels"], rgb[:, 0].astype(np.int32))


class _Nodes:
    def __init__(self, centres):
        self.centres = centres
        self.hier_features = []

    def get_octree_nodes(self, level):
        return self.centres


def test_octree_grid_layout_offsets():
    """recon_octree_mesh's node blocks land at disjoint offsets that tile the grid (utils/mesher.py:297-337 arithmetic)."""
    from shine_mapping_amd.mesher import Mesher

    level, world_level = 10, 12
    scale = 1.0 / (0.2 * 2 ** (world_level - 1))
    size = 2.0 ** (1 - level)
    rng = np.random.default_rng(3)
    ijk = np.unique(rng.integers(0, 40, size=(300, 3)), axis=0)
    centres = ijk * size - 1.0 + 0.5 * size
    cfg = SimpleNamespace(device="cpu", dtype=torch.float32, scale=scale, pad_voxel=2, mc_vis_level=1)
    m = Mesher(cfg, _Nodes(centres), None)
    nodes, node_res, k, mc_res, shape, shift = m.octree_grid_layout(level, 0.1)
    assert k == int(np.ceil(size / scale / 0.1)) == 8 and np.isclose(mc_res * k, node_res)
    assert np.array_equal(shift, (ijk - ijk.min(0)) * k)
    assert np.array_equal(shape, (ijk.max(0) - ijk.min(0) + 1) * k)
    owner = np.full(tuple(shape), -1)
    for n, s in enumerate(shift):
        blk = owner[s[0]:s[0] + k, s[1]:s[1] + k, s[2]:s[2] + k]
        assert blk.shape == (k, k, k) and (blk == -1).all()
        blk[...] = n


def test_memory_estimate_refuses_a_grid_that_does_not_fit():
    from shine_mapping_amd.mesher import dense_grid_bytes, ensure_grid_fits

    assert dense_grid_bytes((100, 100, 100), True) >= 10 ** 6 * 10
    with pytest.raises(MemoryError, match="1300x1300x1300"):
        ensure_grid_fits((1300, 1300, 1300), True, free_bytes=16 * 10 ** 9)
    assert ensure_grid_fits((64, 64, 64), True, free_bytes=16 * 10 ** 9) > 0


def test_marching_cubes_refuses_host_tensors():
    from shine_mapping_amd.mesher import marching_cubes

    with pytest.raises(ValueError, match="CUDA"):
        marching_cubes(torch.zeros(4, 4, 4))


def test_triangle_mesh_transform_matches_open3d_convention():
    from shine_mapping_amd.mesher import TriangleMesh

    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [1, 2, 3]
    m = TriangleMesh([[1.0, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 2]], vertex_normals=[[1.0, 0, 0]] * 3)
    m.transform(T)
    assert np.allclose(m.vertices, [[1, 3, 3], [0, 2, 3], [1, 2, 4]]) and np.allclose(m.vertex_normals, [[0, 1, 0]] * 3)


# ------------------------------------------------------------------------------------- the post-processing oracles (mc_oracle.py)
@pytest.mark.parametrize("name", mp.CLUSTER_NAMES)
def test_cluster_oracles_agree(name):
    """the union-find and the sort + connected_components oracle, on every cluster input of tests/test_gpu_mesh_post.py"""
    if not mo.have_scipy():
        pytest.skip("scipy does not import: nothing to compare the union-find with")
    f = mp.cluster_cases()[name]
    cid, cnt = mo.triangle_clusters(f)
    gid, gcnt = mo.triangle_clusters_graph(f)
    assert np.array_equal(cid, gid) and np.array_equal(cnt, gcnt)
    assert cnt.sum() == len(f) and (cnt > 0).all()
    first = np.full(len(cnt), len(f))
    np.minimum.at(first, gid, np.arange(len(f)))
    assert (np.diff(first) > 0).all(), "clusters are numbered in the order of their first triangle"


def test_cluster_oracle_on_the_meshes_with_known_answers():
    def graph(f):
        return mo.triangle_clusters_graph(f) if mo.have_scipy() else mo.triangle_clusters(f)

    c = mp.cluster_cases()
    for name in ("strip-identity", "strip-reversed", "strip-random", "strip-zigzag"):
        assert graph(c[name])[1].tolist() == [mp.STRIP_LEN]
    f, owner = mp.many_strips()
    cid, cnt = graph(f)
    assert np.array_equal(cid, owner) and cnt.tolist() == list(mp.MANY_STRIPS)
    assert 300 in cnt and 299 in cnt
    assert graph(c["singletons"])[1].tolist() == [1] * mp.SINGLETONS
    assert graph(c["bow-tie"])[0].tolist() == [0, 1]
    assert graph(c["edge-opposite"])[0].tolist() == [0, 0] and graph(c["edge-same"])[0].tolist() == [0, 0]
    for k in mp.BOOKS:
        cid, cnt = graph(c["book-%d" % k])
        assert sorted(cnt.tolist()) == [1, k] and cid[k // 2] == 1 and cnt[1] == 1
    assert graph(c["duplicates"])[0].tolist() == [0, 1, 0, 0]
    assert graph(c["degenerate"])[0].tolist() == [0, 1, 2, 1, 3]
    assert graph(c["degenerate-attached"])[0].tolist() == [0, 1, 1]
    assert graph(c["lone-point"])[0].tolist() == [0]
    cnt = graph(c["sheet-10"])[1]
    assert cnt.max() > 0.9 * len(c["sheet-10"]) and len(cnt) > 10  # one sheet and the crumbs around its holes
    cnt = graph(c["sheet-60"])[1]
    assert len(cnt) > 5000 and len(np.unique(cnt)) >= 20  # at 60 % it falls into many clusters of mixed size
    for F in mp.LAUNCH_F:
        want = [1] if F == 1 else ([F - 2, 2] if F >= 4 else [F - 1, 1])
        assert graph(c["launch-%d-small-last" % F])[1].tolist() == want
        if F > 1:
            assert graph(c["launch-%d-big-last" % F])[1].tolist() == want[::-1]
    small = graph(c["ids-2^16"])
    assert small[0].tolist() == [0, 1, 2, 2, 3, 3] + [4] * 10
    for name in ("ids-2^24", "ids-2^31"):
        assert np.array_equal(graph(c[name])[0], small[0])
    assert c["ids-2^31"].max() == 2 ** 31 - 1
    assert graph(c["ids-top-bit"])[0].tolist() == [0, 1, 0, 2, 3, 4, 5, 6, 6]


@pytest.mark.parametrize("name", mp.NORMALS_NAMES)
def test_plain_fp64_normals_stay_inside_the_bound(name, capsys):
    """an honest fp64 evaluation (numpy's, no contraction, another summation order) passes the bound the kernel is held to
    (mesh_post_cases.check_normals), on every normals input of tests/test_gpu_mesh_post.py"""
    v, f, cancel = mp.normals_cases()[name]
    ref, kv, cond = mp.normals_reference(name)
    ratio = mp.check_normals(mo.vertex_normals(v, f), ref, kv, cond, cancel)
    fin = cond[np.isfinite(cond)]
    with capsys.disabled():
        print("\n  %s: numpy fp64 max |n - n_ref| / bound = %.3g, max cond_v = %.3g" % (name, ratio, fin.max() if len(fin) else 0.0))
    assert ratio <= 1.0


def test_extended_normals_oracle_on_known_meshes():
    v, f, cancel = mp.normals_cases()["cancelling"]
    n, kv, cond = mo.vertex_normals_ext(v, f)
    assert n.dtype == np.longdouble and kv.tolist() == [2, 2, 2, 2, 1, 2, 1]
    assert np.flatnonzero(np.isinf(cond)).tolist() == list(cancel) and (n[list(cancel)] == 0).all()
    assert np.array_equal(n[4], [0, 0, 1]) and np.array_equal(n[6], [0, 0, -1]) and cond[4] == 1.0
    v, f, cancel = mp.normals_cases()["star"]
    n, kv, cond = mo.vertex_normals_ext(v, f)
    assert kv[0] == 7 and kv[12] == 1 and kv[6] == 0 and kv[13] == 0 and np.flatnonzero(np.isinf(cond)).tolist() == [6, 13]
    # a right triangle seen from its sharp corner: |e1| |e2| / |fn| = 1 / sin(angle at v0)
    n, kv, cond = mo.vertex_normals_ext([[0, 0, 0], [1, 0, 0], [1, 1e-3, 0]], [[0, 1, 2]])
    assert np.allclose(cond, np.sqrt(1 + 1e-6) / 1e-3) and np.array_equal(n, [[0, 0, 1]] * 3)
    v, f, _ = mp.normals_cases()["fan"]
    assert mo.vertex_normals_ext(v, f)[1][0] == mp.FAN


def test_mesh_post_entry_points_reject_bad_sizes_without_a_gpu():
    import ctypes as C

    from shine_mapping_amd import _lib

    lib = _lib.lib()
    INVALID = -1
    host = (C.c_char * 4096)()  # stands in for device memory: every call below returns before anything would touch it
    p = C.cast(host, C.c_void_p)
    need, kept = C.c_size_t(0), C.c_int64(-7)

    def normals(nv, nf, ws=None, wb=need):
        return lib.shine_mesh_vertex_normals(p, nv, p, nf, ws, C.byref(wb) if wb is not None else None, p, None)

    def clusters(nf, ws=None, wb=need, out=kept):
        return lib.shine_mesh_cluster_filter(p, nf, 300, ws, C.byref(wb) if wb is not None else None, None, p,
                                             C.byref(out) if out is not None else None, None)

    for ws in (None, p):  # the size query and the call itself
        assert normals(1 << 31, 10, ws) == INVALID and normals(10, 1 << 31, ws) == INVALID
        assert b"shine_mesh_vertex_normals" in lib.shine_error_string(INVALID) and b"2^31" in lib.shine_error_string(INVALID)
        assert normals(-1, 10, ws) == INVALID and normals(10, -1, ws) == INVALID and normals(10, 10, ws, None) == INVALID
        assert clusters(1 << 31, ws) == INVALID and clusters(1 << 40, ws) == INVALID
        assert b"shine_mesh_cluster_filter" in lib.shine_error_string(INVALID) and b"2^31" in lib.shine_error_string(INVALID)
        assert clusters(-1, ws) == INVALID and clusters(10, ws, None) == INVALID
    assert kept.value == -7
    # One below the limit is not refused for its size.  The size query itself asks rocPRIM for its scratch, which asks for the
    # device's architecture: 0 and a size with a GPU, a HIP error (not INVALID) without one, so the sizes, the too-small workspace
    # and the null kept_out, which the library checks after the query, are tested on the device (tests/test_gpu_mesh_post.py).
    for rc in (normals((1 << 31) - 1, 256), clusters(256)):
        assert rc != INVALID and (rc != 0 or need.value >= 256 * 8)
