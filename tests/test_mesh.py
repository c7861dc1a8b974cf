"""CPU: the marching-cubes table (csrc/shine_mc_tables.hpp) is complete, crack-free and consistently oriented; the numpy
oracle (tests/mc_oracle.py) makes closed meshes of the right topology; the PLY writer round-trips; the mesher's host logic
(octree grid layout, memory refusal, empty results)."""
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mc_oracle as mo
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
