"""GPU: the mesh post-processing (csrc/shine_mesh.hip) on the hand-built meshes of tests/mesh_post_cases.py, which a closed
manifold marching-cubes mesh in grid order never gives: permuted strips, interleaved strips, singletons, books around one edge,
duplicate and degenerate triangles, holed open sheets, launch edges and vertex ids up to 2^31 - 1 for the cluster filter, against
the sort + connected_components oracle (mc_oracle.triangle_clusters_graph), exactly; world-sized height fields, a 20 000-face
fan, skinny and cancelling triangles and vertex counts around powers of two for the normals, against the 80-bit oracle
(mc_oracle.vertex_normals_ext) within |n - n_ref| <= 8 (k_v + 8) 2^-53 cond_v (mesh_post_cases.check_normals)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mc_oracle as mo
import mesh_post_cases as mp

pytestmark = pytest.mark.gpu


def _filter(f_dev, min_tri):
    from shine_mapping_amd.mesher import cluster_filter_device

    kept, clusters = cluster_filter_device(f_dev, min_tri, return_clusters=True)
    return kept.cpu().numpy(), clusters.cpu().numpy()


def _check_filter(faces, cid, cnt):
    """cluster ids and kept faces exact for every threshold that can change the answer, and two runs bit-identical"""
    F = len(faces)
    f_dev = torch.tensor(faces).cuda()
    for min_tri in mp.thresholds(cnt, F):
        kept, clusters = _filter(f_dev, min_tri)
        assert clusters.dtype == np.int32 and np.array_equal(clusters, cid), min_tri
        want = faces[cnt[cid] >= min_tri]
        assert kept.shape == want.shape and kept.dtype == np.int32 and np.array_equal(kept, want), min_tri
    assert min_tri == F + 1 and kept.shape == (0, 3)  # (the last threshold: nothing kept)
    mid = int(np.sort(cnt)[len(cnt) // 2])
    a, b = _filter(f_dev, mid), _filter(f_dev, mid)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two runs must be bit-identical"


@pytest.mark.parametrize("name", mp.CLUSTER_NAMES)
def test_cluster_filter_matches_the_graph_oracle(name):
    faces = mp.cluster_cases()[name]
    cid, cnt = mp.cluster_reference(name)
    _check_filter(faces, cid, cnt)


def test_cluster_filter_cuts_between_300_and_299():
    """the Mesher's default min_tri = 300 on interleaved strips, one of exactly 300 and one of 299 triangles"""
    f, owner = mp.many_strips()
    f = f.astype(np.int32)
    kept, clusters = _filter(torch.tensor(f).cuda(), 300)
    assert np.array_equal(clusters, owner)  # clusters are numbered by their first triangle: strip k's is triangle k
    keep = np.array(mp.MANY_STRIPS)[owner] >= 300
    assert keep[owner == 0].all() and not keep[owner == 1].any() and np.array_equal(kept, f[keep])


def test_cluster_filter_singletons_keep_nothing_at_two():
    f = mp.cluster_cases()["singletons"]
    kept, clusters = _filter(torch.tensor(f).cuda(), 2)
    assert kept.shape == (0, 3) and np.array_equal(clusters, np.arange(mp.SINGLETONS))
    kept, _ = _filter(torch.tensor(f).cuda(), 1)
    assert np.array_equal(kept, f)


def test_mesh_post_size_queries_and_refusals_on_the_device():
    """what the library checks after rocPRIM's size query (which asks for the device's architecture, so tests/test_mesh.py cannot
    reach it without one): the sizes, a workspace below them, a null kept_out.  Every refused call returns before a launch."""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    INVALID = -1
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    p = ws.data_ptr()
    need, kept = C.c_size_t(0), C.c_int64(-7)
    last_n = last_c = 0
    for F in (0, 1, 256, 100_000):
        assert lib.shine_mesh_cluster_filter(None, F, 300, None, C.byref(need), None, None, None, None) == 0
        # (the key and value arrays of the edge sort, five int arrays and the flags, rocPRIM's scratch on top)
        assert need.value > 0 and need.value % 8 == 0 and need.value >= F * (4 * 3 * 8 + 5 * 4 + 1) and need.value >= last_c
        last_c = need.value
        assert lib.shine_mesh_vertex_normals(None, F + 7, None, F, None, C.byref(need), None, None) == 0
        assert need.value > 0 and need.value % 8 == 0 and need.value >= F * 3 * 8 * 3 + (F + 7) * 16 and need.value >= last_n
        last_n = need.value
    small = C.c_size_t(64)
    assert lib.shine_mesh_cluster_filter(p, 256, 300, p, C.byref(small), None, p, C.byref(kept), None) == INVALID
    assert b"workspace too small" in lib.shine_error_string(INVALID) and kept.value == -7
    assert lib.shine_mesh_vertex_normals(p, 256, p, 256, p, C.byref(small), p, None) == INVALID
    assert b"workspace too small" in lib.shine_error_string(INVALID)
    big = C.c_size_t(ws.numel())
    assert lib.shine_mesh_cluster_filter(None, 256, 300, None, C.byref(need), None, None, None, None) == 0
    assert need.value <= big.value
    assert lib.shine_mesh_cluster_filter(p, 256, 300, p, C.byref(big), None, p, None, None) == INVALID
    assert b"kept_out" in lib.shine_error_string(INVALID)
    assert lib.shine_mesh_cluster_filter(None, 0, 300, p, C.byref(big), None, None, C.byref(kept), None) == 0 and kept.value == 0


# ---------------------------------------------------------------------------------------------------------------- vertex normals
def _normals(v, f):
    from shine_mapping_amd.mesher import vertex_normals_device

    n = vertex_normals_device(*(a if torch.is_tensor(a) else torch.tensor(a).cuda() for a in (v, f)))
    assert n.dtype == torch.float64 and tuple(n.shape) == (len(v), 3)
    return n


@pytest.mark.parametrize("name", mp.NORMALS_NAMES)
def test_vertex_normals_stay_inside_the_rounding_bound(name, capsys):
    v, f, cancel = mp.normals_cases()[name]
    ref, kv, cond = mp.normals_reference(name)
    n = _normals(v, f).cpu().numpy()
    with capsys.disabled():
        cmp = cond <= mp.COND_LIMIT
        err = np.abs(n.astype(np.longdouble) - ref).max(1)[cmp].astype(np.float64)
        bound = 8.0 * (kv[cmp] + 8) * 2.0 ** -53 * cond[cmp]
        print("\n  %s: max |n - n_ref| / bound = %.3g (max error %.3g)"
              % (name, (err / bound).max() if cmp.any() else 0.0, err.max() if cmp.any() else 0.0))
    mp.check_normals(n, ref, kv, cond, cancel)
    if name in ("cancelling", "no-faces", "key-width-1", "key-width-2"):
        assert (n[list(cancel)] == 0).all()
    if name == "cancelling":
        assert np.array_equal(n[4], [0, 0, 1]) and np.array_equal(n[6], [0, 0, -1])


@pytest.mark.parametrize("name", ["field-world-shuffled", "fan"])
def test_vertex_normals_are_bit_identical_from_run_to_run(name):
    v, f, _ = mp.normals_cases()[name]
    assert torch.equal(_normals(v, f), _normals(v, f))


# ------------------------------------------------------------------------------------------------------------------- composition
def test_remove_vertices_then_filter_and_normals(capsys):
    """estimate_sem's order of work: vertices dropped and ids compacted (open borders, vertices without faces), then the filter
    and the normals on the compacted mesh"""
    from shine_mapping_amd.mesher import remove_vertices_device

    v, _ = mp.height_field(mp.SHEET_N, mp.SHEET_N, shift=mp.WORLD_SHIFT)
    f = mp.cluster_cases()["sheet-10"]
    drop = np.random.default_rng(31).random(len(v)) < 0.30
    rv, rf = mo.remove_vertices_by_mask(v, f, drop)
    dv, df = remove_vertices_device(torch.tensor(v).cuda(), torch.tensor(f).cuda(), torch.tensor(drop).cuda())
    assert df.dtype == torch.int32 and np.array_equal(dv.cpu().numpy(), rv) and np.array_equal(df.cpu().numpy(), rf)
    assert 1000 < len(rf) < len(f)
    cid, cnt = mp.clusters_oracle(rf)
    assert len(cnt) > 100
    for min_tri in (2, 20, 300):
        kept, clusters = _filter(df, min_tri)
        assert np.array_equal(clusters, cid) and np.array_equal(kept, rf[cnt[cid] >= min_tri])
    ref, kv, cond = mo.vertex_normals_ext(rv, rf)
    bare = np.flatnonzero(kv == 0)  # vertices that lost all their faces: normal 0, the only ones outside the bound
    assert len(bare) > 0
    n = _normals(dv, df).cpu().numpy()
    ratio = mp.check_normals(n, ref, kv, cond, tuple(bare.tolist()))
    with capsys.disabled():
        print("\n  composition: max |n - n_ref| / bound = %.3g" % ratio)
    assert (n[bare] == 0).all()
