"""CPU suite of the brick-set marching cubes (csrc/shine_mc_sparse.hip): the entry points' host-side argument
checks, the brick table of an octree_grid_layout result, and the box route's candidate tiles."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

import mc_sparse_oracle as so


def _org(rows):
    a = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 3))
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


def test_sparse_entry_points_reject_bad_arguments_without_a_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    INVALID = -1
    host = (C.c_char * 4096)()  # stands in for device memory: every call below returns before anything would touch it
    p = C.cast(host, C.c_void_p)
    need = C.c_size_t(0)
    counts = (C.c_int64 * 2)(-7, -7)
    keep, org = _org([[0, 0, 0], [12, 0, 0], [12, 12, 24]])

    def count(values=p, mask=None, origins=org, n=3, B=12, shape=(48, 36, 36), ws=None, wb=need, out=counts):
        return lib.shine_mc_sparse_count(values, mask, origins, n, B, shape[0], shape[1], shape[2], 0.0, ws,
                                         C.byref(wb) if wb is not None else None, out, None)

    # the size query is host arithmetic: per brick the classify byte and the record base of (B + 1)^3 apron points, the table
    assert count() == 0
    assert need.value >= 3 * (13 ** 3) * 5 + 3 * (24 + 32)
    first = need.value
    assert count(n=2) == 0 and need.value < first
    assert count(wb=None) == INVALID
    for B in (0, -1, 33, 64):  # the brick edge is 1..32
        assert count(B=B) == INVALID, B
    assert b"shine_mc_sparse_count" in lib.shine_error_string(INVALID)
    assert count(B=1, origins=_org([[0, 0, 0], [1, 0, 0], [47, 35, 35]])[1]) == 0
    assert count(B=32, origins=_org([[0, 0, 0], [32, 0, 0], [32, 32, 32]])[1], shape=(64, 64, 64)) == 0
    bad = {"unaligned": [[0, 0, 0], [12, 0, 0], [12, 13, 24]], "negative": [[0, 0, 0], [-12, 0, 0], [12, 12, 24]],
           "outside": [[0, 0, 0], [48, 0, 0], [12, 12, 24]], "repeated": [[0, 0, 0], [12, 0, 0], [12, 0, 0]]}
    for name, rows in bad.items():
        k, o = _org(rows)
        assert count(origins=o) == INVALID, name
    k, o = _org(bad["unaligned"])
    assert count(origins=o) == INVALID and b"multiple of the brick edge" in lib.shine_error_string(INVALID)
    assert count(shape=(-48, 36, 36)) == INVALID and count(shape=(48, 36, -1)) == INVALID  # negative extents
    assert count(n=-1) == INVALID and count(n=1 << 31) == INVALID
    assert count(values=None) == INVALID and count(origins=None) == INVALID
    # the virtual grid is an index space only, but face keys are cube index * 8 in 64 bits: nx * ny * nz < 2^60
    assert count(shape=(1 << 20, 1 << 20, 1 << 19)) == 0
    assert count(shape=(1 << 20, 1 << 20, 1 << 20)) == INVALID
    assert count(shape=(1 << 40, 1 << 40, 1 << 40)) == INVALID  # (the product wraps around 64 bits)
    # with a workspace: NULL outputs
    big = C.c_size_t(1 << 30)
    assert count(ws=p, wb=big, out=None) == INVALID
    small = C.c_size_t(64)
    assert count(ws=p, wb=small) == INVALID
    # no bricks: an empty mesh, nothing launched
    assert lib.shine_mc_sparse_count(None, None, None, 0, 12, 48, 36, 36, 0.0, p, C.byref(big), counts, None) == 0
    assert (counts[0], counts[1]) == (0, 0)

    nv = C.c_int64(-7)

    def emit(values=p, n=3, B=12, shape=(48, 36, 36), ws=p, wb=1 << 30, nr=100, nf=200, scratch=p, sb=big, verts=p, faces=p,
             nv_out=nv):
        return lib.shine_mc_sparse_emit(values, None, n, B, shape[0], shape[1], shape[2], 0.0, ws, wb, nr, nf, scratch,
                                        C.byref(sb) if sb is not None else None, verts, faces,
                                        C.byref(nv_out) if nv_out is not None else None, None)

    sneed = C.c_size_t(0)
    assert emit(scratch=None, sb=sneed) == 0
    assert sneed.value >= 100 * (32 + 9) + 200 * (32 + 12)  # sort buffers, head flag, scan, rank; face keys and records
    assert emit(sb=None) == INVALID
    for B in (0, 33):
        assert emit(B=B) == INVALID
    assert b"shine_mc_sparse_emit" in lib.shine_error_string(INVALID)
    assert emit(shape=(48, -36, 36)) == INVALID and emit(shape=(1 << 20, 1 << 20, 1 << 20)) == INVALID
    assert emit(nr=-1) == INVALID and emit(nf=1 << 31) == INVALID and emit(nr=0) == INVALID  # (faces without records)
    assert emit(values=None) == INVALID
    assert emit(verts=None) == INVALID and emit(faces=None) == INVALID and emit(nv_out=None) == INVALID  # NULL outputs, n > 0
    assert emit(sb=C.c_size_t(64)) == INVALID and emit(ws=None) == INVALID and emit(wb=64) == INVALID
    assert emit(nr=0, nf=0) == 0 and nv.value == 0
    del keep


class _Nodes:
    def __init__(self, centres):
        self.centres = np.asarray(centres, np.float64)
        self.hier_features = []

    def get_octree_nodes(self, level):
        return self.centres


def _layout_mesher(cells, level, scale):
    """a Mesher whose octree holds the level-`level` nodes with integer cell coordinates `cells`"""
    from shine_mapping_amd.mesher import Mesher

    size = 2.0 ** (1 - level)
    centres = np.asarray(cells, np.float64) * size - 1.0 + 0.5 * size
    cfg = SimpleNamespace(device="cpu", dtype=torch.float32, scale=scale)
    return Mesher(cfg, _Nodes(centres), None)


# face-, edge- and corner-adjacent nodes around (5, 5, 5), and isolated ones
CELLS = [(5, 5, 5), (6, 5, 5), (5, 6, 5), (5, 5, 4), (6, 6, 5), (4, 5, 6), (6, 6, 6), (4, 4, 4), (9, 2, 7), (1, 11, 3), (12, 12, 0)]


def test_brick_table_covers_exactly_the_node_blocks():
    from shine_mapping_amd.mesher import brick_edge, octree_brick_table, split_blocks

    level, scale = 6, 0.02
    m = _layout_mesher(CELLS, level, scale)
    node_m = 2.0 ** (1 - level) / scale  # 1.5625 m
    for mc_res_m, k_want, B_want in ((node_m / 12 * 1.001, 12, 12), (node_m / 36 * 1.001, 36, 18), (node_m / 5 * 1.01, 5, 5), (node_m / 34 * 1.001, 34, 17)):
        nodes, node_res, k, mc_res, shape, shift = m.octree_grid_layout(level, mc_res_m)
        assert k == k_want and brick_edge(k) == B_want
        B, origins = octree_brick_table(k, shift)
        assert B == B_want and origins.dtype == np.int64 and origins.shape == (len(CELLS) * (k // B) ** 3, 3)
        assert (origins % B == 0).all() and (origins >= 0).all() and (origins + B <= np.asarray(shape)).all()
        assert len({tuple(o) for o in origins.tolist()}) == len(origins)  # no two bricks at one origin
        # the points of the node blocks, from the layout alone
        want = so.covered_points(shift, k)
        assert len(want) == len(CELLS) * k ** 3  # (the blocks do not overlap)
        assert so.covered_points(origins, B) == want
        # split_blocks cuts the block values in the table's order: every brick value is its block's at the same grid point
        lin = lambda p: (p[..., 0] * int(shape[1]) + p[..., 1]) * int(shape[2]) + p[..., 2]  # noqa: E731
        ax = np.arange(k)
        blk = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)
        vals = torch.as_tensor(np.stack([lin(blk + s) for s in np.asarray(shift, np.int64)]))
        bricks = split_blocks(vals, B).numpy()
        ax = np.arange(B)
        loc = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)
        assert bricks.shape == (len(origins), B, B, B)
        assert all(np.array_equal(bricks[i], lin(loc + origins[i])) for i in range(len(origins)))
    assert brick_edge(37) == 1 and brick_edge(64) == 32 and brick_edge(1) == 1 and brick_edge(32) == 32


def test_box_candidate_tiles_hold_every_mask_set_point():
    from shine_mapping_amd.mesher import BOX_BRICK, box_candidate_tiles, with_upper_neighbours

    level, scale = 6, 0.02
    size = 2.0 ** (1 - level)
    cells = np.asarray(CELLS, np.int64)
    centres = cells * size - 1.0 + 0.5 * size
    have = {tuple(c) for c in cells.tolist()}
    for voxel, origin, shape in ((0.1, np.array([-45.03, -44.9, -50.2]), (260, 250, 190)),
                                 (0.37, np.array([-47.0, -41.3, -49.0]), (70, 61, 50)),
                                 (0.1, np.array([-40.0, -40.0, -48.0]), (64, 90, 120))):  # (a box that cuts through nodes)
        # get_query_from_bbx's coordinates in fp32, and the node each point falls in (kaolin's quantisation)
        idx = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
        coord = idx.astype(np.float32) * np.float32(voxel)
        coord = coord + origin.astype(np.float32)
        coord = coord * np.float32(scale)
        res = 2 ** level
        q = np.floor(np.clip(res * (coord + np.float32(1.0)) / np.float32(2.0), 0, res - 1.0)).astype(np.int64)
        set_ = np.fromiter((tuple(r) in have for r in q.tolist()), bool, len(q))
        assert set_.sum() > 100  # (the case is not vacuous)
        B = BOX_BRICK
        tiles = box_candidate_tiles(centres, size, scale, origin, voxel, shape, B)
        ntile = (np.asarray(shape) + B - 1) // B
        assert (tiles >= 0).all() and (tiles < ntile).all() and len({tuple(t) for t in tiles.tolist()}) == len(tiles)
        cand = {tuple(t) for t in tiles.tolist()}
        need = {tuple(t) for t in (idx[set_] // B).tolist()}
        assert need <= cand
        assert len(cand) < int(np.prod(ntile))  # (and it leaves tiles out)
        grown = {tuple(t) for t in with_upper_neighbours(tiles, ntile).tolist()}
        for t in list(cand)[:50]:
            for d in ((1, 0, 0), (0, 1, 1), (1, 1, 1)):
                u = tuple(np.add(t, d))
                assert u in grown or not (np.asarray(u) < ntile).all()
        assert cand <= grown
    assert box_candidate_tiles(np.zeros((0, 3)), size, scale, np.zeros(3), 0.1, (10, 10, 10)).shape == (0, 3)
