"""The reference's Mesher (utils/mesher.py) on the device: the SDF query, marching cubes, vertex normals, the small-cluster
filter and the PLY output.

`query_points` keeps the reference's argument list and return convention (numpy arrays; `sdf_pred` is the NEGATED
decoder output, `mc_mask` says whether the point's node exists at the marching-cubes check level) but runs each
chunk as ONE launch of `shine_query_points` (csrc/shine_query.hip): no `[N,8]` index tensors, no `[N,F]` features
and no per-level host round trips.  With `query_sem` the semantic labels are ONE more launch per chunk
(`shine_sem_query_labels`, csrc/shine_semantic.hip: interpolation, semantic decoder, argmax).

`recon_bbx_mesh` / `recon_octree_mesh` / `mc_mesh` keep the reference's surface but never leave the device until the final
arrays: the query writes straight into a dense device grid, `marching_cubes` (csrc/shine_mc.hip) replaces skimage's, and
`compute_vertex_normals` / `filter_isolated_vertices` are csrc/shine_mesh.hip.  The rules the marching cubes follows (corner
sign, vertex placement, degenerate faces, winding, output order) are in DESIGN.md "Meshing".  The mesh comes back as an
open3d TriangleMesh when open3d can be imported, else as this module's `TriangleMesh`; the PLY writer is plain numpy.

A map whose dense grid does not fit the device is meshed from BRICKS instead (`marching_cubes_sparse`, csrc/shine_mc_sparse.hip):
only the node blocks (octree route) or the tiles near existing nodes (box route) are queried and kept, and the mesh is the dense
route's bit for bit.  `recon_octree_mesh` / `recon_bbx_mesh` pick the route with their `sparse` keyword.

With `config.time_conditioned` (utils/mesher.py:29,71-74,94-97) the queries decode at `Mesher.ts`: the time stamp is folded into the
decoder's first bias once per call (`Decoder.fused_params_at`) and the same kernels run.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .ops import _stream


def query_points_device(octree, decoder, coord, check_level=0, negate=True, query_sdf=True, query_mask=True, mlp=None):
    """One launch over `coord [N,3]` (device, scaled to [-1,1]); returns device tensors (sdf f32 | None, mask bool | None).
    `mlp`: the six tensors to decode with instead of decoder.fused_params() — a time-conditioned head folded at one time stamp
    (Decoder.fused_params_at), which this 8 -> 32 -> 32 -> 1 kernel then serves unchanged."""
    t = octree._require_tables()
    coord = octree._check_coord(coord.detach())
    n = coord.shape[0]
    dev = coord.device
    sdf = torch.empty(n, dtype=torch.float32, device=dev) if query_sdf else None
    mask = torch.empty(n, dtype=torch.uint8, device=dev) if query_mask else None
    cfg = octree.step_config()
    if not query_sdf:
        mlp = None
    elif mlp is None:
        mlp = [p.detach() for p in decoder.fused_params()]
    _lib.check(
        _lib.lib().shine_query_points(
            t.handle, C.byref(cfg), coord.data_ptr(), n, octree.feature_ptrs(), octree.row_counts(),
            _lib.ptr_array([p.data_ptr() for p in mlp]) if mlp is not None else None, int(check_level),
            1 if negate else 0, sdf.data_ptr() if sdf is not None else None,
            mask.data_ptr() if mask is not None else None, _stream(),
        ),
        "shine_query_points",
    )
    return sdf, (mask.bool() if mask is not None else None)


def query_labels_device(octree, sem_decoder, coord):
    """Semantic labels of `coord [N,3]` (device, scaled to [-1,1]): sem_label(query_feature(coord, True)) (utils/mesher.py:72-73,
    :98) as ONE launch of shine_sem_query_labels (csrc/shine_semantic.hip); int64 [N] on the device."""
    t = octree._require_tables()
    coord = octree._check_coord(coord.detach())
    n = coord.shape[0]
    label = torch.empty(n, dtype=torch.int64, device=coord.device)
    mlp = [p.detach() for p in sem_decoder.sem_params()]
    if not sem_decoder._params_on(coord.device, mlp):
        raise ValueError("the semantic decoder's parameters must be CUDA float32 contiguous on the coordinates' device")
    cfg = octree.step_config()
    _lib.check(
        _lib.lib().shine_sem_query_labels(
            t.handle, C.byref(cfg), coord.data_ptr(), n, octree.feature_ptrs(), octree.row_counts(),
            _lib.ptr_array([p.data_ptr() for p in mlp]), int(mlp[4].shape[0]), label.data_ptr(), _stream(),
        ),
        "shine_sem_query_labels",
    )
    return label


# ---------------------------------------------------------------------------------------------------------------- meshing
MC_POINT_BYTES = 4 + 4 + 1  # per grid point: the fp32 grid, the vertex-id base and the packed classify byte (csrc/shine_mc.hip)
QUERY_CHUNK = 1 << 22  # grid points per query launch when a grid is filled (the values do not depend on it)


def dense_grid_bytes(shape, with_mask=True, per_point_extra=0):
    """Device bytes a dense marching-cubes grid of `shape` takes: the grid, the optional mask and marching cubes' workspace, plus
    `per_point_extra` bytes per point the caller holds at the same time (e.g. query coordinates)."""
    n = int(np.prod([int(v) for v in shape], dtype=np.int64))
    return n * (MC_POINT_BYTES + (1 if with_mask else 0) + int(per_point_extra)) + (n // 1024 + 1) * 16 + (1 << 20)


def ensure_grid_fits(shape, with_mask=True, per_point_extra=0, free_bytes=None, device=None):
    """Raise MemoryError naming the grid when dense_grid_bytes(...) exceeds the free device memory (or `free_bytes`)."""
    need = dense_grid_bytes(shape, with_mask, per_point_extra)
    if free_bytes is None:
        free_bytes = torch.cuda.mem_get_info(device)[0]
    if need > free_bytes:
        raise MemoryError("marching cubes on a %s grid needs about %.2f GB of device memory, %.2f GB are free: use a coarser "
                          "mc_res_m or a smaller box" % ("x".join(str(int(v)) for v in shape), need / 1e9, free_bytes / 1e9))
    return need


def marching_cubes(sdf, mask=None, level=0.0):
    """Marching cubes of a device grid `sdf [X,Y,Z]` (f32, C order) with an optional mask of the same shape (cube (x,y,z) is
    processed iff mask[x,y,z]); rules in DESIGN.md "Meshing".  Returns (verts [V,3] f32 index units (x, y, z), faces [F,3]
    int32) on the device; an empty surface gives zero rows."""
    if sdf.dim() != 3 or not sdf.is_cuda:
        raise ValueError("marching_cubes: sdf must be a 3-D CUDA tensor, got %s on %s" % (tuple(sdf.shape), sdf.device))
    sdf = sdf.detach().float().contiguous()
    if mask is not None:
        if tuple(mask.shape) != tuple(sdf.shape):
            raise ValueError("marching_cubes: mask shape %s != sdf shape %s" % (tuple(mask.shape), tuple(sdf.shape)))
        mask = mask.detach().to(device=sdf.device, dtype=torch.uint8).contiguous()
    X, Y, Z = (int(v) for v in sdf.shape)
    lib, st = _lib.lib(), _stream()
    mp = mask.data_ptr() if mask is not None else None
    counts = (C.c_int64 * 2)()
    ws, need = _lib.call_with_workspace(
        lib.shine_mc_count, sdf.device, sdf.data_ptr(), mp, X, Y, Z, float(level), _lib.WS, _lib.WS_BYTES, counts, st,
        what=lambda: "shine_mc_count (%dx%dx%d grid: %d vertices, %d faces)" % (X, Y, Z, counts[0], counts[1]))
    nv, nf = int(counts[0]), int(counts[1])
    verts = torch.empty((nv, 3), dtype=torch.float32, device=sdf.device)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=sdf.device)
    if nv or nf:
        _lib.check(lib.shine_mc_emit(sdf.data_ptr(), mp, X, Y, Z, float(level), ws.data_ptr(), need.value, verts.data_ptr(),
                                     faces.data_ptr(), st), "shine_mc_emit")
    return verts, faces


MC_SPARSE_MAX_BRICK = 32  # csrc/shine_mc_sparse.hip: one workgroup stages a brick and its apron, (B + 1)^3 floats, in LDS
BOX_BRICK = 8  # tile edge of the box route's bricks


def marching_cubes_sparse(values, mask, origins, shape, level=0.0):
    """Marching cubes of a brick set: `values [n,B,B,B]` (device f32), `mask` the same shape or None, `origins [n,3]` ints
    (multiples of B inside the grid, no two equal), inside a virtual grid `shape = (X, Y, Z)` that is never allocated.  A point
    no brick covers has value 0 and mask 0; with mask None every cube whose lowest corner a brick covers is processed.  Returns
    what `marching_cubes` returns on that dense grid, bit for bit and in the same order: (verts [V,3] f32 index units of the
    virtual grid, faces [F,3] int32)."""
    if values.dim() != 4 or not values.is_cuda or not (values.shape[1] == values.shape[2] == values.shape[3]):
        raise ValueError("marching_cubes_sparse: values must be a CUDA tensor [n, B, B, B], got %s on %s"
                         % (tuple(values.shape), values.device))
    values = values.detach().float().contiguous()
    n, B = int(values.shape[0]), int(values.shape[1])
    if mask is not None:
        if tuple(mask.shape) != tuple(values.shape):
            raise ValueError("marching_cubes_sparse: mask shape %s != values shape %s" % (tuple(mask.shape), tuple(values.shape)))
        mask = mask.detach().to(device=values.device, dtype=torch.uint8).contiguous()
    org = origins.detach().cpu().numpy() if torch.is_tensor(origins) else np.asarray(origins)
    org = np.ascontiguousarray(org, dtype=np.int64).reshape(-1, 3)
    if org.shape[0] != n:
        raise ValueError("marching_cubes_sparse: %d origins for %d bricks" % (org.shape[0], n))
    X, Y, Z = (int(v) for v in shape)
    dev = values.device
    verts = torch.empty((0, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((0, 3), dtype=torch.int32, device=dev)
    lib, st = _lib.lib(), _stream()
    vp, mp = (values.data_ptr() if n else None), (mask.data_ptr() if mask is not None and n else None)
    op = org.ctypes.data_as(C.POINTER(C.c_int64))
    counts = (C.c_int64 * 2)()
    count_args = (vp, mp, op, n, B, X, Y, Z, float(level), _lib.WS, _lib.WS_BYTES, counts, st)
    if n == 0:
        _lib.workspace_bytes(lib.shine_mc_sparse_count, *count_args)  # (the query checks the arguments)
        return verts, faces
    ws, need = _lib.call_with_workspace(
        lib.shine_mc_sparse_count, dev, *count_args,
        what=lambda: "shine_mc_sparse_count (%d bricks of %d^3 in %dx%dx%d: %d vertex records, %d faces)"
        % (n, B, X, Y, Z, counts[0], counts[1]))
    nr, nf = int(counts[0]), int(counts[1])
    if nr == 0 and nf == 0:
        return verts, faces
    nv = C.c_int64(0)
    verts = torch.empty((nr, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    # (the placeholders stand for the scratch and its size: the same convention)
    scratch, _ = _lib.call_with_workspace(lib.shine_mc_sparse_emit, dev, vp, mp, n, B, X, Y, Z, float(level), ws.data_ptr(),
                                          need.value, nr, nf, _lib.WS, _lib.WS_BYTES, verts.data_ptr(), faces.data_ptr(),
                                          C.byref(nv), st)
    del scratch, ws
    # (a vertex on a brick face has one record per brick that uses it: V <= records; the copy lets the larger buffer go)
    return (verts if nv.value == nr else verts[:nv.value].clone()), faces


def brick_edge(k):
    """Brick edge for node blocks of k^3 points: k itself up to MC_SPARSE_MAX_BRICK, else its largest divisor that fits (each
    block is then cut into (k / edge)^3 bricks)."""
    k = int(k)
    return max(b for b in range(1, min(k, MC_SPARSE_MAX_BRICK) + 1) if k % b == 0)


def octree_brick_table(k, shift):
    """Brick origins of octree_grid_layout's node blocks (`shift [M,3]`, multiples of k): (brick edge B, origins [M * q^3, 3]
    int64 with q = k / B), block-major, a block's bricks in (x, y, z) order — the order split_blocks cuts the values in."""
    B = brick_edge(k)
    q = int(k) // B
    ax = np.arange(q, dtype=np.int64) * B
    off = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    shift = np.asarray(shift, dtype=np.int64).reshape(-1, 3)
    return B, (shift[:, None, :] + off[None]).reshape(-1, 3)


def split_blocks(t, B):
    """[M, k, k, k] -> [M * q^3, B, B, B] (q = k / B), bricks in octree_brick_table's order"""
    M, k = int(t.shape[0]), int(t.shape[1])
    if B == k:
        return t
    q = k // B
    return t.view(M, q, B, q, B, q, B).permute(0, 1, 3, 5, 2, 4, 6).reshape(M * q ** 3, B, B, B)


# ------------------------------------------------------------------------------------- the block cache
def mesh_cache_key(query_level, k, mc_res_scaled, mask_on, check_level, world_scale):
    """What a cached block's values depend on besides the map: a cache built under another key is dropped."""
    return (int(query_level), int(k), float(mc_res_scaled), bool(mask_on), int(check_level), float(world_scale))


def keys_are_prefix(cached_keys, keys):
    """True iff the node keys seen at the previous call are the first len(cached_keys) of the current ones (the tables are
    append-only in insertion order, so anything else means they were replaced)"""
    n = len(cached_keys)
    return n <= len(keys) and bool(np.array_equal(np.asarray(keys[:n]), np.asarray(cached_keys)))


def mesh_cache_rebuild_reason(cached, key, decoder_same, node_keys, node_ids, rows):
    """Why update_octree_mesh must rebuild its cache from nothing, or None.  `cached`: None, or an object with `key`, and per
    featured level `node_keys`, `node_ids` (the host tables seen at the previous call) and `snap_rows` (rows without the trash
    row); `node_keys` / `node_ids` / `rows` are the current ones; `decoder_same()` is asked only when the key matches.  Every
    level's tables must be a prefix, not the query level's alone: the cache holds device copies of all of them, appended by count."""
    if cached is None:
        return "first"
    if cached.key != key:
        return "key"
    if not decoder_same():
        return "decoder"
    if (any(int(r) < int(c) for r, c in zip(rows, cached.snap_rows))
            or not all(keys_are_prefix(c, k) for c, k in zip(cached.node_keys, node_keys))
            or not all(keys_are_prefix(c, i) for c, i in zip(cached.node_ids, node_ids))):
        return "octree"
    return None


def grown_capacity(have, need):
    """rows to allocate for a buffer that holds `have` and must hold `need`: geometric, so appending does not copy per frame"""
    return int(have) if need <= have else max(int(need), 2 * int(have), 16)


class _MeshCache:
    """The state update_octree_mesh keeps between calls."""

    def __init__(self, key, decoder_bits, levels):
        self.key = key
        self.decoder_bits = decoder_bits  # the geo decoder's parameters, one int32 view
        self.values = self.masks = None  # [capacity, k, k, k] f32 (half-rounded) / u8
        self.node_keys = [np.zeros(0, np.int64) for _ in range(levels)]  # the host tables of the previous call (the octree
        self.node_ids = [np.zeros((0, 8), np.int32) for _ in range(levels)]  # replaces these arrays, it never writes into them)
        self.snaps = [None] * levels  # hier_features[s] without its trash row, [capacity, 8]
        self.snap_rows = [0] * levels
        self.dev_keys = [None] * levels  # the octree's node keys / corner ids on the device, appended per call
        self.dev_ids = [None] * levels
        self.dev_nodes = [0] * levels
        self.sorted = [None] * levels  # (node count, sorted keys, permutation) of the slots <= sq


def _grow_rows(buf, used, need, tail, dtype, device):
    cap = grown_capacity(0 if buf is None else buf.shape[0], need)
    if buf is not None and cap == buf.shape[0]:
        return buf
    new = torch.empty((cap,) + tuple(tail), dtype=dtype, device=device)
    if used:
        new[:used] = buf[:used]
    return new


def rows_diff_device(feats, snaps, snap_rows, flags, changed):
    """shine_rows_diff (csrc/shine_mesh_cache.hip): feats[s] [rows, 8] f32 with the trash row last, snaps[s] with room for rows - 1,
    flags[s] u8 [rows - 1], changed int64 [levels] (added to); one launch."""
    _lib.check(_lib.lib().shine_rows_diff(
        len(feats), _lib.ptr_array([f.data_ptr() for f in feats]), _lib.ptr_array([s.data_ptr() for s in snaps]),
        _lib.i64_array([f.shape[0] for f in feats]), _lib.i64_array(snap_rows), _lib.ptr_array([f.data_ptr() for f in flags]),
        changed.data_ptr(), _stream()), "shine_rows_diff")


def mark_dirty_device(sq, node_keys, node_ids, n_nodes, prev_nodes, flags, sorted_keys, sorted_perm, dirty, counts):
    """shine_mesh_mark_dirty: per slot device node keys / [n, 8] int32 corner ids / row flags, host counts; sorted keys and
    permutation (or None) per slot; dirty u8 [n_nodes[sq]] and counts int64 [2] are outputs."""
    ptr = lambda ts: _lib.ptr_array([t.data_ptr() if t is not None else None for t in ts])
    _lib.check(_lib.lib().shine_mesh_mark_dirty(
        len(node_keys), int(sq), ptr(node_keys), ptr(node_ids), _lib.i64_array(n_nodes), _lib.i64_array(prev_nodes), ptr(flags),
        _lib.i64_array([f.shape[0] for f in flags]), ptr(sorted_keys), ptr(sorted_perm), dirty.data_ptr(), counts.data_ptr(),
        _stream()), "shine_mesh_mark_dirty")


def blocks_scatter_device(sdf, mask, index, values, masks):
    """shine_blocks_scatter: block b of `sdf` / `mask` ([n * k^3], mask bool / u8 or None) -> block index[b] of values / masks"""
    n, k3 = int(index.shape[0]), int(values[0].numel())
    _lib.check(_lib.lib().shine_blocks_scatter(sdf.data_ptr(), mask.data_ptr() if mask is not None else None, index.data_ptr(), n,
                                               k3, int(values.shape[0]), values.data_ptr(), masks.data_ptr(), _stream()),
               "shine_blocks_scatter")


def box_candidate_tiles(nodes, node_res_scaled, world_scale, voxel_origin, voxel_size, shape, B=BOX_BRICK):
    """Tiles (B^3 points, tile coordinates [T,3] int64, sorted) of a box grid — point (i, j, l) at voxel_origin + (i, j, l) *
    voxel_size metres — that may hold a point inside one of `nodes` (centres [M,3] in scaled coordinates, edge
    node_res_scaled).  A superset: every node's index range is widened by one point per side, which covers the fp32 rounding of
    get_query_from_bbx's coordinates (relative error 2^-22 on indices < 2^15)."""
    shape = np.asarray(shape, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.float64).reshape(-1, 3)
    ntile = (shape + B - 1) // B
    if len(nodes) == 0 or (shape <= 0).any():
        return np.zeros((0, 3), np.int64)
    lo = ((nodes - 0.5 * node_res_scaled) / world_scale - np.asarray(voxel_origin, np.float64)) / voxel_size
    hi = ((nodes + 0.5 * node_res_scaled) / world_scale - np.asarray(voxel_origin, np.float64)) / voxel_size
    i0 = np.floor(lo).astype(np.int64) - 1
    i1 = np.ceil(hi).astype(np.int64) + 1
    keep = ((i1 >= 0) & (i0 <= shape - 1)).all(1)
    i0, i1 = np.clip(i0[keep], 0, shape - 1), np.clip(i1[keep], 0, shape - 1)
    if len(i0) == 0:
        return np.zeros((0, 3), np.int64)
    t0, t1 = i0 // B, i1 // B
    span = int((t1 - t0).max()) + 1
    ax = np.arange(span, dtype=np.int64)
    off = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    keys = []
    for o in off:  # (span is 1-3 for the shipped settings: a node is about as wide as a tile)
        t = t0 + o
        ok = (t <= t1).all(1)
        t = t[ok]
        keys.append((t[:, 0] * ntile[1] + t[:, 1]) * ntile[2] + t[:, 2])
    keys = np.unique(np.concatenate(keys))
    return np.stack((keys // (ntile[1] * ntile[2]), keys // ntile[2] % ntile[1], keys % ntile[2]), 1)


def with_upper_neighbours(tiles, ntile):
    """`tiles` plus their 7 neighbours towards +x / +y / +z inside the tile grid: the cubes on a tile's upper faces read those
    tiles' values.  Sorted, unique."""
    tiles = np.asarray(tiles, dtype=np.int64).reshape(-1, 3)
    ntile = np.asarray(ntile, dtype=np.int64)
    if len(tiles) == 0:
        return tiles
    off = np.stack(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij"), -1).reshape(-1, 3)
    t = (tiles[:, None, :] + off[None]).reshape(-1, 3)
    t = t[(t < ntile).all(1)]
    keys = np.unique((t[:, 0] * ntile[1] + t[:, 1]) * ntile[2] + t[:, 2])
    return np.stack((keys // (ntile[1] * ntile[2]), keys // ntile[2] % ntile[1], keys % ntile[2]), 1)


def vertex_normals_device(verts, faces):
    """open3d's compute_vertex_normals on device arrays: verts [V,3] f64, faces [F,3] int32 -> normals [V,3] f64."""
    verts = verts.detach().double().contiguous()
    faces = faces.detach().to(torch.int32).contiguous()
    nv, nf = verts.shape[0], faces.shape[0]
    out = torch.zeros((nv, 3), dtype=torch.float64, device=verts.device)
    fn = _lib.lib().shine_mesh_vertex_normals
    args = (verts.data_ptr(), nv, faces.data_ptr() if nf else None, nf, _lib.WS, _lib.WS_BYTES, out.data_ptr(), _stream())
    if nv == 0:
        _lib.workspace_bytes(fn, *args)  # (the query checks the arguments)
    else:
        _lib.call_with_workspace(fn, verts.device, *args)
    return out


def cluster_filter_device(faces, min_tri, return_clusters=False):
    """Mesher.filter_isolated_vertices on device faces [F,3] int32: drop the triangles of edge-connected clusters with fewer
    than `min_tri` triangles (order kept).  With return_clusters, also the cluster id of every input triangle (open3d's
    numbering: clusters in the order of their first triangle)."""
    faces = faces.detach().to(torch.int32).contiguous()
    nf = faces.shape[0]
    out = torch.empty((nf, 3), dtype=torch.int32, device=faces.device)
    clusters = torch.empty(nf, dtype=torch.int32, device=faces.device) if return_clusters else None
    kept = C.c_int64(0)
    fn = _lib.lib().shine_mesh_cluster_filter
    args = (faces.data_ptr(), nf, int(min_tri), _lib.WS, _lib.WS_BYTES, clusters.data_ptr() if clusters is not None else None,
            out.data_ptr(), C.byref(kept), _stream())
    if nf == 0:
        _lib.workspace_bytes(fn, *args)  # (the query checks the arguments)
    else:
        _lib.call_with_workspace(fn, faces.device, *args)
    out = out[:kept.value]
    return (out, clusters) if return_clusters else out


def remove_vertices_device(verts, faces, drop, *vertex_attrs):
    """open3d's remove_vertices_by_mask on device arrays: drop the vertices where `drop`, every triangle that uses one, and
    reindex the rest (torch index ops)."""
    keep = ~drop.bool()
    new_id = torch.cumsum(keep.to(torch.int64), 0) - 1
    f = faces.long()
    fk = keep[f].all(1)
    return (verts[keep], new_id[f[fk]].to(torch.int32)) + tuple(a[keep] if a is not None else None for a in vertex_attrs)


def write_ply(path, vertex_props, faces=None):
    """Binary little-endian PLY in plain numpy.  vertex_props: [(name, 1-D array, ply type)], ply type one of double / float /
    int / uchar; faces [F,3] (written as a uchar count + int indices)."""
    types = {"double": "<f8", "float": "<f4", "int": "<i4", "uchar": "u1"}
    n = len(vertex_props[0][1]) if vertex_props else 0
    rec = np.empty(n, dtype=[(name, types[t]) for name, _, t in vertex_props])
    for name, arr, _ in vertex_props:
        rec[name] = np.asarray(arr).reshape(-1)
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n]
    head += ["property %s %s" % (t, name) for name, _, t in vertex_props]
    if faces is not None:
        faces = np.asarray(faces).reshape(-1, 3)
        head += ["element face %d" % len(faces), "property list uchar int vertex_indices"]
    head.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        fh.write(rec.tobytes())
        if faces is not None:
            fr = np.empty(len(faces), dtype=[("n", "u1"), ("i", "<i4", 3)])
            fr["n"] = 3
            fr["i"] = faces
            fh.write(fr.tobytes())


class TriangleMesh:
    """The part of open3d's TriangleMesh the drivers use, for when open3d cannot be imported: numpy arrays and transform()."""

    def __init__(self, vertices, triangles, vertex_normals=None, vertex_colors=None):
        self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
        self.vertex_normals = np.zeros((0, 3)) if vertex_normals is None else np.asarray(vertex_normals, np.float64)
        self.vertex_colors = np.zeros((0, 3)) if vertex_colors is None else np.asarray(vertex_colors, np.float64)
        self.vertex_labels = None

    def has_vertex_normals(self):
        return len(self.vertex_normals) > 0

    def has_vertex_colors(self):
        return len(self.vertex_colors) > 0

    def transform(self, T):
        """open3d's TriangleMesh.transform: points through the homogeneous 4x4, normals through its linear part."""
        T = np.asarray(T, dtype=np.float64)
        if len(self.vertices):
            h = self.vertices @ T[:3, :3].T + T[:3, 3]
            w = self.vertices @ T[3, :3] + T[3, 3]
            self.vertices = h / w[:, None]
        if self.has_vertex_normals():
            self.vertex_normals = self.vertex_normals @ T[:3, :3].T
        return self


def _open3d():
    try:
        import open3d as o3d  # noqa: F401

        return o3d
    except Exception:
        return None


def _sem_color_map(config=None):
    """class -> (r, g, b) 0-255: the reference's table when it can be imported, else the config's own map (sem_color_map, or the
    colours of label_map_path: semantic_kitti.LabelMap), else None"""
    try:
        from utils.semantic_kitti_utils import sem_kitti_color_map

        return sem_kitti_color_map
    except Exception:
        pass
    cmap = getattr(config, "sem_color_map", None)
    if cmap:
        return cmap
    if getattr(config, "label_map_path", None):
        from .semantic_kitti import LabelMap

        colors = LabelMap.from_yaml(config.label_map_path, int(getattr(config, "sem_class_count", 20))).colors
        if colors is not None:
            return {k: c * 255.0 for k, c in enumerate(colors)}
    return None


def _make_mesh(verts, faces, normals=None, colors=None):
    o3d = _open3d()
    if o3d is None:
        return TriangleMesh(verts, faces, normals, colors)
    m = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(np.asarray(verts, np.float64)),
                                  o3d.utility.Vector3iVector(np.asarray(faces, np.int32)))
    if normals is not None:
        m.vertex_normals = o3d.utility.Vector3dVector(normals)
    if colors is not None:
        m.vertex_colors = o3d.utility.Vector3dVector(colors)
    return m


def _transform_device(verts, normals, T):
    T = torch.as_tensor(np.asarray(T, dtype=np.float64), device=verts.device)
    h = verts @ T[:3, :3].T + T[:3, 3]
    w = verts @ T[3, :3] + T[3, 3]
    verts = h / w[:, None]
    if normals is not None:
        normals = normals @ T[:3, :3].T
    return verts, normals


class Mesher:
    """utils/mesher.py's Mesher: same constructor arguments, same methods and defaults."""

    def __init__(self, config, octree, geo_decoder, sem_decoder=None):
        self.config = config
        self.octree = octree
        self.geo_decoder = geo_decoder
        self.sem_decoder = sem_decoder
        self.device = config.device
        self.cur_device = self.device
        self.dtype = config.dtype
        self.world_scale = config.scale
        self.ts = 0
        self.global_transform = np.eye(4)
        self.last_mesh_device = None  # (verts f64, faces int32) of the last mesh _finish made, on the device
        self._mesh_cache = None  # update_octree_mesh's blocks, snapshots and node tables (reset_mesh_cache drops them)
        self.last_update_stats = None

    def get_query_from_bbx(self, bbx, voxel_size):
        """utils/mesher.py:110-152: grid query points of a box (anything with get_min_bound()/get_max_bound(), e.g. an
        open3d AxisAlignedBoundingBox), padded, one extra layer underground; same fp32 op order, built on the device."""
        voxel_num_xyz, voxel_origin = self._bbx_layout(bbx, voxel_size)
        dev = self.octree.hier_features[0].device if len(self.octree.hier_features) else self.device
        x = torch.arange(int(voxel_num_xyz[0]), dtype=torch.int16, device=dev)
        y = torch.arange(int(voxel_num_xyz[1]), dtype=torch.int16, device=dev)
        z = torch.arange(int(voxel_num_xyz[2]), dtype=torch.int16, device=dev)
        x, y, z = torch.meshgrid(x, y, z, indexing="ij")
        coord = torch.stack((x.flatten(), y.flatten(), z.flatten())).transpose(0, 1).float()
        coord *= voxel_size
        coord += torch.tensor(voxel_origin, dtype=self.dtype, device=dev)
        coord *= self.world_scale
        return coord, voxel_num_xyz, voxel_origin

    def query_points(self, coord, bs, query_sdf=True, query_sem=False, query_mask=True):
        """utils/mesher.py:33-108.  Returns (sdf_pred, sem_pred, mc_mask) as numpy arrays (None when not asked for)."""
        mlp = self._decoder_params() if query_sdf else None  # (folded once per call, not per chunk)
        sample_count = coord.shape[0]
        iter_n = math.ceil(sample_count / bs)
        check_level = min(self.octree.featured_level_num, self.config.mc_vis_level) - 1
        dev = self.octree.hier_features[0].device
        with torch.no_grad():
            if iter_n > 1:  # chunked: the reference fills float64 numpy buffers (:43-53)
                sdf_pred = np.zeros(sample_count) if query_sdf else None
                sem_pred = np.zeros(sample_count) if query_sem else None
                mc_mask = np.zeros(sample_count) if query_mask else None
                for i in range(iter_n):
                    head, tail = i * bs, min((i + 1) * bs, sample_count)
                    chunk = coord[head:tail].to(dev)
                    if query_sdf or query_mask:
                        sdf, mask = query_points_device(self.octree, self.geo_decoder, chunk, check_level, True, query_sdf,
                                                        query_mask, mlp)
                    if query_sdf:
                        sdf_pred[head:tail] = sdf.cpu().numpy()
                    if query_sem:
                        sem_pred[head:tail] = query_labels_device(self.octree, self.sem_decoder, chunk).cpu().numpy()
                    if query_mask:
                        mc_mask[head:tail] = mask.cpu().numpy()
            else:
                sdf = mask = None
                if query_sdf or query_mask:
                    sdf, mask = query_points_device(self.octree, self.geo_decoder, coord.to(dev), check_level, True,
                                                    query_sdf, query_mask, mlp)
                sdf_pred = sdf.cpu().numpy() if query_sdf else None
                # (the reference's unchunked branch returns the int64 array of .cpu().numpy(), :98)
                sem_pred = query_labels_device(self.octree, self.sem_decoder, coord.to(dev)).cpu().numpy() if query_sem else None
                mc_mask = mask.cpu().numpy() if query_mask else None
        return sdf_pred, sem_pred, mc_mask

    # ------------------------------------------------------------------------------------------------ utils/mesher.py:153-367
    def generate_sdf_map(self, coord, sdf_pred, mc_mask, map_path):
        """utils/mesher.py:153-175: the query grid as a point cloud (world metres), the SDF in metres as `intensities`, the mask
        as `labels`, after global_transform; written as binary PLY."""
        # (coord /= world_scale in the reference: float32)
        pts = (coord.detach() / self.world_scale).cpu().numpy().astype(np.float64) if torch.is_tensor(coord) else \
            (np.asarray(coord, np.float32) / np.float32(self.world_scale)).astype(np.float64)
        sdf_world = np.asarray(sdf_pred, np.float64) * self.config.logistic_gaussian_ratio * self.config.sigma_sigmoid_m
        T = np.asarray(self.global_transform, np.float64)
        pts = pts @ T[:3, :3].T + T[:3, 3]
        props = [("x", pts[:, 0], "float"), ("y", pts[:, 1], "float"), ("z", pts[:, 2], "float"),
                 ("intensities", sdf_world, "float")]
        if mc_mask is not None:
            props.append(("labels", np.asarray(mc_mask).astype(np.int32), "int"))
        write_ply(map_path, props)
        print("save the sdf map to %s" % (map_path))

    def assign_to_bbx(self, sdf_pred, sem_pred, mc_mask, voxel_num_xyz):
        """utils/mesher.py:177-198: the flat query results as [X,Y,Z] grids (numpy or device tensors alike)."""
        shape = tuple(int(v) for v in voxel_num_xyz)
        if sdf_pred is not None:
            sdf_pred = sdf_pred.reshape(shape)
        if sem_pred is not None:
            sem_pred = sem_pred.reshape(shape)
        if mc_mask is not None:
            mc_mask = mc_mask.reshape(shape).bool() if torch.is_tensor(mc_mask) else mc_mask.reshape(shape).astype(dtype=bool)
        return sdf_pred, sem_pred, mc_mask

    def mc_mesh(self, mc_sdf, mc_mask, voxel_size, mc_origin):
        """utils/mesher.py:200-222 with marching_cubes (csrc/shine_mc.hip) at level 0 in place of skimage's: numpy or device
        grids in, (verts = mc_origin + verts * voxel_size float64 numpy, faces int32 numpy) out; an empty surface gives empty
        arrays."""
        verts, faces = self._mc_device(mc_sdf, mc_mask)
        verts = np.asarray(mc_origin, np.float64) + verts.double().cpu().numpy() * voxel_size
        return verts, faces.cpu().numpy()

    def _mc_device(self, mc_sdf, mc_mask):
        dev = self.octree.hier_features[0].device if len(self.octree.hier_features) else torch.device("cuda")
        sdf = torch.as_tensor(np.asarray(mc_sdf, np.float32) if not torch.is_tensor(mc_sdf) else mc_sdf).to(dev, torch.float32)
        mask = None
        if mc_mask is not None:
            mask = torch.as_tensor(np.asarray(mc_mask, bool) if not torch.is_tensor(mc_mask) else mc_mask).to(dev)
        return marching_cubes(sdf, mask, 0.0)

    def estimate_vertices_sem(self, mesh, verts, filter_free_space_vertices=True):
        """utils/mesher.py:224-238: vertex labels (shine_sem_query_labels), colours from the reference's colour map or the
        config's, then the free-space vertices (label <= 0) removed with their triangles."""
        dev = self.octree.hier_features[0].device
        v = torch.as_tensor(np.asarray(verts, np.float64), device=dev)
        f = torch.as_tensor(np.asarray(mesh.triangles, np.int32), device=dev)
        v, f, labels, colors = self._sem_device(v, f, filter_free_space_vertices)
        out = _make_mesh(v.cpu().numpy(), f.cpu().numpy(), None, colors.cpu().numpy() if colors is not None else None)
        if isinstance(out, TriangleMesh):
            out.vertex_labels = labels.cpu().numpy()
        return out

    def _sem_device(self, verts, faces, filter_free_space_vertices):
        labels = query_labels_device(self.octree, self.sem_decoder, (verts * self.world_scale).float())
        cmap = _sem_color_map(self.config)
        colors = None
        if cmap is not None:
            rows = max(max(int(k) for k in cmap), int(getattr(self.config, "sem_class_count", 0))) + 1  # (a class without a colour: black)
            lut = np.zeros((rows, 3), np.float64)
            for k, c in cmap.items():
                lut[int(k)] = np.asarray(c, np.float64) / 255.0
            colors = torch.as_tensor(lut, device=verts.device)[labels]
        if filter_free_space_vertices:
            verts, faces, labels, colors = remove_vertices_device(verts, faces, labels <= 0, labels, colors)
        return verts, faces, labels, colors

    def filter_isolated_vertices(self, mesh, filter_cluster_min_tri=300):
        """utils/mesher.py:240-251: drop the triangles of edge-connected clusters with fewer than filter_cluster_min_tri
        triangles (shine_mesh_cluster_filter); vertices are kept."""
        dev = self.octree.hier_features[0].device
        f = torch.as_tensor(np.asarray(mesh.triangles, np.int32), device=dev)
        kept = cluster_filter_device(f, filter_cluster_min_tri).cpu().numpy()
        o3d = _open3d()
        mesh.triangles = o3d.utility.Vector3iVector(kept) if o3d is not None and not isinstance(mesh, TriangleMesh) else kept
        return mesh

    def _finish(self, verts, faces, voxel_size, origin, mesh_path, estimate_sem, estimate_normal, filter_isolated_mesh,
                filter_free_space_vertices, min_tri):
        """the tail of recon_bbx_mesh / recon_octree_mesh (utils/mesher.py:270-292, :344-367) on device arrays: world
        coordinates, [semantics], [normals], [cluster filter], global_transform, PLY."""
        dev = verts.device
        v = torch.as_tensor(np.asarray(origin, np.float64), device=dev) + verts.double() * float(voxel_size)
        f = faces
        labels = colors = normals = None
        if estimate_sem:
            v, f, labels, colors = self._sem_device(v, f, filter_free_space_vertices)
        if estimate_normal:
            normals = vertex_normals_device(v, f)
        if filter_isolated_mesh:
            f = cluster_filter_device(f, min_tri)
        v, normals = _transform_device(v, normals, self.global_transform)
        self.last_mesh_device = (v, f)  # fp64 vertices + int32 faces, still on the device (evaluation.eval_mesh takes the pair)
        vn, fn = v.cpu().numpy(), f.cpu().numpy()
        nn = normals.cpu().numpy() if normals is not None else None
        cn = colors.cpu().numpy() if colors is not None else None
        props = [("x", vn[:, 0], "double"), ("y", vn[:, 1], "double"), ("z", vn[:, 2], "double")]
        if nn is not None:
            props += [("nx", nn[:, 0], "double"), ("ny", nn[:, 1], "double"), ("nz", nn[:, 2], "double")]
        if cn is not None:
            rgb = np.clip(np.round(cn * 255.0), 0, 255).astype(np.uint8)
            props += [("red", rgb[:, 0], "uchar"), ("green", rgb[:, 1], "uchar"), ("blue", rgb[:, 2], "uchar")]
        if mesh_path is not None:  # (update_octree_mesh may be asked for the arrays only)
            write_ply(mesh_path, props, fn)
            print("save the mesh to %s\n" % (mesh_path))
        mesh = _make_mesh(vn, fn, nn, cn)
        if isinstance(mesh, TriangleMesh) and labels is not None:
            mesh.vertex_labels = labels.cpu().numpy()
        return mesh

    def _fill_grid(self, coord, shape, check_level, query_mask):
        """query_points_device over `coord` in chunks, straight into a device sdf grid and mask grid"""
        n = coord.shape[0]
        dev = self.octree.hier_features[0].device
        sdf = torch.empty(n, dtype=torch.float32, device=dev)
        mask = torch.empty(n, dtype=torch.bool, device=dev) if query_mask else None
        mlp = self._decoder_params()
        with torch.no_grad():
            for head in range(0, n, QUERY_CHUNK):
                tail = min(head + QUERY_CHUNK, n)
                s, m = query_points_device(self.octree, self.geo_decoder, coord[head:tail].to(dev), check_level, True, True,
                                           query_mask, mlp)
                sdf[head:tail] = s
                if query_mask:
                    mask[head:tail] = m
        return sdf.view(shape), (mask.view(shape) if mask is not None else None)

    def _check_level(self):
        return min(self.octree.featured_level_num, self.config.mc_vis_level) - 1

    def _decoder_params(self):
        """what query_points_device decodes with: None (the decoder's own six tensors) or, with config.time_conditioned, the head
        at self.ts (utils/mesher.py:29,71-74,94-97) folded into an 8-wide decoder.  Asked for once per public call, before its
        chunks: self.ts is read at call time and the fold is two small torch ops."""
        if getattr(self.config, "time_conditioned", False):
            return self.geo_decoder.fused_params_at(self.ts)
        return None

    def _bbx_layout(self, bbx, voxel_size):
        """utils/mesher.py:113-121: the box grid, padded, one extra layer underground: (shape [3], voxel_origin [3] metres)"""
        min_bound = np.asarray(bbx.get_min_bound(), dtype=np.float64).copy()
        max_bound = np.asarray(bbx.get_max_bound(), dtype=np.float64)
        shape = (np.ceil((max_bound - min_bound) / voxel_size) + self.config.pad_voxel * 2).astype(np.int_)
        voxel_origin = min_bound - self.config.pad_voxel * voxel_size
        voxel_origin[2] -= voxel_size
        shape[2] += 1
        return shape, voxel_origin

    def bbx_bricks_device(self, bbx, voxel_size):
        """recon_bbx_mesh's grid as bricks: the BOX_BRICK^3 tiles that may hold a point whose node exists at the mask's check
        level (box_candidate_tiles) plus their upper neighbours, each queried at its own points with get_query_from_bbx's fp32
        arithmetic — so every value a processed cube reads is the dense grid's, bit for bit.  Returns (values [n,B,B,B] f32, mask
        [n,B,B,B] u8, origins [n,3] int64, shape, voxel_origin)."""
        shape, voxel_origin = self._bbx_layout(bbx, voxel_size)
        B = BOX_BRICK
        dev = self.octree.hier_features[0].device
        check_level = self._check_level()
        level = self.octree.max_level - check_level
        node_res_scaled = 2 ** (1 - level)
        tiles = box_candidate_tiles(self.octree.get_octree_nodes(level), node_res_scaled, self.world_scale, voxel_origin, voxel_size,
                                    shape, B)
        tiles = with_upper_neighbours(tiles, (np.asarray(shape, np.int64) + B - 1) // B)
        origins = tiles * B
        n = len(origins)
        values = torch.empty((n, B, B, B), dtype=torch.float32, device=dev)
        mask = torch.zeros((n, B, B, B), dtype=torch.uint8, device=dev)
        ax = torch.arange(B, dtype=torch.int64, device=dev)
        gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
        local = torch.stack((gx.flatten(), gy.flatten(), gz.flatten()), 1)
        org_dev = torch.as_tensor(origins, device=dev)
        top = torch.as_tensor(np.asarray(shape, np.int64) - 1, device=dev)
        origin_t = torch.tensor(voxel_origin, dtype=self.dtype, device=dev)
        per = max(1, QUERY_CHUNK // (B ** 3))
        mlp = self._decoder_params()
        with torch.no_grad():
            for h in range(0, n, per):
                t = min(h + per, n)
                # (points of a tile beyond the grid are never read: they are queried at the grid's last point)
                idx = torch.minimum(org_dev[h:t, None, :] + local[None], top).reshape(-1, 3)
                coord = idx.float()  # get_query_from_bbx: int16 indices -> float32, * voxel_size, + origin, * world_scale
                coord *= voxel_size
                coord += origin_t
                coord *= self.world_scale
                s, m = query_points_device(self.octree, self.geo_decoder, coord, check_level, True, True, True, mlp)
                values[h:t] = s.view(-1, B, B, B)
                mask[h:t] = m.view(-1, B, B, B)
        return values, mask, origins, tuple(int(v) for v in shape), voxel_origin

    def _recon(self, sparse, fits_shape, per_point_extra, dense_fn, brick_fn, *finish):
        """what recon_bbx_mesh and recon_octree_mesh share: the route (`sparse` None: bricks iff the dense grid of fits_shape(), a
        shape or None for "do not ask", does not fit), the route's marching cubes — dense_fn / brick_fn return (verts, faces,
        voxel size m, origin m) — and _finish with its remaining arguments `finish`."""
        if sparse is None:
            shape = fits_shape()
            if shape is not None:
                try:
                    ensure_grid_fits(shape, True, per_point_extra, device=self.octree.hier_features[0].device)
                except MemoryError:
                    sparse = True
        verts, faces, voxel, origin = brick_fn() if sparse else dense_fn()
        return self._finish(verts, faces, voxel, origin, *finish)

    def recon_bbx_mesh(self, bbx, voxel_size, mesh_path, map_path, save_map=False, estimate_sem=False, estimate_normal=True,
                       filter_isolated_mesh=True, filter_free_space_vertices=True, sparse=None):
        """utils/mesher.py:253-292 on the device: grid query -> marching cubes -> [semantics] -> [normals] -> [filter with
        config.min_cluster_vertices] -> global_transform -> PLY.  `sparse`: False = the dense grid (MemoryError when it does
        not fit), True = bricks (bbx_bricks_device + marching_cubes_sparse: the same mesh, memory proportional to the tiles
        near the map's nodes), None = dense when it fits, else bricks.  The brick route needs config.mc_mask_on and cannot
        save the SDF map."""
        mask_on = bool(getattr(self.config, "mc_mask_on", True))
        extra = 12 + 6  # per point, next to the grid: the query coordinates and get_query_from_bbx's int16 axes

        def bricks():
            if not mask_on:
                raise ValueError("recon_bbx_mesh: sparse=True needs config.mc_mask_on (without the mask every cube of the box is "
                                 "processed, so no tile can be left out)")
            if save_map:
                raise ValueError("recon_bbx_mesh: save_map=True cannot be combined with the brick route (sparse=True, or a box "
                                 "whose dense grid does not fit): there is no sparse SDF map")
            values, mask, origins, shape, voxel_origin = self.bbx_bricks_device(bbx, voxel_size)
            return marching_cubes_sparse(values, mask, origins, shape, 0.0) + (voxel_size, voxel_origin)

        def dense():
            ensure_grid_fits(self._bbx_layout(bbx, voxel_size)[0], mask_on, extra, device=self.octree.hier_features[0].device)
            coord, voxel_num_xyz, voxel_origin = self.get_query_from_bbx(bbx, voxel_size)
            sdf, mask = self._fill_grid(coord, tuple(int(v) for v in voxel_num_xyz), self._check_level(), mask_on)
            if save_map:
                self.generate_sdf_map(coord, sdf.reshape(-1).cpu().numpy(),
                                      mask.reshape(-1).cpu().numpy() if mask is not None else None, map_path)
            del coord
            return marching_cubes(sdf, mask, 0.0) + (voxel_size, voxel_origin)

        return self._recon(sparse, lambda: self._bbx_layout(bbx, voxel_size)[0] if mask_on else None, extra, dense, bricks,
                           mesh_path, estimate_sem, estimate_normal, filter_isolated_mesh, filter_free_space_vertices,
                           getattr(self.config, "min_cluster_vertices", 300))

    def octree_grid_layout(self, query_level, mc_res_m):
        """utils/mesher.py:297-321's arithmetic (numpy, the reference's op order): (node centres [M,3] scaled, node_res_scaled,
        voxels per node side k, mc_res_scaled, grid shape [3], shift_coord [M,3] = each node block's offset in the grid)."""
        nodes = self.octree.get_octree_nodes(query_level)
        if len(nodes) == 0:
            raise ValueError("recon_octree_mesh: the octree has no node at level %d" % query_level)
        min_nodes = np.min(nodes, 0)
        max_nodes = np.max(nodes, 0)
        node_res_scaled = 2 ** (1 - query_level)
        k = int(np.ceil(node_res_scaled / self.world_scale / mc_res_m).astype(dtype=int))
        mc_res_scaled = node_res_scaled / k
        shape = ((max_nodes - min_nodes) / mc_res_scaled + k).astype(int)
        shift = ((nodes - min_nodes) / node_res_scaled * k).astype(int)
        return nodes, node_res_scaled, k, mc_res_scaled, shape, shift

    def _octree_blocks(self, query_level, mc_res_m):
        """The node blocks of get_octree_nodes(query_level), every block queried at once per chunk of nodes instead of one query
        per node (utils/mesher.py:326-337).  Returns (k, grid shape [3], shift_coord [M,3], voxel size m, origin m, chunks);
        `chunks` yields (h, t, sdf, mask) for the nodes h..t-1: the blocks' (t - h) * k^3 values, block-major and (x, y, z)
        inside a block, and their mask, None with config.mc_mask_on off.  The reference keeps its grid as float16 (:323); the
        values are rounded the same way (.half().float()) so the meshes agree."""
        nodes, node_res_scaled, k, mc_res_scaled, shape, shift, voxel, origin = self._block_layout(query_level, mc_res_m)
        return k, shape, shift, voxel, origin, self._query_blocks(nodes, node_res_scaled, k, mc_res_scaled)

    def _block_layout(self, query_level, mc_res_m):
        """octree_grid_layout plus the grid's (voxel size m, origin m)"""
        nodes, node_res_scaled, k, mc_res_scaled, shape, shift = self.octree_grid_layout(query_level, mc_res_m)
        voxel = mc_res_scaled / self.world_scale
        origin = (np.min(nodes, 0) - 0.5 * (node_res_scaled - mc_res_scaled)) / self.world_scale
        return nodes, node_res_scaled, k, mc_res_scaled, shape, shift, voxel, origin

    def _query_blocks(self, nodes, node_res_scaled, k, mc_res_scaled):
        """The k^3 blocks of the nodes with centres `nodes [m,3]` (scaled), queried QUERY_CHUNK points at a time: yields (h, t, sdf,
        mask) as _octree_blocks documents.  A block's values depend on its own node only: on no other row of `nodes`, and not on
        the grid's origin."""
        dev = self.octree.hier_features[0].device
        # the reference's node block: int16 grid coordinates, float32, times mc_res_scaled (:304-313)
        ax = torch.arange(k, dtype=torch.int16, device=dev)
        gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
        block = torch.stack((gx.flatten(), gy.flatten(), gz.flatten())).transpose(0, 1).float()
        block *= mc_res_scaled
        block64 = block.double()
        origins = torch.as_tensor(nodes - 0.5 * (node_res_scaled - mc_res_scaled), dtype=torch.float64, device=dev)
        mask_on = bool(getattr(self.config, "mc_mask_on", True))
        check_level = self._check_level()
        per = max(1, QUERY_CHUNK // (k ** 3))
        mlp = self._decoder_params()
        for h in range(0, len(nodes), per):
            t = min(h + per, len(nodes))
            # cur_coord += cur_origin (:329-330): a float32 tensor plus a float64 one, computed in double, stored as float32
            coord = (block64[None] + origins[h:t, None, :]).float().reshape(-1, 3)
            with torch.no_grad():
                s, m = query_points_device(self.octree, self.geo_decoder, coord, check_level, True, True, mask_on, mlp)
            yield h, t, s.half().float(), m

    def octree_grid_device(self, query_level, mc_res_m):
        """recon_octree_mesh's dense grid, assembled on the device: every node block (_octree_blocks) scattered to its shift_coord
        offset.  Unfilled cells stay 0 with the mask off.  Returns (sdf [X,Y,Z] f32, mask [X,Y,Z] bool, voxel size m, origin m)."""
        k, shape, shift, voxel, origin, chunks = self._octree_blocks(query_level, mc_res_m)
        dev = self.octree.hier_features[0].device
        ensure_grid_fits(shape, True, device=dev)
        X, Y, Z = (int(v) for v in shape)
        ax = torch.arange(k, dtype=torch.int64, device=dev)
        lin_block = ((ax[:, None, None] * Y + ax[None, :, None]) * Z + ax[None, None, :]).reshape(-1)
        base = torch.as_tensor((shift[:, 0].astype(np.int64) * Y + shift[:, 1]) * Z + shift[:, 2], device=dev)
        sdf = torch.zeros(X * Y * Z, dtype=torch.float32, device=dev)
        mask = torch.zeros(X * Y * Z, dtype=torch.bool, device=dev)
        for h, t, s, m in chunks:
            idx = (base[h:t, None] + lin_block[None]).reshape(-1)
            sdf[idx] = s
            if m is not None:  # (without the mask the reference assigns None, i.e. False, to its bool grid: :336)
                mask[idx] = m
        return sdf.view(X, Y, Z), mask.view(X, Y, Z), voxel, origin

    def octree_bricks_device(self, query_level, mc_res_m):
        """octree_grid_device's grid as bricks: every node block (_octree_blocks) KEPT as a brick instead of being scattered into
        a dense grid, which is never allocated.  Blocks wider than MC_SPARSE_MAX_BRICK are cut into bricks of brick_edge(k).
        Returns (values [n,B,B,B] f32, mask [n,B,B,B] u8, origins [n,3] int64, shape, voxel size m, origin m)."""
        k, shape, shift, voxel, origin, chunks = self._octree_blocks(query_level, mc_res_m)
        dev = self.octree.hier_features[0].device
        values = torch.empty((len(shift), k, k, k), dtype=torch.float32, device=dev)
        mask = torch.zeros((len(shift), k, k, k), dtype=torch.uint8, device=dev)
        for h, t, s, m in chunks:
            values[h:t] = s.view(-1, k, k, k)
            if m is not None:
                mask[h:t] = m.view(-1, k, k, k)
        return self._blocks_as_bricks(values, mask, shape, shift) + (voxel, origin)

    @staticmethod
    def _blocks_as_bricks(values, mask, shape, shift):
        """node blocks [M, k, k, k] at grid offsets `shift` as marching_cubes_sparse's (values, mask, origins, shape)"""
        B, brick_origins = octree_brick_table(values.shape[1], shift)
        return split_blocks(values, B), split_blocks(mask, B), brick_origins, tuple(int(v) for v in shape)

    def reset_mesh_cache(self):
        """Drop update_octree_mesh's cache: its next call queries every block again (reason "first")."""
        self._mesh_cache = None

    def update_octree_mesh(self, query_level, mc_res_m, mesh_path=None, estimate_sem=False, estimate_normal=True,
                           filter_isolated_mesh=True, filter_free_space_vertices=True):
        """recon_octree_mesh(..., sparse=True) on the octree's current state — the same vertices, faces, order, normals, colours
        and PLY bytes — from a block cache that persists between calls: only the node blocks whose values can have changed since the
        previous call are queried again (changed feature rows -> dirty nodes -> dirty query-level nodes, all on
        the device).  Marching cubes and the mesh's tail still run over everything.  mesh_path None writes no file; the mesh is
        left in last_mesh_device either way, and last_update_stats says what was queried: nodes, new_nodes, dirty_nodes,
        requeried_nodes, requeried_points, full, reason ("first" / "key" / "decoder" / "octree" when the cache was rebuilt from
        nothing, else None), and changed_rows per level, the count shine_rows_diff leaves next to them.  The cache costs the size of the feature tables plus 5 bytes per grid point."""
        if getattr(self.config, "time_conditioned", False):
            raise NotImplementedError("update_octree_mesh keeps one block cache, not one per time stamp: mesh a time-conditioned "
                                      "map with recon_octree_mesh")
        try:
            return self._update_octree_mesh(query_level, mc_res_m, mesh_path, estimate_sem, estimate_normal, filter_isolated_mesh,
                                            filter_free_space_vertices)
        except BaseException:
            self._mesh_cache = None  # (a call that stopped half-way leaves snapshots ahead of the blocks)
            raise

    def _update_octree_mesh(self, query_level, mc_res_m, *finish):
        octree = self.octree
        nodes, node_res_scaled, k, mc_res_scaled, shape, shift, voxel, origin = self._block_layout(query_level, mc_res_m)
        dev = octree.hier_features[0].device
        L, sq = octree.featured_level_num, query_level - octree.free_level_num
        feats = [p.detach() for p in octree.feature_list()]
        if not all(f.is_cuda and f.dtype == torch.float32 and f.is_contiguous() for f in feats):
            raise ValueError("update_octree_mesh: the feature tables must be CUDA float32 contiguous")
        rows = [int(f.shape[0]) - 1 for f in feats]  # without the trash row
        # (octree_grid_layout's get_octree_nodes merged the device's growth into the host tables)
        node_keys, node_ids = list(octree._node_keys), list(octree._node_ids)
        counts = [len(a) for a in node_keys]
        M = counts[sq]
        key = mesh_cache_key(query_level, k, mc_res_scaled, bool(getattr(self.config, "mc_mask_on", True)), self._check_level(),
                             self.world_scale)
        decoder_bits = torch.cat([p.detach().reshape(-1) for p in self.geo_decoder.fused_params()]).view(torch.int32)
        c = self._mesh_cache
        reason = mesh_cache_rebuild_reason(c, key, lambda: torch.equal(c.decoder_bits, decoder_bits), node_keys, node_ids, rows)
        if reason is not None:  # from nothing: an empty snapshot and no node seen make every row changed and every node new
            c = self._mesh_cache = _MeshCache(key, decoder_bits, L)
        prev = [len(a) for a in c.node_keys]

        # the feature rows that changed since the previous call (and the snapshot brought up to date)
        flags = [torch.empty(r, dtype=torch.uint8, device=dev) for r in rows]
        counters = torch.zeros(L + 2, dtype=torch.int64, device=dev)  # changed rows per level, then mark_dirty's two counts
        for s in range(L):
            c.snaps[s] = _grow_rows(c.snaps[s], c.snap_rows[s], rows[s], (_lib.FEATURE_DIM,), torch.float32, dev)
        rows_diff_device(feats, c.snaps, c.snap_rows, flags, counters[:L])
        c.snap_rows = rows

        # the node tables on the device (appended), the sorted keys of the slots the search runs in, the dirty query nodes
        for s in range(L):
            n0, n1 = c.dev_nodes[s], counts[s]
            c.dev_keys[s] = _grow_rows(c.dev_keys[s], n0, n1, (), torch.int64, dev)
            c.dev_ids[s] = _grow_rows(c.dev_ids[s], n0, n1, (8,), torch.int32, dev)
            if n1 > n0:
                c.dev_keys[s][n0:n1] = torch.from_numpy(node_keys[s][n0:n1]).to(dev)
                c.dev_ids[s][n0:n1] = torch.from_numpy(np.ascontiguousarray(node_ids[s][n0:n1], np.int32)).to(dev)
            c.dev_nodes[s] = n1
            if s <= sq and (c.sorted[s] is None or c.sorted[s][0] != n1):
                c.sorted[s] = (n1,) + tuple(torch.sort(c.dev_keys[s][:n1]))
        dirty = torch.empty(M, dtype=torch.uint8, device=dev)
        mark_dirty_device(sq, c.dev_keys, c.dev_ids, counts, prev, flags, [e[1] if e else None for e in c.sorted],
                          [e[2] if e else None for e in c.sorted], dirty, counters[L:])
        index = torch.nonzero(dirty).reshape(-1)
        index_host = index.cpu().numpy()
        counted = [int(v) for v in counters.tolist()]
        changed_rows, old_dirty, all_dirty = counted[:L], counted[L], counted[L + 1]
        if all_dirty != len(index_host) or all_dirty != (M - prev[sq]) + old_dirty or (reason is not None and all_dirty != M):
            raise RuntimeError("update_octree_mesh: %d flagged blocks, %d counted (%d of them old), %d nodes, %d seen before "
                               "(rebuilt: %s)" % (len(index_host), all_dirty, old_dirty, M, prev[sq], reason))

        # the dirty and the new blocks, queried as _octree_blocks queries them, written into the cache
        chunks = self._query_blocks(nodes[index_host], node_res_scaled, k, mc_res_scaled)
        c.values = _grow_rows(c.values, prev[sq], M, (k, k, k), torch.float32, dev)
        c.masks = _grow_rows(c.masks, prev[sq], M, (k, k, k), torch.uint8, dev)
        for h, t, s, m in chunks:
            blocks_scatter_device(s, m, index[h:t], c.values, c.masks)
        c.node_keys, c.node_ids = node_keys, node_ids
        self.last_update_stats = {
            "nodes": M, "new_nodes": M - prev[sq], "dirty_nodes": old_dirty, "requeried_nodes": all_dirty,
            "requeried_points": all_dirty * k ** 3, "full": reason is not None, "reason": reason, "changed_rows": changed_rows,
        }
        verts, faces = marching_cubes_sparse(*self._blocks_as_bricks(c.values[:M], c.masks[:M], shape, shift), 0.0)
        return self._finish(verts, faces, voxel, origin, *finish, 300)

    def recon_octree_mesh(self, query_level, mc_res_m, mesh_path, map_path, save_map=False, estimate_sem=False,
                          estimate_normal=True, filter_isolated_mesh=True, filter_free_space_vertices=True, sparse=None):
        """utils/mesher.py:294-367 on the device (the reference's save_map is commented out there, :342-344, and ignored here
        too; its cluster filter uses the default 300 triangles, :356).  `sparse`: False = the dense grid over the nodes'
        bounding box (MemoryError when it does not fit), True = the node blocks as bricks (octree_bricks_device +
        marching_cubes_sparse: the same mesh, memory proportional to the nodes), None = dense when it fits, else bricks."""
        def bricks():
            values, mask, origins, shape, voxel, origin = self.octree_bricks_device(query_level, mc_res_m)
            return marching_cubes_sparse(values, mask, origins, shape, 0.0) + (voxel, origin)

        def dense():
            sdf, mask, voxel, origin = self.octree_grid_device(query_level, mc_res_m)
            return marching_cubes(sdf, mask, 0.0) + (voxel, origin)

        return self._recon(sparse, lambda: self.octree_grid_layout(query_level, mc_res_m)[4], 0, dense, bricks, mesh_path,
                           estimate_sem, estimate_normal, filter_isolated_mesh, filter_free_space_vertices, 300)
