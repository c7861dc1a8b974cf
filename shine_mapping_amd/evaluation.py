"""The reference's mesh evaluation (eval/eval_utils.py: eval_mesh, nn_correspondance, crop_intersection) on the device.

    from shine_mapping_amd.evaluation import eval_mesh
    metrics = eval_mesh("mesh.ply", "gt_cloud.ply", down_sample_res=0.02, threshold=0.1, truncation_acc=0.2, truncation_com=2.0)

    python -m shine_mapping_amd.evaluation PRED.ply GT.ply [--spacing --threshold --trunc-acc --trunc-com --no-bbx-mask
                                                             --samples --seed --csv OUT.csv]

Every stage is a device function of csrc/shine_eval.hip with a wrapper here, all geometry in fp64: `crop_mesh`,
`sample_points_uniformly`, `voxel_down_sample`, `nn_correspondence` (the hot path: a two-level uniform grid over the reference
set, one query per lane) and the metric sums.  open3d is not needed: `read_ply` and `mesher.write_ply` are
plain numpy.  There is no CPU path: every stage raises without the HIP library and a device.

Differences from the reference, all deliberate:
  * the sample points come from a counter-based generator keyed by (seed, sample), not from open3d's Mersenne stream, and the
    down-sampled clouds are ordered by ascending voxel key (open3d's order is that of a hash map): the metrics are means over
    the clouds, so neither changes what is measured, but single runs differ from the reference's in the sampling noise;
  * `down_sample_res <= 0` means "no down-sampling" (the reference hits an undefined name there);
  * a query without a reference point inside the truncation has index -1 (the reference reports its out-of-range neighbour).
"""
from __future__ import annotations

import argparse
import collections
import csv
import ctypes as C
import math
import sys

import numpy as np

from . import _lib

METRIC_KEYS = ["MAE_accuracy (m)", "MAE_completeness (m)", "Chamfer_L1 (m)", "Chamfer_L2 (m)", "Precision [Accuracy] (%)",
               "Recall [Completeness] (%)", "F-score (%)", "Spacing (m)", "Inlier_threshold (m)", "Outlier_truncation_acc (m)",
               "Outlier_truncation_com (m)"]

# the search grid (csrc/shine_eval.hip): fine cells of edge CELL_FACTOR x (mean spacing of the reference set), grouped
# FINE_PER_COARSE^3 into the coarse cells the walk probes (DESIGN.md §3.10 has the measurements behind the values)
CELL_FACTOR = 3.0
FINE_PER_COARSE = 4
AXIS_BITS = 21

NNResult = collections.namedtuple("NNResult", "index dist keep indices distances max_coarse_cells max_fine_cells cell")


def _torch():
    import torch

    return torch


def _stream():
    return _lib.current_stream_handle()


def _device(device=None):
    torch = _torch()
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise _lib.ShineHipError("shine_mapping_amd.evaluation runs on the device only (no GPU is visible; there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def _points(x, device=None):
    """[n,3] fp64 contiguous on the device (device tensors of that form are used in place)."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        dev = x.device if x.is_cuda else _device(device)
        t = x.detach().to(device=dev, dtype=torch.float64)
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(_device(device))
    if t.numel() == 0:
        t = t.reshape(0, 3)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("expected an [n,3] array of points, got shape %s" % (tuple(t.shape),))
    return t.contiguous()


def _faces(x, device):
    torch = _torch()
    if isinstance(x, torch.Tensor):
        t = x.detach().to(device=device, dtype=torch.int32)
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.int32))).to(device)
    if t.numel() == 0:
        t = t.reshape(0, 3)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("expected an [f,3] array of triangles, got shape %s" % (tuple(t.shape),))
    return t.contiguous()


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _host_points(x):
    """the array itself if it lives on the host (bounds of host input are taken before the upload), else None"""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return x.detach().double().numpy().reshape(-1, 3) if not x.is_cuda else None
    return np.asarray(x, dtype=np.float64).reshape(-1, 3)


def bounds(points):
    """Per-axis (min, max) of a cloud as two numpy [3] arrays (device reduction for device input)."""
    host = _host_points(points)
    if host is not None:
        if len(host) == 0:
            raise ValueError("bounds of an empty cloud")
        return host.min(0), host.max(0)
    pts = _points(points)
    if pts.shape[0] == 0:
        raise ValueError("bounds of an empty cloud")
    torch = _torch()
    out = torch.empty(6, dtype=torch.float64, device=pts.device)
    _lib.call_with_workspace(_lib.lib().shine_eval_bounds, pts.device, pts.data_ptr(), pts.shape[0], _lib.WS, _lib.WS_BYTES,
                             out.data_ptr(), _stream())
    b = out.cpu().numpy()
    return b[:3].copy(), b[3:].copy()


def crop_mesh(verts, faces, min_bound, max_bound):
    """open3d's TriangleMesh.crop with an axis-aligned box: keep the vertices with min <= p <= max on every axis (inclusive),
    the triangles whose three vertices are kept, re-indexed.  Returns device (verts [v,3] f64, faces [f,3] int32)."""
    from .mesher import remove_vertices_device

    torch = _torch()
    v = _points(verts)
    f = _faces(faces, v.device)
    drop = torch.zeros(v.shape[0], dtype=torch.uint8, device=v.device)
    _lib.check(_lib.lib().shine_eval_box_mask(v.data_ptr() if v.shape[0] else None, v.shape[0], _d3(min_bound), _d3(max_bound),
                                              drop.data_ptr() if v.shape[0] else None, _stream()), "shine_eval_box_mask")
    nv, nf = remove_vertices_device(v, f, drop)
    return nv.contiguous(), nf.reshape(-1, 3).contiguous()


def sample_points_uniformly(verts, faces, n, seed=0, uniforms=None, return_triangles=False):
    """open3d's sample_points_uniformly: `n` points on the mesh, area-weighted.  Sample i takes three uniforms (u0, u1, u2) in
    [0,1): its triangle is the first whose cumulative area share (fp64 inclusive prefix sum over the total) is > u0 — a
    zero-area triangle is never chosen — and the point is (1 - sqrt u1) v0 + sqrt u1 (1 - u2) v1 + sqrt u1 u2 v2.  The uniforms
    come from a counter-based generator keyed by (seed, i) — NOT open3d's Mersenne stream; the same seed gives the same bits on
    every run and for every launch geometry — or from `uniforms` [n,3] fp64.  Returns [n,3] fp64 on the device (and the int32
    triangle of every sample with return_triangles)."""
    torch = _torch()
    v = _points(verts)
    f = _faces(faces, v.device)
    n = int(n)
    if n < 0:
        raise ValueError("sample_points_uniformly: n must be >= 0")
    if f.shape[0] == 0 and n > 0:
        raise ValueError("sample_points_uniformly: the mesh has no triangles")
    u = None
    if uniforms is not None:
        u = _points(uniforms, v.device)
        if u.shape[0] != n:
            raise ValueError("sample_points_uniformly: uniforms must be [n,3]")
    out = torch.empty((n, 3), dtype=torch.float64, device=v.device)
    tri = torch.empty(n, dtype=torch.int32, device=v.device) if return_triangles else None
    if n:
        _lib.call_with_workspace(_lib.lib().shine_eval_sample_mesh, v.device, v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], n,
                                 int(seed) & (2 ** 64 - 1), u.data_ptr() if u is not None else None, _lib.WS, _lib.WS_BYTES,
                                 out.data_ptr(), tri.data_ptr() if tri is not None else None, _stream())
    return (out, tri) if return_triangles else out


def _check_axis_bits(lo, hi, origin, cell, what):
    cells = np.floor((np.asarray(hi, np.float64) - origin) / cell) + 1
    if not np.all(np.isfinite(cells)) or cells.max() > 2 ** AXIS_BITS:
        raise ValueError("%s: the cloud spans %s cells of %g m per axis, more than the %d-bit cell index holds (2^%d); "
                         "use a larger cell" % (what, cells.tolist(), cell, AXIS_BITS, AXIS_BITS))
    return cells.astype(np.int64)


def voxel_down_sample(points, voxel, return_keys=False, attrs=None):
    """open3d's voxel_down_sample: one point per occupied voxel, the mean (fp64 sums) of the voxel's points.  The voxel index is
    floor((p - (min_bound - voxel/2)) / voxel) per axis with min_bound the cloud's own minimum; the output is ordered by
    ascending voxel key (ix << 42 | iy << 21 | iz) — open3d's order is that of a hash map — and is bit-identical from run to
    run.  Refuses clouds that need more than 21 bits per axis.  Returns [m,3] fp64 on the device (and the uint64 keys as int64
    with return_keys).  attrs: [n] or [n,a] (a = 1..4) fp64 values carried along, the way open3d carries colours
    (shine_voxel_down_attr): their per-voxel means, summed in input order, are returned last ([m] or [m,a]); points and keys are
    the same bits as without attrs."""
    torch = _torch()
    voxel = float(voxel)
    if not voxel > 0.0:
        raise ValueError("voxel_down_sample: voxel must be > 0")
    host = _host_points(points)
    n = len(host) if host is not None else int(points.shape[0])
    att, flat = None, False
    if attrs is not None:
        att = attrs.detach() if isinstance(attrs, torch.Tensor) else torch.as_tensor(np.asarray(attrs, dtype=np.float64))
        flat = att.dim() == 1
        att = att.reshape(n, -1) if n else att.reshape(0, 1 if flat else att.shape[-1])
        if att.shape[1] < 1 or att.shape[1] > 4:
            raise ValueError("voxel_down_sample: attrs must be [n] or [n,a] with 1 <= a <= 4, got %s" % (tuple(attrs.shape),))

    def result(out, keys, aout):
        res = (out,) + ((keys,) if return_keys else ()) + ((aout[:, 0] if flat else aout,) if att is not None else ())
        return res[0] if len(res) == 1 else res

    if n == 0:
        pts = _points(points)
        return result(torch.empty((0, 3), dtype=torch.float64, device=pts.device), torch.empty(0, dtype=torch.int64, device=pts.device),
                      torch.empty((0, att.shape[1]), dtype=torch.float64, device=pts.device) if att is not None else None)
    lo, hi = bounds(points)
    origin = lo - voxel * 0.5
    _check_axis_bits(lo, hi, origin, voxel, "voxel_down_sample")
    pts = _points(points)
    lib, st = _lib.lib(), _stream()
    out = torch.empty((n, 3), dtype=torch.float64, device=pts.device)
    keys = torch.empty(n, dtype=torch.int64, device=pts.device) if return_keys else None
    keys_ptr = keys.data_ptr() if keys is not None else None
    m = C.c_int64(0)
    if att is None:
        _lib.call_with_workspace(lib.shine_eval_voxel_down, pts.device, pts.data_ptr(), n, _d3(origin), voxel, _lib.WS,
                                 _lib.WS_BYTES, out.data_ptr(), keys_ptr, C.byref(m), st)
        aout = None
    else:
        att = att.to(device=pts.device, dtype=torch.float64).contiguous()
        a = int(att.shape[1])
        aout = torch.empty((n, a), dtype=torch.float64, device=pts.device)
        _lib.call_with_workspace(lib.shine_voxel_down_attr, pts.device, pts.data_ptr(), att.data_ptr(), a, n, _d3(origin), voxel,
                                 _lib.WS, _lib.WS_BYTES, out.data_ptr(), aout.data_ptr(), keys_ptr, C.byref(m), st)
        aout = aout[:m.value].clone()
    return result(out[:m.value].clone(), keys[:m.value].clone() if keys is not None else None, aout)


class NNGrid:
    """The search grid over a reference set (csrc/shine_eval.hip): build once, query many times."""

    def __init__(self, ref, cell=None, spacing=None):
        torch = _torch()
        self.ref = _points(ref)
        n = self.ref.shape[0]
        if n == 0:
            raise ValueError("NNGrid: empty reference set")
        if int(_lib.lib().shine_eval_fine_per_coarse()) != FINE_PER_COARSE:
            raise _lib.ShineHipError("libshine_hip.so was built with another FINE_PER_COARSE than evaluation.py states")
        self.n = n
        self.lo, self.hi = bounds(self.ref)
        if not (np.all(np.isfinite(self.lo)) and np.all(np.isfinite(self.hi))):
            raise ValueError("NNGrid: the reference set holds non-finite coordinates")
        extent = float((self.hi - self.lo).max())
        floor_cell = max(extent / (2 ** AXIS_BITS - 2), 1e-300)  # 21-bit indices; a single point gets any positive cell
        if cell is None:
            if spacing is None:
                spacing = self._estimate_spacing(extent, floor_cell)
            cell = CELL_FACTOR * float(spacing)
        self.cell = max(float(cell), floor_cell) if extent > 0 else max(float(cell), 1e-6)
        self._build()

    def _count(self, cell):
        counts = (C.c_int64 * 2)()
        ws, need = _lib.call_with_workspace(_lib.lib().shine_eval_grid_count, self.ref.device, self.ref.data_ptr(), self.n,
                                            _d3(self.lo), cell, _lib.WS, _lib.WS_BYTES, counts, _stream())
        return ws, need.value, int(counts[0]), int(counts[1])

    def _estimate_spacing(self, extent, floor_cell):
        """mean spacing of a surface-like set from one trial grid: with p points per occupied cell of edge h, s = h / sqrt(p)"""
        if extent <= 0 or self.n < 2:
            return 1.0
        h0 = max(8.0 * extent / math.sqrt(self.n), floor_cell)
        _, _, n_fine, _ = self._count(h0)
        return h0 / math.sqrt(self.n / max(n_fine, 1))

    def _build(self):
        self.cells_per_axis = _check_axis_bits(self.lo, self.hi, self.lo, self.cell, "nn_correspondence")
        ws, ws_bytes, self.n_fine, self.n_coarse = self._count(self.cell)
        # (the grid is a result, sized and refused like a workspace: the placeholders stand for `grid` and `grid_bytes`)
        self.grid, _ = _lib.call_with_workspace(_lib.lib().shine_eval_grid_emit, self.ref.device, self.ref.data_ptr(), self.n,
                                                ws.data_ptr(), ws_bytes, self.n_fine, self.n_coarse, _lib.WS, _lib.WS_BYTES,
                                                _stream())

    @property
    def coarse_cell(self):
        return self.cell * FINE_PER_COARSE

    def max_coarse_cells(self, truncation):
        """the most coarse cells one query can probe: (2 ceil(truncation / C) + 1)^3, and never more than the grid has"""
        k = 2 * math.ceil(float(truncation) / self.coarse_cell) + 1
        per_axis = [min(k, int((c - 1) // FINE_PER_COARSE) + 1) for c in self.cells_per_axis]
        return per_axis[0] * per_axis[1] * per_axis[2]

    def max_fine_cells(self, truncation):
        """the most fine cells one query can test: only those of occupied coarse cells it probed"""
        return min(self.n_fine, FINE_PER_COARSE ** 3 * min(self.n_coarse, self.max_coarse_cells(truncation)))

    def query(self, query, truncation, stats=False):
        """(index int32 [n_q] (-1: nothing inside the truncation), dist fp64 [n_q] (clamped to the truncation), keep bool [n_q])
        on the device, in the caller's order; with stats also (max coarse cells probed, max fine cells tested) of any query."""
        torch = _torch()
        q = _points(query, self.ref.device)
        nq = q.shape[0]
        truncation = float(truncation)
        if not truncation >= 0.0:
            raise ValueError("nn_correspondence: truncation must be >= 0")
        idx = torch.empty(nq, dtype=torch.int32, device=q.device)
        dist = torch.empty(nq, dtype=torch.float64, device=q.device)
        keep = torch.empty(nq, dtype=torch.uint8, device=q.device)
        st_dev = torch.zeros(2, dtype=torch.int32, device=q.device) if stats else None
        if nq:
            _lib.call_with_workspace(
                _lib.lib().shine_eval_nn_search, q.device, self.grid.data_ptr(), self.n, self.n_fine, self.n_coarse, _d3(self.lo),
                self.cell, (C.c_int64 * 3)(*[int(c) for c in self.cells_per_axis]), q.data_ptr(), nq, truncation, _lib.WS,
                _lib.WS_BYTES, idx.data_ptr(), dist.data_ptr(), keep.data_ptr(), st_dev.data_ptr() if stats else None, _stream())
        keep = keep.bool()
        if stats:
            mc, mf = (int(v) for v in st_dev.cpu())
            return idx, dist, keep, mc, mf
        return idx, dist, keep


def nn_correspondence(ref_points, query_points, truncation, ignore_outlier=True, cell=None, spacing=None, stats=False, grid=None):
    """eval_utils.nn_correspondance: for each query point the nearest reference point.  keep = d^2 < truncation^2 (strict); a
    dropped query is removed from the compacted result when `ignore_outlier`, else kept with dist = truncation.  Either set
    empty gives an empty result.  Returns NNResult: index / dist / keep per query on the device (index -1 where keep is
    False), indices / distances = the compacted form the reference returns (device tensors), and with stats=True the largest
    number of coarse / fine cells one query visited.  `cell` is the fine cell edge (default CELL_FACTOR x the reference set's
    mean spacing: `spacing` if given, else estimated); `grid` re-uses an NNGrid built over `ref_points`."""
    torch = _torch()
    q = _points(query_points, grid.ref.device if grid is not None else None)
    if grid is None:
        r = _points(ref_points, q.device)
        if r.shape[0] == 0 or q.shape[0] == 0:
            e_i = torch.empty(0, dtype=torch.int32, device=q.device)
            e_d = torch.empty(0, dtype=torch.float64, device=q.device)
            return NNResult(e_i, e_d, torch.empty(0, dtype=torch.bool, device=q.device), e_i, e_d, 0, 0, None)
        grid = NNGrid(r, cell=cell, spacing=spacing)
    res = grid.query(q, truncation, stats=stats)
    idx, dist, keep = res[:3]
    mc, mf = (res[3], res[4]) if stats else (None, None)
    if ignore_outlier:
        return NNResult(idx, dist, keep, idx[keep], dist[keep], mc, mf, grid.cell)
    return NNResult(idx, dist, keep, idx, dist, mc, mf, grid.cell)


def distance_sums(dist_p, dist_r, threshold):
    """ONE launch over the two distance arrays: numpy [8] = sum, sum of squares, count(< threshold) of dist_p, the same of dist_r,
    len(dist_p), len(dist_r)."""
    torch = _torch()
    dp = dist_p.detach().double().contiguous()
    dr = dist_r.detach().to(dp.device).double().contiguous()
    out = torch.empty(8, dtype=torch.float64, device=dp.device)
    _lib.call_with_workspace(_lib.lib().shine_eval_metrics, dp.device, dp.data_ptr() if dp.numel() else None, dp.numel(),
                             dr.data_ptr() if dr.numel() else None, dr.numel(), float(threshold), _lib.WS, _lib.WS_BYTES,
                             out.data_ptr(), _stream())
    return out.cpu().numpy()


def metrics_from_sums(sums, down_sample_res, threshold, truncation_acc, truncation_com):
    """the reference's dict (same eleven keys, same order) from distance_sums' eight numbers; an empty array gives NaN where
    numpy's mean of an empty array does, and the F-score is NaN when precision + recall is 0"""
    sp, sp2, cp, sr, sr2, cr, n_p, n_r = (float(v) for v in sums)
    nan = float("nan")
    mean_p, mean_p2, precision = (sp / n_p, sp2 / n_p, cp / n_p * 100.0) if n_p else (nan, nan, nan)
    mean_r, mean_r2, recall = (sr / n_r, sr2 / n_r, cr / n_r * 100.0) if n_r else (nan, nan, nan)
    denom = precision + recall
    fscore = 2 * precision * recall / denom if denom != 0 else nan
    vals = [mean_p, mean_r, 0.5 * (mean_p + mean_r), math.sqrt(0.5 * (mean_p2 + mean_r2)) if n_p and n_r else nan, precision, recall,
            fscore, down_sample_res, threshold, truncation_acc, truncation_com]
    return dict(zip(METRIC_KEYS, vals))


# ------------------------------------------------------------------------------------------------ PLY input
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path):
    """PLY reader in plain numpy: ascii and binary_little_endian; returns a dict with "vertices" [n,3] fp64, "faces" [f,3] int32
    or None (a vertex-only file is a cloud), and every other vertex property under its own name (1-D arrays)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok or tok[0] in ("ply", "comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("%s: property before any element" % path)
            if tok[1] == "list":
                elements[-1][2].append((tok[4], ("list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("%s: unsupported PLY format %r (ascii and binary_little_endian are read)" % (path, fmt))
    out = {"vertices": np.zeros((0, 3)), "faces": None}
    tokens = data[body:].split() if fmt == "ascii" else None
    pos = 0 if fmt == "ascii" else body
    for name, count, props in elements:
        has_list = any(isinstance(t, tuple) for _, t in props)
        if not has_list:
            if fmt == "ascii":
                flat = np.array(tokens[pos:pos + count * len(props)], dtype=np.float64).reshape(count, len(props))
                pos += count * len(props)
                cols = {p: flat[:, k].astype(t) for k, (p, t) in enumerate(props)}
            else:
                dt = np.dtype([(p, "<" + t) for p, t in props])
                rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                cols = {p: rec[p] for p, _ in props}
            if name == "vertex":
                out["vertices"] = np.stack([cols[a].astype(np.float64) for a in ("x", "y", "z")], 1).reshape(-1, 3)
                for p, _ in props:
                    if p not in ("x", "y", "z"):
                        out[p] = np.array(cols[p])
            continue
        if len(props) != 1:
            raise ValueError("%s: element %s mixes a list with other properties (not read)" % (path, name))
        _, (_, ct, it) = props[0]
        if fmt == "ascii":
            rows = []
            for _ in range(count):
                k = int(tokens[pos])
                rows.append([int(t) for t in tokens[pos + 1:pos + 1 + k]])
                pos += 1 + k
        else:
            dt = np.dtype([("n", "<" + ct), ("i", "<" + it, 3)])
            rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
            if count and not np.all(rec["n"] == 3):
                raise ValueError("%s: only triangle faces are read" % path)
            pos += count * dt.itemsize
            rows = rec["i"]
        if name == "face":
            if fmt == "ascii" and any(len(r) != 3 for r in rows):
                raise ValueError("%s: only triangle faces are read" % path)
            out["faces"] = np.asarray(rows, dtype=np.int64).astype(np.int32).reshape(-1, 3)
    return out


def _load_mesh(pred):
    """(verts, faces) from a PLY path, a mesher.TriangleMesh / open3d mesh (anything with .vertices and .triangles) or a pair"""
    if isinstance(pred, str) or hasattr(pred, "__fspath__"):
        d = read_ply(pred)
        if d["faces"] is None:
            raise ValueError("%s holds no faces: the prediction must be a mesh" % pred)
        return d["vertices"], d["faces"]
    if hasattr(pred, "vertices") and hasattr(pred, "triangles"):
        return np.asarray(pred.vertices, dtype=np.float64), np.asarray(pred.triangles, dtype=np.int32)
    if isinstance(pred, (tuple, list)) and len(pred) == 2:
        return pred
    raise TypeError("eval_mesh: pred must be a PLY path, a TriangleMesh or a (verts, faces) pair")


def _load_cloud(trgt):
    if isinstance(trgt, str) or hasattr(trgt, "__fspath__"):
        return read_ply(trgt)["vertices"]
    if hasattr(trgt, "points"):
        return np.asarray(trgt.points, dtype=np.float64)
    return trgt


def eval_mesh(file_pred, file_trgt, down_sample_res=0.02, threshold=0.05, truncation_acc=0.50, truncation_com=0.50,
              gt_bbx_mask_on=True, mesh_sample_point=10000000, possion_sample_init_factor=5, seed=0, return_points=False):
    """eval_utils.eval_mesh: mesh metrics between a predicted mesh and a target cloud; same parameters, defaults and return dict
    (possion_sample_init_factor is accepted and ignored, as there).  `file_pred`: a PLY path, a mesher.TriangleMesh, an open3d
    mesh or a (verts, faces) pair of arrays / tensors (device tensors are used in place); `file_trgt`: a PLY path or an [n,3]
    array / tensor.  With down_sample_res <= 0 neither cloud is down-sampled (the reference fails there).  `seed` keys the
    sampler (not open3d's random stream).  return_points additionally returns the two clouds the distances were taken
    between (device tensors)."""
    verts, faces = _load_mesh(file_pred)
    trgt = _points(_load_cloud(file_trgt))
    v = _points(verts, trgt.device)
    f = _faces(faces, trgt.device)
    if gt_bbx_mask_on and trgt.shape[0]:
        lo, hi = bounds(trgt)
        lo[2] -= down_sample_res
        hi[2] += down_sample_res
        v, f = crop_mesh(v, f, lo, hi)
    if f.shape[0]:
        pred = sample_points_uniformly(v, f, int(mesh_sample_point), seed=seed)
    else:  # nothing of the mesh is left: every metric of the prediction side is NaN, as numpy's mean of nothing
        pred = v.new_zeros((0, 3))
    if down_sample_res > 0:
        before = pred.shape[0]
        pred = voxel_down_sample(pred, down_sample_res)
        trgt = voxel_down_sample(trgt, down_sample_res)
        print("Predicted mesh unifrom sample: ", before, " --> ", pred.shape[0], " (", down_sample_res, "m)")
    spacing = down_sample_res if down_sample_res > 0 else None
    dist_p = nn_correspondence(trgt, pred, truncation_acc, True, spacing=spacing).distances
    dist_r = nn_correspondence(pred, trgt, truncation_com, False, spacing=spacing).distances
    sums = distance_sums(dist_p, dist_r, threshold)
    metrics = metrics_from_sums(sums, down_sample_res, threshold, truncation_acc, truncation_com)
    return (metrics, pred, trgt) if return_points else metrics


def crop_intersection(file_gt, files_pred, out_file_crop, dist_thre=0.1, mesh_sample_point=1000000, seed=0):
    """eval_utils.crop_intersection: keep the ground-truth points that have a sample of EVERY predicted mesh within dist_thre
    (squared distance < dist_thre^2), in their order, and write them as a binary PLY cloud."""
    from .mesher import write_ply

    print("Load the original ground truth point cloud from:", file_gt)
    gt = _points(_load_cloud(file_gt))
    for cur in files_pred:
        print("Process", cur)
        verts, faces = _load_mesh(cur)
        sample = sample_points_uniformly(_points(verts, gt.device), faces, int(mesh_sample_point), seed=seed)
        if gt.shape[0]:
            gt = gt[nn_correspondence(sample, gt, dist_thre, True).keep]
    print("Output the croped ground truth to:", out_file_crop)
    g = gt.cpu().numpy()
    write_ply(out_file_crop, [("x", g[:, 0], "double"), ("y", g[:, 1], "double"), ("z", g[:, 2], "double")])
    return gt


def write_csv(path, metrics):
    """the one-row CSV of eval/evaluator.py (same column order)"""
    with open(path, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=METRIC_KEYS)
        w.writeheader()
        w.writerow(metrics)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m shine_mapping_amd.evaluation",
                                 description="Mesh metrics of a predicted mesh against a ground-truth cloud, on the device.")
    ap.add_argument("pred", help="predicted mesh (PLY)")
    ap.add_argument("gt", help="ground-truth point cloud (PLY)")
    ap.add_argument("--spacing", type=float, default=0.02, help="voxel size of the down-sampling (<= 0: none)")
    ap.add_argument("--threshold", type=float, default=0.05, help="inlier distance of precision / recall")
    ap.add_argument("--trunc-acc", type=float, default=0.50, help="truncation of the accuracy distances (outliers dropped)")
    ap.add_argument("--trunc-com", type=float, default=0.50, help="truncation of the completeness distances (outliers clamped)")
    ap.add_argument("--no-bbx-mask", action="store_true", help="do not crop the mesh to the ground truth's bounding box")
    ap.add_argument("--samples", type=int, default=10000000, help="points sampled from the mesh")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--csv", default=None, help="also write the one-row CSV here")
    a = ap.parse_args(argv)
    m = eval_mesh(a.pred, a.gt, down_sample_res=a.spacing, threshold=a.threshold, truncation_acc=a.trunc_acc,
                  truncation_com=a.trunc_com, gt_bbx_mask_on=not a.no_bbx_mask, mesh_sample_point=a.samples, seed=a.seed)
    print(m)
    if a.csv:
        write_csv(a.csv, m)
    return 0


if __name__ == "__main__":
    sys.exit(main())
