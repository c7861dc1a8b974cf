"""Numpy marching cubes with the rules of DESIGN.md "Meshing", on the table parsed from csrc/shine_mc_tables.hpp: the oracle the
device kernel (csrc/shine_mc.hip) is compared with, bit for bit on faces and to 1e-6 index units on vertices.  Also the small
host oracles of the mesh post-processing (area-weighted normals in fp64 and in 80-bit long double, edge-connected clusters by
union-find and by sort + connected components, remove_vertices_by_mask) and a PLY reader."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "shine_mapping_amd", "csrc", "shine_mc_tables.hpp")


def parse_tables(path=HEADER):
    text = open(path).read()
    base = [int(v) for v in re.search(r"MC_EDGE_BASE\[12\]\s*=\s*\{([^}]*)\}", text).group(1).split(",")]
    ntri = [int(v) for v in re.search(r"MC_NTRI\[256\]\s*=\s*\{([^}]*)\}", text).group(1).replace("\n", " ").split(",")
            if v.strip()]
    body = re.search(r"MC_TRI\[256\]\[SHINE_MC_TRI_WIDTH\]\s*=\s*\{(.*)\};", text, re.S).group(1)
    rows = re.findall(r"\{([^}]*)\}", body)
    tri = []
    for r in rows:
        vals = [int(v) for v in r.split(",")]
        k = vals.index(-1) if -1 in vals else len(vals)
        tri.append([tuple(vals[i:i + 3]) for i in range(0, k, 3)])
    assert len(base) == 12 and len(ntri) == 256 and len(tri) == 256
    assert all(len(t) == n for t, n in zip(tri, ntri))
    return base, tri


EDGE_BASE, TRI = parse_tables()


def edge_corners(e):
    a = e // 4
    c0 = EDGE_BASE[e]
    return c0, c0 | (1 << a)


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def marching_cubes(sdf, mask=None, level=0.0):
    """(verts [V,3] float32 index units, faces [F,3] int32)"""
    v = np.ascontiguousarray(sdf, dtype=np.float32)
    X, Y, Z = v.shape
    lev = np.float32(level)
    if min(X, Y, Z) < 2:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    inn = v > lev
    proc = np.ones((X - 1, Y - 1, Z - 1), bool) if mask is None else np.asarray(mask, bool)[:-1, :-1, :-1].copy()
    # processed cube flags padded so that the 4 cubes around an edge can be read with shifts (outside the grid: not processed)
    P = np.zeros((X + 1, Y + 1, Z + 1), bool)
    P[1:X, 1:Y, 1:Z] = proc  # P[x+1, y+1, z+1] = cube (x, y, z)

    def cube_any(a, x0, y0, z0, sx, sy, sz):
        # any processed cube among those containing the axis-a edge from point (x, y, z): origins differ by -1 / 0 on the other axes
        out = np.zeros((sx, sy, sz), bool)
        others = [k for k in range(3) if k != a]
        for d1 in (0, 1):
            for d2 in (0, 1):
                o = [1, 1, 1]
                o[others[0]] -= d1
                o[others[1]] -= d2
                out |= P[o[0]:o[0] + sx, o[1]:o[1] + sy, o[2]:o[2] + sz]
        return out

    # edges per axis: active = crossing and used by a processed cube
    act, collapse_hi, collapse_lo = [], [], []
    for a in range(3):
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[a] = slice(0, -1)
        sl1[a] = slice(1, None)
        v0, v1 = v[tuple(sl0)], v[tuple(sl1)]
        i0, i1 = inn[tuple(sl0)], inn[tuple(sl1)]
        cross = i0 != i1
        shp = v0.shape
        used = cube_any(a, 0, 0, 0, *shp)
        ac = cross & used
        act.append(ac)
        collapse_hi.append(ac & i0 & (v1 == lev))  # out end is the upper point and sits exactly on the level
        collapse_lo.append(ac & i1 & (v0 == lev))
    corner = np.zeros((X, Y, Z), bool)
    for a in range(3):
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[a] = slice(0, -1)
        sl1[a] = slice(1, None)
        corner[tuple(sl1)] |= collapse_hi[a]
        corner[tuple(sl0)] |= collapse_lo[a]
    own = np.zeros((X, Y, Z, 4), bool)
    own[..., 0] = corner
    for a in range(3):
        sl = [slice(None)] * 3
        sl[a] = slice(0, -1)
        own[tuple(sl) + (a + 1,)] = act[a] & ~collapse_hi[a] & ~collapse_lo[a]
    flat = own.reshape(-1)
    vid = np.cumsum(flat) - 1
    vid = vid.reshape(X, Y, Z, 4).astype(np.int64)
    nV = int(flat.sum())
    verts = np.zeros((nV, 3), np.float32)
    gx, gy, gz = np.meshgrid(np.arange(X, dtype=np.float32), np.arange(Y, dtype=np.float32), np.arange(Z, dtype=np.float32),
                             indexing="ij")
    pos = np.stack([gx, gy, gz], -1)
    sel = own[..., 0]
    verts[vid[..., 0][sel]] = pos[sel]
    for a in range(3):
        sel = own[..., a + 1]
        idx = np.nonzero(sel)
        up = list(idx)
        up[a] = up[a] + 1
        v0 = v[idx]
        v1 = v[tuple(up)]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((lev - v0) / (v1 - v0)).astype(np.float32)
        p = pos[idx].copy()
        p[:, a] = p[:, a] + t
        verts[vid[..., a + 1][idx]] = p
    # faces: processed cubes in linear order, then table order
    cidx = np.nonzero(proc)
    if len(cidx[0]) == 0:
        return verts, np.zeros((0, 3), np.int32)
    cx, cy, cz = cidx
    case = np.zeros(cx.shape, np.int64)
    for c in range(8):
        dx, dy, dz = corner_offset(c)
        case |= inn[cx + dx, cy + dy, cz + dz].astype(np.int64) << c
    ntri = np.array([len(t) for t in TRI])[case]
    lin = (cx.astype(np.int64) * Y + cy) * Z + cz
    out_f, out_key = [], []
    tri_arr = np.full((256, 5, 3), -1, np.int64)
    for c, t in enumerate(TRI):
        for k, tr in enumerate(t):
            tri_arr[c, k] = tr

    def edge_vid(e, sel):
        a = e // 4
        c0, c1 = edge_corners(e)
        o0, o1 = corner_offset(c0), corner_offset(c1)
        p0 = (cx[sel] + o0[0], cy[sel] + o0[1], cz[sel] + o0[2])
        p1 = (cx[sel] + o1[0], cy[sel] + o1[1], cz[sel] + o1[2])
        a0, a1 = v[p0], v[p1]
        i0 = a0 > lev
        res = vid[p0 + (np.full(p0[0].shape, a + 1),)].copy()
        hi = i0 & (a1 == lev)
        lo = (~i0) & (a0 == lev)
        res[hi] = vid[tuple(q[hi] for q in p1) + (np.zeros(int(hi.sum()), np.int64),)]
        res[lo] = vid[tuple(q[lo] for q in p0) + (np.zeros(int(lo.sum()), np.int64),)]
        return res

    for k in range(5):
        has = ntri > k
        if not has.any():
            continue
        sel = np.nonzero(has)[0]
        tr = tri_arr[case[sel], k]  # [n, 3] edges
        ids = np.zeros((len(sel), 3), np.int64)
        for j in range(3):
            for e in range(12):
                m = tr[:, j] == e
                if m.any():
                    ids[m, j] = edge_vid(e, sel[m])
        ok = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2])
        out_f.append(ids[ok])
        out_key.append(lin[sel[ok]] * 8 + k)
    if not out_f:
        return verts, np.zeros((0, 3), np.int32)
    faces = np.concatenate(out_f)
    key = np.concatenate(out_key)
    order = np.argsort(key, kind="stable")
    return verts, faces[order].astype(np.int32)


# ---- mesh post-processing oracles
def vertex_normals(verts, faces):
    """open3d's compute_vertex_normals: per vertex, the sum of its faces' (v1 - v0) x (v2 - v0) in face order, normalised (a
    zero sum stays zero)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    n = np.zeros_like(v)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    for j in range(3):
        np.add.at(n, f[:, j], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0.0)


def triangle_clusters(faces):
    """open3d's cluster_connected_triangles: triangles sharing an undirected edge are one cluster; cluster ids in the order of
    their smallest triangle.  Returns (cluster id per triangle, triangles per cluster)."""
    f = np.asarray(faces, np.int64)
    F = len(f)
    parent = np.arange(F)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    edges = {}
    for t in range(F):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            k = (min(f[t, a], f[t, b]), max(f[t, a], f[t, b]))
            if k in edges:
                ra, rb = find(edges[k]), find(t)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            else:
                edges[k] = t
    roots = np.array([find(t) for t in range(F)], np.int64)
    uniq, cid = np.unique(roots, return_inverse=True)  # (roots are the smallest triangle of each cluster: sorted = open3d order)
    return cid.astype(np.int64), np.bincount(cid, minlength=len(uniq))


def have_scipy():
    try:
        import scipy.sparse.csgraph  # noqa: F401

        return True
    except Exception:
        return False


def triangle_clusters_graph(faces):
    """The same rule as triangle_clusters without a union-find: the 3F undirected edge keys stable-sorted with their triangle
    ids, neighbours with equal keys linked in a sparse F x F graph, scipy's connected_components, and the components renumbered
    by their smallest triangle (open3d: clusters appear in the order of their first triangle).  Returns (cluster id per
    triangle, triangles per cluster)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    if F == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)  # edge j of triangle t: (f[t, j], f[t, j + 1])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    tri = np.repeat(np.arange(F, dtype=np.int64), 3)
    order = np.lexsort((hi, lo))  # (stable: by lo, then hi, then position)
    lo, hi, tri = lo[order], hi[order], tri[order]
    same = (lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1])
    g = coo_matrix((np.ones(int(same.sum()), np.int8), (tri[:-1][same], tri[1:][same])), shape=(F, F))
    ncomp, lab = connected_components(g, directed=False)
    first = np.full(ncomp, F, np.int64)
    np.minimum.at(first, lab, np.arange(F, dtype=np.int64))
    rank = np.empty(ncomp, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(ncomp, dtype=np.int64)
    cid = rank[lab]
    return cid, np.bincount(cid, minlength=ncomp)


def vertex_normals_ext(verts, faces):
    """vertex_normals' rule in np.longdouble (80-bit on x86: eps 1.08e-19), written out with products and differences: per
    vertex the sum of its faces' (v1 - v0) x (v2 - v0) in face order, normalised, a zero sum stays zero.  Returns (normals
    [V,3] longdouble, valence k_v [V] (a face counts once per corner it puts on the vertex), cond_v [V] float64 = sum over the
    vertex's faces of |e1| |e2| / |sum of the face normals|, inf where that sum is zero): the edge lengths, not |fn|, in the
    numerator, so that skinny triangles count with the rounding they cause."""
    L = np.longdouble
    v = np.asarray(verts, np.float64).reshape(-1, 3).astype(L)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1x, e1y, e1z = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1], p1[:, 2] - p0[:, 2]
    e2x, e2y, e2z = p2[:, 0] - p0[:, 0], p2[:, 1] - p0[:, 1], p2[:, 2] - p0[:, 2]
    fn = np.stack([e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x], 1)
    w = np.sqrt(e1x * e1x + e1y * e1y + e1z * e1z) * np.sqrt(e2x * e2x + e2y * e2y + e2z * e2z)
    corner = f.reshape(-1)  # face-major: ufunc.at adds in this order, so every vertex sums in face order
    n = np.zeros((V, 3), L)
    num = np.zeros(V, L)
    np.add.at(n, corner, np.repeat(fn, 3, axis=0))
    np.add.at(num, corner, np.repeat(w, 3))
    kv = np.bincount(corner, minlength=V).astype(np.int64)
    ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    nz = ln > 0
    cond = np.full(V, np.inf)
    cond[nz] = (num[nz] / ln[nz]).astype(np.float64)
    n[nz] = n[nz] / ln[nz][:, None]
    return n, kv, cond


def remove_vertices_by_mask(verts, faces, drop, *vertex_attrs):
    """open3d's remove_vertices_by_mask: drop the vertices, every triangle using one, reindex."""
    drop = np.asarray(drop, bool)
    keep = ~drop
    new_id = np.cumsum(keep) - 1
    f = np.asarray(faces, np.int64)
    fk = keep[f].all(1)
    return (np.asarray(verts)[keep], new_id[f[fk]].astype(np.int32)) + tuple(np.asarray(a)[keep] for a in vertex_attrs)


def read_ply(path):
    """Binary little-endian PLY reader for what shine_mapping_amd.mesher.write_ply writes: {element: {property: array}}."""
    types = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8"}
    with open(path, "rb") as fh:
        assert fh.readline().strip() == b"ply"
        assert fh.readline().strip() == b"format binary_little_endian 1.0"
        elems = []
        while True:
            line = fh.readline().strip().decode()
            if line == "end_header":
                break
            w = line.split()
            if w[0] == "element":
                elems.append((w[1], int(w[2]), []))
            elif w[0] == "property":
                elems[-1][2].append(tuple(w[1:]))
        out = {}
        for name, n, props in elems:
            if props and props[0][0] == "list":
                _, ct, it, pname = props[0]
                dt = np.dtype([("n", "<" + types[ct]), ("i", "<" + types[it], 3)])
                rec = np.frombuffer(fh.read(n * dt.itemsize), dt)
                assert (rec["n"] == 3).all()
                out[name] = {pname: rec["i"].copy()}
            else:
                dt = np.dtype([(p[1], "<" + types[p[0]]) for p in props])
                rec = np.frombuffer(fh.read(n * dt.itemsize), dt)
                out[name] = {p[1]: rec[p[1]].copy() for p in props}
        assert fh.read() == b""
    return out
