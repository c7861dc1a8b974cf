"""Hand-built meshes for the mesh post-processing (csrc/shine_mesh.hip: vertex normals, cluster filter), everything from a seed in
numpy: the inputs a closed manifold marching-cubes mesh in grid order never gives.  tests/test_mesh.py checks the host oracles
on them (the two cluster oracles agree; the plain fp64 normals stay inside the bound), tests/test_gpu_mesh_post.py the kernels.
References are computed once per process and handed out read-only."""
import functools

import numpy as np

import mc_oracle as mo

I32 = np.int32


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------------------------------------------------------ cluster inputs
def strip(n, first_vertex=0):
    """n triangles (i, i+1, i+2), consistently wound: neighbours share the edge (i+1, i+2); one cluster"""
    i = np.arange(n, dtype=np.int64) + first_vertex
    odd = (np.arange(n) & 1).astype(bool)
    return np.stack([np.where(odd, i + 1, i), np.where(odd, i, i + 1), i + 2], 1)


def zigzag(n):
    """0, n-1, 1, n-2, ..."""
    p = np.empty(n, np.int64)
    p[0::2] = np.arange((n + 1) // 2)
    p[1::2] = n - 1 - np.arange(n // 2)
    return p


STRIP_LEN = 100_000
MANY_STRIPS = (300, 299, 1, 2, 3, 17, 63, 64, 65, 128, 257, 301, 500, 777, 1000, 1024, 1500, 2000, 3000, 4097)
SINGLETONS = 70_001
BOOKS = (3, 4, 65)
LAUNCH_F = (1, 2, 85, 86, 255, 256, 257, 65_536 + 1)
SHEET_N = 160  # vertices per side of the open sheet: 2 * 159^2 = 50 562 triangles before the holes


def many_strips():
    """strips of MANY_STRIPS lengths on disjoint vertices, interleaved triangle by triangle (round robin while a strip has
    triangles left): strip k's first triangle is triangle k, so cluster k is strip k"""
    parts, owner, base = [], [], 0
    for k, n in enumerate(MANY_STRIPS):
        parts.append(strip(n, base))
        owner.append(np.stack([np.arange(n), np.full(n, k)], 1))  # (position in the strip, strip)
        base += n + 2
    f, o = np.concatenate(parts), np.concatenate(owner)
    order = np.lexsort((o[:, 1], o[:, 0]))
    return f[order], o[order, 1]


def grid_faces(nx, ny):
    """two triangles per cell of an nx x ny vertex grid (vertex id = x * ny + y), wound towards +z"""
    x, y = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (x * ny + y).reshape(-1)
    b, c, d = a + ny, a + ny + 1, a + 1
    return np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)


def holed_sheet(frac, seed):
    """the open SHEET_N^2 sheet with `frac` of its triangles deleted at random and the rest shuffled"""
    f = grid_faces(SHEET_N, SHEET_N)
    rng = np.random.default_rng(seed)
    f = f[rng.random(len(f)) >= frac]
    return f[rng.permutation(len(f))]


def book(k):
    """k triangles around the edge (0, 1), alternately wound, and an unrelated triangle that touches vertex 0 only"""
    pages = [(0, 1, 2 + i) if i % 2 == 0 else (1, 0, 2 + i) for i in range(k)]
    return np.array(pages[:k // 2] + [(0, k + 10, k + 11)] + pages[k // 2:], np.int64)


def two_clusters(F, small_last):
    """F triangles as two strips (F - 2 and 2 triangles; F - 1 and 1 below 4; one triangle for F = 1), the small one last or
    first: the last triangle is in the cluster that a threshold between the sizes keeps or drops"""
    if F == 1:
        return strip(1)
    m = 2 if F >= 4 else 1
    big, small = strip(F - m), strip(m, F + 10)
    return np.concatenate([big, small] if small_last else [small, big])


_SMALL = np.concatenate([np.array([(0, 1, 2), (2, 3, 4), (5, 6, 7), (6, 5, 8), (9, 10, 11), (9, 10, 12)], np.int64), strip(10, 13)])
TOP = 1 << 30  # ids p and p | TOP differ only in the top bit that an int32 id can have set


def top_bit_mesh():
    """the edge (p, q = p | 2^30) shared by two triangles; around them triangles whose keys agree with it in one half only (the
    same low id with another high id, the same high id with another low id) and must stay apart"""
    p, q = 5, 5 | TOP
    return np.array([(p, q, 100), (6, q, 102), (q, p, 101), (p, 200, 201), (q, 300 | TOP, 301 | TOP), (p | 1 << 29, q, 103),
                     (p, 5 | 1 << 29, 104), ((1 << 31) - 1, (1 << 31) - 2, p), ((1 << 31) - 2, (1 << 31) - 1, 6)], np.int64)


@functools.lru_cache(maxsize=None)
def cluster_cases():
    """{name: faces [F,3] int32}"""
    rng = np.random.default_rng(11)
    s = strip(STRIP_LEN)
    c = {"strip-identity": s, "strip-reversed": s[::-1], "strip-random": s[rng.permutation(STRIP_LEN)],
         "strip-zigzag": s[zigzag(STRIP_LEN)],
         "many-strips": many_strips()[0],
         "singletons": np.arange(3 * SINGLETONS, dtype=np.int64).reshape(-1, 3),
         "bow-tie": np.array([(0, 1, 2), (2, 3, 4)]),
         "edge-opposite": np.array([(0, 1, 2), (1, 0, 3)]), "edge-same": np.array([(0, 1, 2), (0, 1, 3)])}
    for k in BOOKS:
        c["book-%d" % k] = book(k)
    c["duplicates"] = np.array([(0, 1, 2), (5, 6, 7), (0, 1, 2), (2, 1, 0)])
    c["degenerate"] = np.array([(0, 0, 1), (2, 2, 2), (3, 4, 5), (2, 2, 2), (6, 6, 0)])
    c["degenerate-attached"] = np.array([(7, 7, 7), (0, 1, 1), (0, 1, 2)])
    c["lone-point"] = np.array([(5, 5, 5)])
    c["sheet-10"] = holed_sheet(0.10, 21)
    c["sheet-60"] = holed_sheet(0.60, 22)
    for F in LAUNCH_F:
        c["launch-%d-small-last" % F] = two_clusters(F, True)
        if F > 1:
            c["launch-%d-big-last" % F] = two_clusters(F, False)
    for name, shift in (("ids-2^16", (1 << 16) - 6), ("ids-2^24", (1 << 24) - 6), ("ids-2^31", (1 << 31) - 1 - int(_SMALL.max()))):
        c[name] = _SMALL + shift
    c["ids-top-bit"] = top_bit_mesh()
    out = {}
    for name, f in c.items():
        assert f.min() >= 0 and f.max() < 1 << 31, name
        out[name] = _ro(np.ascontiguousarray(f, I32))
    return out


CLUSTER_NAMES = tuple(["strip-identity", "strip-reversed", "strip-random", "strip-zigzag", "many-strips", "singletons", "bow-tie",
                       "edge-opposite", "edge-same"] + ["book-%d" % k for k in BOOKS]
                      + ["duplicates", "degenerate", "degenerate-attached", "lone-point", "sheet-10", "sheet-60"]
                      + [n for F in LAUNCH_F for n in (["launch-%d-small-last" % F] + (["launch-%d-big-last" % F] if F > 1 else []))]
                      + ["ids-2^16", "ids-2^24", "ids-2^31", "ids-top-bit"])


def clusters_oracle(faces):
    """(cluster ids, counts) by the graph oracle; by the union-find where scipy does not import (and says so)"""
    if mo.have_scipy():
        return mo.triangle_clusters_graph(faces)
    print("scipy does not import: clusters by mc_oracle.triangle_clusters (the union-find) instead of the graph oracle")
    return mo.triangle_clusters(faces)


@functools.lru_cache(maxsize=None)
def cluster_reference(name):
    return _ro(*clusters_oracle(cluster_cases()[name]))


def thresholds(counts, F):
    """min_tri in {0, 1, every distinct cluster size s, s + 1, F + 1}"""
    s = np.unique(counts)
    return sorted(set([0, 1, F + 1]) | set(int(v) for v in s) | set(int(v) + 1 for v in s))


# ------------------------------------------------------------------------------------------------------------------ normals inputs
def height_field(nx, ny, cell=(0.1, 0.1), shift=(0.0, 0.0, 0.0), seed=5):
    """a bumpy open sheet: waves of a few cells' length plus seeded roughness, two triangles per cell"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    z = 0.04 * np.sin(0.37 * x) * np.cos(0.23 * y) + 0.02 * np.sin(0.05 * x * y / max(nx, ny)) + 0.01 * rng.standard_normal(x.shape)
    v = np.stack([x * cell[0], y * cell[1], z], -1).reshape(-1, 3) + np.asarray(shift, np.float64)
    return v, grid_faces(nx, ny)


FAN = 20_000
WORLD_SHIFT = (3000.0, -1500.0, 40.0)
KEY_WIDTH_V = (1, 2, 3, 255, 256, 257, 65_536, 65_537)


def cone_fan():
    """FAN faces around the apex (vertex 0): one vertex sums a run of FAN face normals"""
    t = 2 * np.pi * np.arange(FAN) / FAN
    rim = np.stack([np.cos(t), np.sin(t), np.zeros(FAN)], 1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], rim]) + np.array([12.5, -7.25, 3.0])
    i = np.arange(FAN)
    return v, np.stack([np.zeros(FAN, np.int64), 1 + i, 1 + (i + 1) % FAN], 1)


def star():
    """an open fan of 7 faces around vertex 0, a pendant vertex (valence 1) on one more face, and two vertices without faces: one
    in the middle of the id range, one at V - 1"""
    rng = np.random.default_rng(8)
    v = rng.standard_normal((14, 3))
    t = 2 * np.pi * np.arange(8) / 9
    v[0] = (0, 0, 0.5)
    ring = [1, 2, 3, 4, 5, 7, 8, 9]  # (vertex 6 stays unused)
    v[ring] = np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(3 * t)], 1)
    f = [(0, ring[k], ring[k + 1]) for k in range(7)] + [(9, 10, 11), (10, 12, 11)]
    # vertex 12: valence 1; vertices 6 and 13: valence 0
    return v + np.array([2.0, 3.0, -1.0]), np.array(f, np.int64), (6, 13)


def cancelling():
    """integer coordinates, every operation exact in fp64: two coincident triangles of opposite winding (vertices 0, 1, 2), and a
    fold whose two faces' normals are (0, 0, 1) and (0, 0, -1) at the vertices they share (3 and 5)"""
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 3, 0), (10, 10, 10), (11, 10, 10), (10, 11, 10), (9, 10, 10)], np.float64)
    f = np.array([(0, 1, 2), (0, 2, 1), (3, 4, 5), (3, 6, 5)], np.int64)
    return v, f, (0, 1, 2, 3, 5)


def key_width(V):
    """V vertices along a bumpy zig-zag band, every one used, faces (i, i+1, i+2) in shuffled order (in strip order the keys are
    nearly sorted before the sort, and a stable sort that leaves the top bit out still keeps every run together): vertex 0 and
    vertex V - 1 both have faces.  Below 3 vertices only degenerate faces fit: every normal is zero."""
    rng = np.random.default_rng(100 + V)
    i = np.arange(V, dtype=np.float64)
    v = np.stack([0.05 * i, 0.1 * (np.arange(V) & 1) + 0.01 * rng.standard_normal(V), 0.02 * np.sin(0.3 * i) + 7.0], 1)
    if V == 1:
        return v, np.array([(0, 0, 0)], np.int64), (0,)
    if V == 2:
        return v, np.array([(0, 0, 1), (1, 1, 0)], np.int64), (0, 1)
    f = strip(V - 2)
    if V >= 6:  # two more faces on vertex 0 and on vertex V - 1, wound like the strip: their runs hold three faces each
        extra = np.array([(0, 2, 3), (0, 3, 4), (V - 1, V - 3, V - 4), (V - 1, V - 4, V - 5)], np.int64)
        e1, e2 = v[extra[:, 1]] - v[extra[:, 0]], v[extra[:, 2]] - v[extra[:, 0]]
        s0 = v[f[0, 1]] - v[f[0, 0]], v[f[0, 2]] - v[f[0, 0]]
        flip = np.sign(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) != np.sign(s0[0][0] * s0[1][1] - s0[0][1] * s0[1][0])
        extra[flip] = extra[flip][:, [0, 2, 1]]
        f = np.concatenate([f, extra])
    return v, f[rng.permutation(len(f))], ()


def with_degenerates():
    """(a, a, b) and (a, a, a) faces mixed into a proper sheet: they add zero to their vertices"""
    v, f = height_field(20, 23, seed=9)
    rng = np.random.default_rng(10)
    a, b = rng.integers(0, len(v), 60), rng.integers(0, len(v), 60)
    deg = np.concatenate([np.stack([a[:20], a[:20], b[:20]], 1), np.stack([a[20:40], b[20:40], b[20:40]], 1),
                          np.stack([a[40:], a[40:], a[40:]], 1)])
    at = np.sort(rng.integers(0, len(f), len(deg)))
    return v, np.insert(f, at, deg, axis=0)


@functools.lru_cache(maxsize=None)
def normals_cases():
    """{name: (verts [V,3] f64, faces [F,3] int32, indices of the vertices whose face normals cancel or that have no proper
    face)}"""
    rng = np.random.default_rng(12)
    c = {}
    c["field-origin"] = height_field(200, 200) + ((),)
    v, f = height_field(200, 200, shift=WORLD_SHIFT)
    c["field-world"] = (v, f, ())
    c["field-world-shuffled"] = (v, f[rng.permutation(len(f))], ())
    c["fan"] = cone_fan() + ((),)
    c["star"] = star()
    c["skinny"] = height_field(60, 60, cell=(0.1, 1000.0), seed=6) + ((),)
    c["cancelling"] = cancelling()
    for V in KEY_WIDTH_V:
        c["key-width-%d" % V] = key_width(V)
    c["no-faces"] = (rng.standard_normal((5, 3)), np.zeros((0, 3), np.int64), (0, 1, 2, 3, 4))
    c["degenerate-faces"] = with_degenerates() + ((),)
    out = {}
    for name, (v, f, cancel) in c.items():
        assert len(f) == 0 or (f.min() >= 0 and f.max() < len(v)), name
        out[name] = _ro(np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, I32)) + (tuple(cancel),)
    return out


NORMALS_NAMES = tuple(["field-origin", "field-world", "field-world-shuffled", "fan", "star", "skinny", "cancelling"]
                      + ["key-width-%d" % V for V in KEY_WIDTH_V] + ["no-faces", "degenerate-faces"])

COND_LIMIT = 1e6


@functools.lru_cache(maxsize=None)
def normals_reference(name):
    v, f, _ = normals_cases()[name]
    return _ro(*mo.vertex_normals_ext(v, f))


def check_normals(n, ref, kv, cond, cancel=()):
    """Assert |n - n_ref|_inf <= 8 (k_v + 8) 2^-53 cond_v at every vertex with cond_v <= 1e6, that only vertices listed in `cancel`
    are beyond that limit, and that a vertex whose reference sum is exactly zero is exactly (0, 0, 0).  The bound counts
    roundings: one per edge difference, about three per cross-product component (contracted or not) relative to |e1| |e2|, k - 1
    for a sum of k terms in any fixed order, a few for the normalisation, and 8 for the constants.  Returns the largest
    error / bound ratio (0 where nothing is compared)."""
    n = np.asarray(n, np.float64)
    assert n.shape == ref.shape
    beyond = np.flatnonzero(cond > COND_LIMIT)
    assert set(beyond.tolist()) <= set(cancel), "ill-conditioned vertices that were not built to cancel: %s" % beyond[:10]
    zero = (ref == 0).all(1)
    assert (n[zero] == 0).all(), "a zero sum must stay exactly zero"
    cmp = cond <= COND_LIMIT
    if not cmp.any():
        return 0.0
    err = np.abs(n.astype(np.longdouble) - ref).max(1)[cmp].astype(np.float64)
    bound = 8.0 * (kv[cmp] + 8) * 2.0 ** -53 * cond[cmp]
    ratio = float((err / bound).max())
    worst = int(np.argmax(err / bound))
    assert (err <= bound).all(), "error %.3e over the bound %.3e (ratio %.3g)" % (err[worst], bound[worst], ratio)
    return ratio
