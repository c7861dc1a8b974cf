"""The workspace convention of include/shine_hip.h, entry point by entry point.

CPU: the size queries that are host arithmetic (no rocPRIM temporaries in them) answer exactly the bytes recorded in
tests/golden/workspace_sizes.json — recorded from the library as it was BEFORE the layouts moved onto one arena, not from the code
under test — and a NULL workspace_bytes is SHINE_E_INVALID.  Shapes: 1, one below / at / one above the entry point's tile, the
count at which a 256-byte slot of its arrays fills, and a few thousand.

GPU: every entry point with the size gate, rocPRIM ones included, at n <= 4096: a workspace of exactly the queried size filled
with 0xFF gives the same bits as one 4096 bytes larger filled with 0x00 (shine_plan_batch: see _plan_canonical); one byte
less is refused with "workspace too small" and leaves the host counters and the outputs alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, load_golden, product_from_golden

WS, WSB = "WS", "WS_BYTES"  # where the workspace pointer and its size_t* go in a recorded argument list
SIZES = os.path.join(GOLDEN_DIR, "workspace_sizes.json")
INVALID = -1


def host_cases():
    """(entry, args) of the queries that need no device: the list the golden file was recorded over"""
    out = []

    def add(entry, *args):
        out.append((entry, list(args)))

    for n in (1, 1023, 1024, 1025, 5000, 32767, 32768):  # 1024 draws (+ the closing spacing) per block sum, 32 sums per slot
        add("shine_sample_sorted", 1000, n, 1, 0, None, None, 0, None, None, WS, WSB, None)
        add("shine_sample_sorted_dev", 1000, n, 1, None, None, None, 0, None, None, WS, WSB, None)
        add("shine_sample_sorted_slice", 1000, n, 0, n, 1, 0, None, None, None, 0, None, None, WS, WSB, None)
    for n in (1, 127, 128, 129, 5000):  # chunks of bs * down_rate = 128 samples, sorted in LDS: the small form
        add("shine_importance_chunks", None, n, 64, 2, None, None, -(-n // 128), WS, WSB, None)
    for n in (1, 5000):
        add("shine_eval_bounds", None, n, WS, WSB, None, None)
    for nf in (1, 31, 32, 33, 1023, 1024, 1025, 5000):  # 8 bytes per triangle, one block total per 1024 triangles
        add("shine_eval_sample_mesh", None, 3, None, nf, 10, 0, None, WS, WSB, None, None, None)
    for n_p, n_r in ((1, 1), (5000, 3000)):
        add("shine_eval_metrics", None, n_p, None, n_r, 0.05, WS, WSB, None, None)
    for n, n_fine, n_coarse in ((1, 1, 1), (9, 9, 9), (10, 10, 10), (11, 11, 8), (64, 16, 16), (65, 17, 17), (4000, 1500, 300)):
        add("shine_eval_grid_emit", None, n, None, 0, n_fine, n_coarse, WS, WSB, None)  # (WS / WSB: the grid and its size)
    for n in (1, 2047, 2048, 2049, 5000, 65536, 65537):  # tiles of 8 x 256 points, 32 tile states per slot
        add("shine_frame_filter", None, n, 0, 4, -3.0, 30.0, 1.0, 50.0, WS, WSB, None, None, None)
        add("shine_sem_frame_filter", None, n, 0, 4, None, None, 1.0, 1, 1, -3.0, 30.0, 50.0, WS, WSB, None, None, None, None, None)
    for w, h in ((1, 1), (1025, 1), (640, 480), (32769, 1)):  # tiles of 4 x 256 pixels
        add("shine_depth_unproject", None, 0, w, h, w, 500.0, 500.0, 0.5 * w, 0.5 * h, 1000.0, 5.0, None, -3.0, 30.0, 0.0, 50.0,
            WS, WSB, None, None, None, None)
    for n in (1, 255, 256, 257, 1023, 1024, 1025, 5000, 32768, 32769):  # one flag byte per row, tiles of 4 x 256 rows
        add("shine_pool_window_filter", None, n, None, 1.0, 1, None, None, None, WS, WSB, None, None)
    for n in (1, 63, 64, 65, 4000):  # two int32 lists of n
        grid = (None, n, 1, 1, None, 0.1, None)
        add("shine_knn_search", *grid, 8, -1.0, WS, WSB, None, None, None, None, None)
        add("shine_sor_mean_dist", *grid, 8, WS, WSB, None, None, None, None)
        add("shine_frame_normals", *grid, 0.5, 8, None, WS, WSB, None, None)
    return out


def call(lib, entry, args, ws_ptr, need):
    """the library call with the two workspace arguments filled in; need: a c_size_t, or None for a NULL workspace_bytes"""
    real = [(ws_ptr if a == WS else (C.byref(need) if need is not None else None)) if isinstance(a, str) else a for a in args]
    return getattr(lib, entry)(*real)


def test_host_size_queries_answer_the_recorded_bytes():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    with open(SIZES) as f:
        recorded = json.load(f)
    assert [(r["entry"], r["args"]) for r in recorded] == [(e, a) for e, a in host_cases()], "the golden file covers other cases"
    for r in recorded:
        need = C.c_size_t(0)
        assert call(lib, r["entry"], r["args"], None, need) == 0, (r["entry"], r["args"], lib.shine_error_string(INVALID))
        assert need.value == r["bytes"], (r["entry"], r["args"], need.value, r["bytes"])
        assert call(lib, r["entry"], r["args"], None, None) == INVALID, (r["entry"], r["args"])  # NULL workspace_bytes


# ------------------------------------------------------------------------------------------------------------------ GPU
# A builder makes one call's arguments afresh (seeded inputs, zeroed outputs): -> (entry, args, outputs to compare, host counters).

def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def _scene():
    import frame_nn_oracle as fo

    return fo.scene()  # [3945,3] fp64: three noisy faces, outliers, duplicates


def _stream():
    from shine_mapping_amd import _lib

    return _lib.current_stream_handle()


def _sheet():
    import mesh_post_cases as mp

    v, f = mp.height_field(37, 29)  # 1073 vertices, 2016 triangles
    return v, f.astype(np.int32)


def _sphere(n=17):
    x = np.linspace(-1.0, 1.0, n, dtype=np.float32)
    g = np.stack(np.meshgrid(x, x, x, indexing="ij"), -1)
    return (np.linalg.norm(g, axis=-1) - 0.62).astype(np.float32)


def b_frame_filter():
    p = _dev(np.concatenate([_scene(), np.zeros((3945, 1))], 1), torch.float32)
    out, kept = torch.zeros((len(p), 3), dtype=torch.float64, device="cuda"), C.c_int64(-7)
    return ("shine_frame_filter", [p.data_ptr(), len(p), 0, 4, -3.0, 30.0, 1.0, 15.0, WS, WSB, out.data_ptr(), C.byref(kept), _stream()],
            [out], [kept], [p])


def b_sem_frame_filter():
    p = _dev(_scene(), torch.float32)
    rng = np.random.default_rng(3)
    labels = _dev(rng.choice([0, 1, 10, 40, 252], len(p)).astype(np.int32))
    lut = np.full(65536, -1, np.int32)
    lut[[0, 1, 10, 40, 252]] = [0, 0, 1, 9, 1]
    lut = _dev(lut)
    out, cls = torch.zeros((len(p), 3), dtype=torch.float64, device="cuda"), torch.zeros(len(p), dtype=torch.int32, device="cuda")
    kept, unknown = C.c_int64(-7), C.c_int64(-7)
    return ("shine_sem_frame_filter", [p.data_ptr(), len(p), 0, 3, labels.data_ptr(), lut.data_ptr(), 1.0, 1, 1, -3.0, 30.0, 15.0, WS,
                                       WSB, out.data_ptr(), cls.data_ptr(), C.byref(kept), C.byref(unknown), _stream()],
            [out, cls], [kept, unknown], [p, labels, lut])


def b_depth_unproject():
    w, h = 65, 63  # 4095 pixels: four tiles, the last one short
    rng = np.random.default_rng(4)
    img = _dev(rng.integers(0, 6000, (h, w)).astype(np.int16))  # (uint16 millimetres; torch has no uint16 arithmetic, none needed)
    pts, idx = torch.zeros((w * h, 3), dtype=torch.float64, device="cuda"), torch.zeros(w * h, dtype=torch.int32, device="cuda")
    kept = C.c_int64(-7)
    return ("shine_depth_unproject", [img.data_ptr(), 0, w, h, w, 60.0, 60.0, 32.0, 31.0, 1000.0, 5.0, None, -30.0, 30.0, 0.0, 50.0,
                                      WS, WSB, pts.data_ptr(), idx.data_ptr(), C.byref(kept), _stream()], [pts, idx], [kept], [img])


def b_pool_window_filter():
    from shine_mapping_amd import _lib

    coord = _dev(_scene(), torch.float32)
    n = len(coord)
    a0, a1 = coord.clone(), torch.arange(n, dtype=torch.int32, device="cuda")
    o0, o1 = torch.zeros_like(a0), torch.zeros_like(a1)
    kept = C.c_int64(-7)
    hold = [coord, a0, a1, (C.c_float * 3)(6.0, 5.0, -1.5), _lib.ptr_array([a0.data_ptr(), a1.data_ptr()]),
            _lib.ptr_array([o0.data_ptr(), o1.data_ptr()]), (C.c_int32 * 2)(3, 1)]
    return ("shine_pool_window_filter", [coord.data_ptr(), n, hold[3], 3.0, 2, hold[4], hold[5], hold[6], WS, WSB, C.byref(kept),
                                         _stream()], [o0, o1], [kept], hold)


_GRID = {}


def _grid_args():
    """the search grid over the scene (built once: it is an input here) as the leading arguments of the frame searches"""
    from shine_mapping_amd import evaluation as ev

    if not _GRID:
        g = ev.NNGrid(_dev(_scene()))
        _GRID["g"] = g
        _GRID["args"] = [g.grid.data_ptr(), g.n, g.n_fine, g.n_coarse, ev._d3(g.lo), g.cell,
                         (C.c_int64 * 3)(*[int(c) for c in g.cells_per_axis])]
    return _GRID["g"], list(_GRID["args"])


def b_knn_search():
    g, args = _grid_args()
    idx = torch.zeros((g.n, 8), dtype=torch.int32, device="cuda")
    d2 = torch.zeros((g.n, 8), dtype=torch.float64, device="cuda")
    count = torch.zeros(g.n, dtype=torch.int32, device="cuda")
    rounds = C.c_int32(-7)
    return ("shine_knn_search", args + [8, -1.0, WS, WSB, idx.data_ptr(), d2.data_ptr(), count.data_ptr(), C.byref(rounds), _stream()],
            [idx, d2, count], [rounds], [])


def b_sor_mean_dist():
    g, args = _grid_args()
    avg, stats = torch.zeros(g.n, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    rounds = C.c_int32(-7)
    return ("shine_sor_mean_dist", args + [8, WS, WSB, avg.data_ptr(), stats.data_ptr(), C.byref(rounds), _stream()], [avg, stats],
            [rounds], [])


def b_frame_normals():
    from shine_mapping_amd import evaluation as ev

    g, args = _grid_args()
    out = torch.zeros((g.n, 3), dtype=torch.float64, device="cuda")
    return ("shine_frame_normals", args + [0.5, 16, ev._d3((0.0, 0.0, 0.0)), WS, WSB, out.data_ptr(), _stream()], [out], [], [])


def b_eval_bounds():
    p, out = _dev(_scene()), torch.zeros(6, dtype=torch.float64, device="cuda")
    return ("shine_eval_bounds", [p.data_ptr(), len(p), WS, WSB, out.data_ptr(), _stream()], [out], [], [p])


def b_eval_sample_mesh():
    v, f = _sheet()
    v, f, n = _dev(v), _dev(f), 3001
    out, tri = torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    return ("shine_eval_sample_mesh", [v.data_ptr(), len(v), f.data_ptr(), len(f), n, 11, None, WS, WSB, out.data_ptr(),
                                       tri.data_ptr(), _stream()], [out, tri], [], [v, f])


def _voxel_origin(p, voxel):
    return (C.c_double * 3)(*[float(x) - 0.5 * voxel for x in p.min(0)])


def b_eval_voxel_down():
    s = _scene()
    p, o = _dev(s), _voxel_origin(s, 0.25)
    out, keys = torch.zeros((len(p), 3), dtype=torch.float64, device="cuda"), torch.zeros(len(p), dtype=torch.int64, device="cuda")
    m = C.c_int64(-7)
    return ("shine_eval_voxel_down", [p.data_ptr(), len(p), o, 0.25, WS, WSB, out.data_ptr(), keys.data_ptr(), C.byref(m), _stream()],
            [out, keys], [m], [p, o])


def b_voxel_down_attr():
    s = _scene()
    p, o, att = _dev(s), _voxel_origin(s, 0.25), _dev(np.random.default_rng(5).random((len(s), 3)))
    out, aout = torch.zeros((len(p), 3), dtype=torch.float64, device="cuda"), torch.zeros((len(p), 3), dtype=torch.float64, device="cuda")
    keys, m = torch.zeros(len(p), dtype=torch.int64, device="cuda"), C.c_int64(-7)
    return ("shine_voxel_down_attr", [p.data_ptr(), att.data_ptr(), 3, len(p), o, 0.25, WS, WSB, out.data_ptr(), aout.data_ptr(),
                                      keys.data_ptr(), C.byref(m), _stream()], [out, aout, keys], [m], [p, o, att])


def b_eval_grid_count():
    s = _scene()
    p, o = _dev(s), (C.c_double * 3)(*[float(x) for x in s.min(0)])
    counts = (C.c_int64 * 2)(-7, -7)
    return ("shine_eval_grid_count", [p.data_ptr(), len(p), o, 0.2, WS, WSB, counts, _stream()], [], [counts], [p, o])


def b_eval_nn_search():
    g, args = _grid_args()
    q = _dev(_scene()[::3] + 0.01)
    nq = len(q)
    idx, dist = torch.zeros(nq, dtype=torch.int32, device="cuda"), torch.zeros(nq, dtype=torch.float64, device="cuda")
    keep, stats = torch.zeros(nq, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    return ("shine_eval_nn_search", args + [q.data_ptr(), nq, 0.5, WS, WSB, idx.data_ptr(), dist.data_ptr(), keep.data_ptr(),
                                            stats.data_ptr(), _stream()], [idx, dist, keep, stats], [], [q])


def b_eval_metrics():
    rng = np.random.default_rng(6)
    dp, dr, out = _dev(rng.random(4001) * 0.1), _dev(rng.random(3001) * 0.1), torch.zeros(8, dtype=torch.float64, device="cuda")
    return ("shine_eval_metrics", [dp.data_ptr(), len(dp), dr.data_ptr(), len(dr), 0.05, WS, WSB, out.data_ptr(), _stream()], [out],
            [], [dp, dr])


def b_mc_count():
    sdf = _dev(_sphere())
    counts = (C.c_int64 * 2)(-7, -7)
    return ("shine_mc_count", [sdf.data_ptr(), None, 17, 17, 17, 0.0, WS, WSB, counts, _stream()], [], [counts], [sdf])


def b_mc_sparse_count():
    import mc_sparse_oracle as so

    values, _, org = so.cut(_sphere(), None, 4)
    v, org = _dev(values), np.ascontiguousarray(org, dtype=np.int64)
    counts = (C.c_int64 * 2)(-7, -7)
    return ("shine_mc_sparse_count", [v.data_ptr(), None, org.ctypes.data_as(C.POINTER(C.c_int64)), len(org), 4, 17, 17, 17, 0.0, WS,
                                      WSB, counts, _stream()], [], [counts], [v, org])


def b_mesh_vertex_normals():
    v, f = _sheet()
    v, f = _dev(v), _dev(f)
    out = torch.zeros((len(v), 3), dtype=torch.float64, device="cuda")
    return ("shine_mesh_vertex_normals", [v.data_ptr(), len(v), f.data_ptr(), len(f), WS, WSB, out.data_ptr(), _stream()], [out], [],
            [v, f])


def b_mesh_cluster_filter():
    import mesh_post_cases as mp

    f = mp.grid_faces(40, 40)  # an open sheet with half of its triangles deleted at random: 1500-odd faces in many clusters
    f = _dev(f[np.random.default_rng(2).random(len(f)) >= 0.5].astype(np.int32))
    out, cl = torch.zeros_like(f), torch.zeros(len(f), dtype=torch.int32, device="cuda")
    kept = C.c_int64(-7)
    return ("shine_mesh_cluster_filter", [f.data_ptr(), len(f), 3, WS, WSB, cl.data_ptr(), out.data_ptr(), C.byref(kept), _stream()],
            [out, cl], [kept], [f])


def b_morton_sort():
    from shine_mapping_amd import _lib

    cfg = _lib.StepConfig()
    cfg.n_levels, cfg.max_level = 3, 12
    coord = _dev(np.random.default_rng(7).uniform(-0.9, 0.9, (4001, 3)), torch.float32)
    perm = torch.zeros(len(coord), dtype=torch.int32, device="cuda")
    return ("shine_morton_sort", [C.byref(cfg), coord.data_ptr(), len(coord), perm.data_ptr(), WS, WSB, _stream()], [perm], [],
            [cfg, coord])


def _sampler(entry):
    def build():
        n = 4000
        idx, parts = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
        bits = _dev(np.random.default_rng(8).integers(-2 ** 31, 2 ** 31, 1000 // 32 + 1).astype(np.int32))
        state = torch.zeros(4, dtype=torch.int64, device="cuda")
        tail = [idx.data_ptr(), None, 0, bits.data_ptr(), parts.data_ptr(), WS, WSB, _stream()]
        head = {"shine_sample_sorted": [1000, n, 5, 9], "shine_sample_sorted_dev": [1000, n, 5, state.data_ptr()],
                "shine_sample_sorted_slice": [1000, n, 0, n, 5, 9, None]}[entry]
        return entry, head + tail, [idx, parts, state], [], [bits]

    return build


def b_touched_index():
    from shine_mapping_amd import _lib

    rng, rows = np.random.default_rng(9), [300, 4000]
    flags = [_dev((rng.random(r) < 0.3).astype(np.uint8)) for r in rows]
    idx = [torch.zeros(r, dtype=torch.int32, device="cuda") for r in rows]
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    hold = [flags, _lib.ptr_array([f.data_ptr() for f in flags]), _lib.i64_array(rows), _lib.ptr_array([t.data_ptr() for t in idx])]
    return ("shine_touched_index", [2, hold[1], hold[2], hold[3], counts.data_ptr(), WS, WSB, _stream()], idx + [counts], [], hold)


def b_rows_pack():
    from shine_mapping_amd import _lib

    rng, n_rows, cap, tail_n = np.random.default_rng(10), 4000, 1024, 40
    flags = _dev((rng.random(n_rows) < 0.2).astype(np.uint8))
    bucket = _dev(rng.standard_normal(n_rows * 8 + tail_n), torch.float32)
    msg = torch.zeros(int(_lib.lib().shine_rows_message_words(cap, tail_n)), dtype=torch.int32, device="cuda")
    return ("shine_rows_pack", [flags.data_ptr(), n_rows, None, 0, bucket.data_ptr(), n_rows * 8, tail_n, cap, msg.data_ptr(), WS, WSB,
                                _stream()], [msg, bucket, flags], [], [])


_TREE = {}


def b_plan_batch():
    if not _TREE:
        fx = load_golden("maicity_bce_L3")
        _, octree, _ = product_from_golden(fx)
        _TREE.update(octree=octree, coord=octree._check_coord(fx["coord"].cuda()), t=octree._require_tables(with_ranks=True))
    octree, coord = _TREE["octree"], _TREE["coord"]
    n, L = coord.shape[0], octree.featured_level_num
    cfg = octree.step_config(kernel_variant=0x800)  # (the counting sort at any size: the path that uses the workspace)
    perm, slots = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, L), dtype=torch.int32, device="cuda")
    return ("shine_plan_batch", [_TREE["t"].handle, C.byref(cfg), coord.data_ptr(), n, perm.data_ptr(), slots.data_ptr(), None, 0, WS,
                                 WSB, _stream()], [perm, slots], [], [cfg])


def _plan_canonical(outs):
    """The order inside a bucket comes from atomics (csrc/shine_plan.hip: "order inside a bucket is arbitrary") and the points of a
    bucket share their slots, so two runs agree in: the slot rows in visiting order, every point's own slot row, and perm as a
    set.  An untouched output (all zeros) is returned as it is."""
    perm, slots = outs
    if not bool(perm.any()):
        return [perm, slots]
    by_point = torch.zeros_like(slots).index_copy_(0, perm.long(), slots)
    return [slots, by_point, perm.sort().values]


CANONICAL = {"shine_plan_batch": _plan_canonical}


def _importance_chunks(bs, down_rate):
    """bs = 64: chunks sorted in LDS, the workspace is a token 256 bytes; bs = 20000 (> 16384): the radix form, whose keys, values
    and rocPRIM temporaries lie in the workspace"""
    def build():
        n = 4001
        perm = _dev(np.random.default_rng(11).permutation(n).astype(np.int32))
        idx, n_chunks = torch.zeros(n, dtype=torch.int32, device="cuda"), -(-n // (bs * down_rate))
        begin = (C.c_int64 * (n_chunks + 1))(*([-7] * (n_chunks + 1)))
        return ("shine_importance_chunks", [perm.data_ptr(), n, bs, down_rate, idx.data_ptr(), begin, n_chunks, WS, WSB, _stream()],
                [idx], [begin], [perm])

    return build


BUILDERS = [b_frame_filter, b_sem_frame_filter, b_depth_unproject, b_pool_window_filter, b_knn_search, b_sor_mean_dist,
            b_frame_normals, b_eval_bounds, b_eval_sample_mesh, b_eval_voxel_down, b_voxel_down_attr, b_eval_grid_count,
            b_eval_nn_search, b_eval_metrics, b_mc_count, b_mc_sparse_count, b_mesh_vertex_normals, b_mesh_cluster_filter,
            b_morton_sort, _sampler("shine_sample_sorted"), _sampler("shine_sample_sorted_dev"),
            _sampler("shine_sample_sorted_slice"), b_touched_index, b_rows_pack, b_plan_batch, _importance_chunks(64, 2),
            _importance_chunks(20000, 1)]
IDS = ["frame_filter", "sem_frame_filter", "depth_unproject", "pool_window_filter", "knn_search", "sor_mean_dist", "frame_normals",
       "eval_bounds", "eval_sample_mesh", "eval_voxel_down", "voxel_down_attr", "eval_grid_count", "eval_nn_search", "eval_metrics",
       "mc_count", "mc_sparse_count", "mesh_vertex_normals", "mesh_cluster_filter", "morton_sort", "sample_sorted",
       "sample_sorted_dev", "sample_sorted_slice", "touched_index", "rows_pack", "plan_batch", "importance_chunks",
       "importance_chunks_radix"]


def _counter_values(counters):
    return [list(c) if hasattr(c, "__len__") else c.value for c in counters]


def _run(lib, build, extra, fill):
    """one real call with a workspace of the queried size + extra bytes, filled with `fill` -> (outputs, counters, bytes)"""
    entry, args, outs, counters, _hold = build()
    need = C.c_size_t(0)
    assert call(lib, entry, args, None, need) == 0, (entry, lib.shine_error_string(INVALID))
    before = _counter_values(counters)
    ws = torch.full((need.value + extra,), fill, dtype=torch.uint8, device="cuda")
    size = C.c_size_t(need.value + extra)
    rc = call(lib, entry, args, ws.data_ptr(), size)
    torch.cuda.synchronize()
    assert rc == 0, (entry, rc, lib.shine_error_string(rc))
    assert _counter_values(counters) != before or not counters, entry  # (the sentinels were replaced: the call did run)
    return CANONICAL.get(entry, list)([o.clone() for o in outs]), _counter_values(counters), need.value


@pytest.mark.gpu
@pytest.mark.parametrize("build", BUILDERS, ids=IDS)
def test_exact_workspace_gives_the_bits_of_a_larger_one_and_a_shorter_one_is_refused(build):
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    outs_a, counters_a, need = _run(lib, build, 0, 0xFF)
    outs_b, counters_b, need_b = _run(lib, build, 4096, 0x00)
    print("%s: %d bytes" % (build()[0], need))
    assert need == need_b and need > 0
    assert counters_a == counters_b
    for a, b in zip(outs_a, outs_b):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # one byte short: refused before anything runs
    entry, args, outs, counters, _hold = build()
    before, outs_before = _counter_values(counters), [o.clone() for o in outs]
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    assert call(lib, entry, args, ws.data_ptr(), C.c_size_t(need - 1)) == INVALID
    assert b"workspace too small" in lib.shine_error_string(INVALID), lib.shine_error_string(INVALID)
    torch.cuda.synchronize()
    assert _counter_values(counters) == before
    for a, b in zip(outs, outs_before):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.gpu
def test_by_value_sizes_refuse_a_short_workspace():
    """shine_mc_emit and shine_eval_grid_emit re-use the workspace of their count call and cannot be queried: the same refusal"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    entry, args, _, counts, hold = b_mc_count()
    need = C.c_size_t(0)
    assert call(lib, entry, args, None, need) == 0
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    assert call(lib, entry, args, ws.data_ptr(), need) == 0 and counts[0][0] > 0
    verts = torch.zeros((counts[0][0], 3), dtype=torch.float32, device="cuda")
    faces = torch.zeros((counts[0][1], 3), dtype=torch.int32, device="cuda")
    emit = args[:6] + [ws.data_ptr(), need.value - 1, verts.data_ptr(), faces.data_ptr(), _stream()]
    assert lib.shine_mc_emit(*emit) == INVALID and b"shine_mc_emit: workspace too small" in lib.shine_error_string(INVALID)
    torch.cuda.synchronize()
    assert not bool(verts.any()) and not bool(faces.any())

    entry, args, _, counts, hold = b_eval_grid_count()
    assert call(lib, entry, args, None, need) == 0
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    assert call(lib, entry, args, ws.data_ptr(), need) == 0
    n_fine, n_coarse = counts[0][0], counts[0][1]
    gneed = C.c_size_t(0)
    emit = [args[0], args[1], ws.data_ptr(), need.value - 1, n_fine, n_coarse]
    assert lib.shine_eval_grid_emit(*emit, None, C.byref(gneed), _stream()) == 0 and gneed.value > 0
    grid = torch.zeros(gneed.value, dtype=torch.uint8, device="cuda")
    assert lib.shine_eval_grid_emit(*emit, grid.data_ptr(), C.byref(gneed), _stream()) == INVALID
    assert b"shine_eval_grid_emit: workspace too small" in lib.shine_error_string(INVALID)
    torch.cuda.synchronize()
    assert not bool(grid.any())
