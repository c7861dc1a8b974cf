"""Evaluation measurements: the nearest-neighbour search at 10^5 / 10^6 / 10^7 points per side on two
surface-like clouds 3 cm apart (with and without 5 % of the queries farther than the truncation from everything), every other
stage, the cell-size sweep behind evaluation.CELL_FACTOR, `eval_mesh` end to end on a synthetic maicity map against a
ground-truth cloud cast from the analytic scene (the project's first quality numbers: recorded, not asserted), and the CPU
stand-in for the reference's method on the same box and clouds: scipy's cKDTree with 16 workers (open3d's KD-tree, which the
reference queries one point at a time from Python, is not installed here).

    python tools/eval_bench.py [--out profiles/eval_bench.json] [--quick]

Times are device events around synchronised work, warm (every shape runs once before it is timed), median of 5.  Kernel times
come from a separate `rocprofv3 --kernel-trace --stats` run of `--quick`.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY = 6.3e12  # MI355X_MICROARCH.md: achievable copy rate
SPACING, TRUNC = 0.02, 2.0
CENTRE = np.array([1500.0, -900.0, 40.0])


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def sphere(n, radius, seed, sigma=0.002):
    """Fibonacci sphere with noise, built on the device in fp64"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(n, dtype=torch.float64, device="cuda") + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = torch.sqrt(1.0 - z * z)
    p = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], 1) * radius
    return p + torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=g) * sigma + torch.as_tensor(CENTRE, device="cuda")


def pair(n, outliers):
    radius = math.sqrt(n * SPACING ** 2 / (4 * math.pi))  # ~SPACING between neighbours
    ref, qry = sphere(n, radius, 1), sphere(n, radius + 0.03, 2)
    if outliers:
        g = torch.Generator(device="cuda").manual_seed(3)
        k = n // 20
        where = torch.randperm(n, device="cuda", generator=g)[:k]
        d = torch.randn((k // 2, 3), dtype=torch.float64, device="cuda", generator=g)
        d = d / d.norm(dim=1, keepdim=True) * torch.rand((k // 2, 1), dtype=torch.float64, device="cuda", generator=g) ** (1 / 3)
        c = torch.as_tensor(CENTRE, device="cuda")
        qry[where[:k // 2]] = c + d * max(radius - TRUNC - 0.5, 0.0)  # deep inside the sphere
        far = torch.rand((k - k // 2, 3), dtype=torch.float64, device="cuda", generator=g) * 10.0
        qry[where[k // 2:]] = c + torch.tensor([radius + 20.0, 0.0, 0.0], dtype=torch.float64, device="cuda") + far
    return ref, qry


def cpu_tree(ref, qry):
    try:
        from scipy.spatial import cKDTree
    except Exception as e:
        return dict(skipped="scipy does not import: %s" % type(e).__name__)
    r, q = ref.cpu().numpy(), qry.cpu().numpy()
    t0 = time.perf_counter()
    tree = cKDTree(r)
    t1 = time.perf_counter()
    tree.query(q, k=1, workers=16)
    t2 = time.perf_counter()
    return dict(build_s=t1 - t0, query_s=t2 - t1, queries_per_s=len(q) / (t2 - t1), workers=16)


def nn_section(res, reps, quick, cpu_max):
    from shine_mapping_amd import evaluation as ev

    out = {}
    for n in ((100000, 1000000) if quick else (100000, 1000000, 10000000)):
        row = {}
        for name, outl in (("clean", False), ("outliers_5pct", True)):
            ref, qry = pair(n, outl)
            t_all, r = timed(lambda: ev.nn_correspondence(ref, qry, TRUNC, False, spacing=SPACING), reps)
            grid = ev.NNGrid(ref, spacing=SPACING)
            t_build, _ = timed(lambda: ev.NNGrid(ref, spacing=SPACING), reps)
            t_query, _ = timed(lambda: grid.query(qry, TRUNC), reps)
            st = grid.query(qry, TRUNC, stats=True)
            row[name] = dict(call_ms=t_all, grid_build_ms=t_build, sort_and_search_ms=t_query, queries_per_s=n / (t_all * 1e-3),
                             search_queries_per_s=n / (t_query * 1e-3), kept=int(r.keep.sum()), fine_cells=grid.n_fine,
                             coarse_cells=grid.n_coarse, points_per_fine_cell=n / grid.n_fine, max_coarse_cells_one_query=st[3],
                             max_fine_cells_one_query=st[4], bound_coarse_cells=grid.max_coarse_cells(TRUNC),
                             # what the search has to move at least: the query in, the answer out, every reference point once
                             necessary_bytes=n * (24 + 13) + n * 28)
            if n <= cpu_max:
                row[name]["cpu_ckdtree"] = cpu_tree(ref, qry)
                if "query_s" in row[name]["cpu_ckdtree"]:
                    row[name]["device_over_cpu"] = row[name]["cpu_ckdtree"]["query_s"] / (t_all * 1e-3)
            else:
                row[name]["cpu_ckdtree"] = dict(skipped="not run at this size (--cpu-max)")
            del ref, qry, grid, r
        row["outlier_over_clean"] = row["outliers_5pct"]["call_ms"] / row["clean"]["call_ms"]
        out[str(n)] = row
    res["nn_correspondence"] = out
    # the cell-size sweep behind evaluation.CELL_FACTOR
    n = 1000000
    sweep = {}
    for name, outl in (("clean", False), ("outliers_5pct", True)):
        ref, qry = pair(n, outl)
        for factor in (1.0, 1.5, 2.0, 3.0, 4.0):
            grid = ev.NNGrid(ref, cell=factor * SPACING)
            t, _ = timed(lambda: grid.query(qry, TRUNC), reps)
            sweep.setdefault(name, {})[str(factor)] = dict(sort_and_search_ms=t, points_per_fine_cell=n / grid.n_fine)
    res["cell_factor_sweep_1e6"] = sweep


def stages_section(res, reps, quick):
    from shine_mapping_amd import evaluation as ev
    from tools.mesh_bench import terrain
    from shine_mapping_amd.mesher import marching_cubes

    v, f = marching_cubes(terrain(256, 256, 128) if quick else terrain(512, 512, 256))
    v = v.double() * 0.1 + torch.as_tensor(CENTRE, device="cuda")
    n = 2000000 if quick else 10000000
    lo, hi = ev.bounds(v)
    out = dict(mesh=dict(verts=int(v.shape[0]), faces=int(f.shape[0])), samples=n)
    out["bounds_ms"], _ = timed(lambda: ev.bounds(v), reps)
    out["crop_mesh_ms"], _ = timed(lambda: ev.crop_mesh(v, f, lo + 5.0, hi - 5.0), reps)
    out["sample_points_uniformly_ms"], pts = timed(lambda: ev.sample_points_uniformly(v, f, n, seed=1), reps)
    out["voxel_down_sample_ms"], ds = timed(lambda: ev.voxel_down_sample(pts, SPACING), reps)
    out["voxel_points_out"] = int(ds.shape[0])
    d = torch.rand(n, dtype=torch.float64, device="cuda")
    out["distance_sums_ms"], _ = timed(lambda: ev.distance_sums(d, d, 0.05), reps)
    res["stages"] = out


def ground_truth(cfg, seed=42, device="cuda"):
    """the synthetic maicity street in metres, cast densely from sensor positions along it (synth.cast_scan knows the scene
    analytically); the same boxes and the same shift as synth.make_frames"""
    from shine_mapping_amd import synth

    g = torch.Generator().manual_seed(seed)
    lo, hi = synth._boxes(cfg.street_len, g, n=20)
    lo, hi = lo.to(device), hi.to(device)
    dirs = synth.sensor_dirs(256, 1800, device=device)
    shift = torch.tensor([cfg.street_len / 2, 0.0, 0.0], device=device)
    pts = []
    for x in np.arange(0.0, cfg.street_len, 2.0):
        o = torch.tensor([float(x), 0.0, 1.8], device=device)
        pts.append(synth.cast_scan(o, dirs, lo, hi, max_range=cfg.pc_radius_m, min_range=cfg.min_range_m) - shift)
    return torch.cat(pts).double()


def map_section(res, reps, quick):
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd import synth
    from shine_mapping_amd.mesher import Mesher
    from tools.mesh_bench import Box, train

    wl = synth.build_workload("maicity", frames=20 if quick else 100, device="cuda", seed=42)
    iters = 200 if quick else 2000
    train(wl, iters)
    cfg = wl.cfg
    cfg.mc_mask_on = True
    cfg.min_cluster_vertices = 300
    m = Mesher(cfg, wl.octree, wl.decoder, None)
    lo = (wl.pool.coord.min(0).values / cfg.scale).cpu().numpy()
    hi = (wl.pool.coord.max(0).values / cfg.scale).cpu().numpy()
    tmp = tempfile.mkdtemp()
    m.recon_bbx_mesh(Box(lo, hi), 0.2 if quick else 0.1, os.path.join(tmp, "m.ply"), None)
    v, f = m.last_mesh_device
    gt = ground_truth(cfg)
    kw = dict(down_sample_res=0.02, threshold=0.1, truncation_acc=0.2, truncation_com=2.0,  # eval/evaluator.py's maicity setup
              mesh_sample_point=2000000 if quick else 10000000)
    t, metrics = timed(lambda: ev.eval_mesh((v, f), gt, **kw), max(1, reps // 2))
    res["eval_mesh_synthetic_maicity"] = dict(train_iters=iters, mesh=dict(verts=int(v.shape[0]), faces=int(f.shape[0])),
                                              gt_points=int(gt.shape[0]), settings=kw, end_to_end_ms=t, metrics=metrics,
                                              note="quality of a briefly trained synthetic map: recorded, not asserted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/eval_bench.json")
    ap.add_argument("--quick", action="store_true", help="smaller sizes, one timed rep, no CPU stand-in (for the profiler run)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-max", type=int, default=1000000, help="largest size the 16-thread cKDTree stand-in is run at")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on the GPU; none is visible")
    from shine_mapping_amd import build

    build.build(verbose=False)
    reps = 1 if a.quick else a.reps
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, spacing=SPACING, truncation=TRUNC, hbm_copy_Bps=HBM_COPY,
               cpu_stand_in="scipy.spatial.cKDTree(...).query(k=1, workers=16) on the same box; open3d does not import here")
    nn_section(res, reps, a.quick, 0 if a.quick else a.cpu_max)
    stages_section(res, reps, a.quick)
    map_section(res, reps, a.quick)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
