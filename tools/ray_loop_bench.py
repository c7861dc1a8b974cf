#!/usr/bin/env python
"""A training iteration of a ray-rendering map (ray_loss, main_loss_type dr / dr_neus), two routes on the synthetic KITTI-like map:

    tier_a   the loop body tools/loss_modes_bench.py times: query_feature -> Decoder.sdf -> sigmoid(pred / sigma_size) ->
             losses.batch_ray_rendering_loss (one HIP launch) [+ get_gradient + eikonal] -> zero_grad -> backward -> fused Adam with
             the sigma_size group, on batches of rays made up front — the only route before the graphed loop took ray mode;
    loop     loop.GraphedIteration(ray=RayTerm(...)) on a sampler.RayPool: {sorted draw of rays [+ the batch's surface count],
             k_ray_step (ops.fused_ray_step), graph-safe Adam} replayed as a captured stream graph (--unroll iterations per graph).

Cells: 4096 rays x 6 samples and 8192 rays x 9 samples (the sizes of loss_modes_bench.py) x {dr, dr_neus} x {plain, + eikonal}.  In
one process the two routes alternate --rounds times; every window is at least --window seconds of iterations after warm-up, timed
with device events, and every window is recorded.  A cell counts as WON when the loop's slowest window is below Tier A's fastest.
Then, per cell, one child process under `rocprofv3 --kernel-trace --stats` (no counters) replays the loop for --trace-iters
iterations: the kernel-stats rows of k_ray_step, k_ray_surf_count, the draw and k_adam* go into the document.  A child that ends on
a time limit, an abort or a fault ends the sweep: nothing more is started on that card.

    python tools/ray_loop_bench.py --out profiles/ray_loop_bench.json
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FATAL_EXITS = (124, 134, 137, 139)
KERNELS = ("k_ray_step", "k_ray_surf_count", "k_sample", "k_adam")
SURFACE_N = 3


def build(frames, samples, pool_rays):
    """the map, a decoder, sigma_size and a ray-major pool of `pool_rays` rays of `samples` samples"""
    import torch

    from shine_mapping_amd import Decoder, synth

    wl = synth.build_workload("kitti", frames=frames, device="cuda", seed=42, tree_level_feat=3, surface_sample_n=SURFACE_N,
                              free_sample_n=samples - SURFACE_N)
    cfg = wl.cfg
    cfg.ray_loss, cfg.opt_adam, cfg.adam_eps, cfg.lr_level_reduce_ratio, cfg.semantic_on = True, True, 1e-15, 1.0, False
    torch.manual_seed(0)
    wl.ray_decoder = Decoder(cfg)
    wl.sigma_size = torch.nn.Parameter(torch.ones(1, device="cuda"))
    gen = torch.Generator(device="cuda").manual_seed(1)
    pts = wl.pool.coord[wl.pool.weight > 0]
    origin = pts.mean(0) + torch.tensor([0.0, 0.0, 1.8 * cfg.scale], device="cuda")
    hit = pts[torch.randint(0, pts.shape[0], (pool_rays,), device="cuda", generator=gen)]
    coord, _, weight = synth.sample_rays(hit, origin, cfg, gen)
    wl.rays = (coord, weight, (coord - origin).norm(dim=1).contiguous(), (hit - origin).norm(dim=1).contiguous())
    return wl, gen


def make_loop(wl, n, samples, neus, eik, unroll):
    from shine_mapping_amd import StepOptions, optim
    from shine_mapping_amd.loop import GraphedIteration, RayTerm
    from shine_mapping_amd.sampler import RayPool

    cfg = wl.cfg
    pool = RayPool(wl.octree, *wl.rays, samples=samples, seed=3)
    opt = optim.setup_optimizer(cfg, list(wl.octree.parameters()), wl.ray_decoder.fused_params(), None, wl.sigma_size)
    opts = StepOptions(sigma=cfg.sigma_sigmoid, ekional_loss_on=eik, weight_e=cfg.weight_e)
    return GraphedIteration(wl.octree, wl.ray_decoder, pool, opt, opts, n, unroll=unroll, ray=RayTerm(wl.sigma_size, neus_on=neus))


def window(fn, iters):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn(iters)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / 1e3


def cells_of(a):
    for spec in a.sizes.split(","):
        n, samples = [int(x) for x in spec.split("x")]
        for mode in a.modes.split(","):
            for term in a.terms.split(","):
                yield n, samples, mode, term


def measure(a):
    import torch

    from shine_mapping_amd import autograd_ops, losses, optim

    cells = []
    built = {}
    for n, samples, mode, term in cells_of(a):
        neus, eik = mode == "dr_neus", term == "eikonal"
        if samples not in built:
            # the same map twice, a copy per route: a captured graph holds the addresses of its parameters' .grad tensors, which
            # the Tier A route's zero_grad(set_to_none=True) would free under it
            built = {samples: (build(a.frames, samples, a.pool_rays), build(a.frames, samples, a.pool_rays))}
        (wl, gen), (wl_loop, _) = built[samples]
        octree, cfg, dec, sigma_size = wl.octree, wl.cfg, wl.ray_decoder, wl.sigma_size
        opt_a = optim.setup_optimizer(cfg, list(octree.parameters()), list(dec.parameters()), None, sigma_size)
        autograd_ops.FUSE_WITH_COORD_GRAD = True
        batches = []
        for _ in range(8):  # (batches made up front, as loss_modes_bench.py makes them)
            ray = torch.randint(0, a.pool_rays, (n,), device="cuda", generator=gen)
            rows = (ray.view(-1, 1) * samples + torch.arange(samples, device="cuda").view(1, -1)).reshape(-1)
            batches.append((wl.rays[0][rows].contiguous(), wl.rays[1][rows].contiguous(), wl.rays[2][rows].contiguous(),
                            wl.rays[3][ray].contiguous()))
        state = {"k": 0}

        def tier_a(iters):
            for _ in range(iters):
                coord, weight, depth, ray_depth = batches[state["k"] % len(batches)]
                state["k"] += 1
                if eik:
                    coord = coord.detach().requires_grad_(True)
                pred = dec.sdf(octree.query_feature(coord))
                pred_ray = torch.sigmoid(pred / sigma_size).reshape(n, -1)
                loss = losses.batch_ray_rendering_loss(depth.reshape(n, -1), pred_ray, ray_depth, neus)
                if eik:
                    g = losses.get_gradient(coord, pred) * cfg.sigma_sigmoid
                    loss = loss + cfg.weight_e * ((g[weight > 0].norm(2, dim=-1) - 1.0) ** 2).mean()
                opt_a.zero_grad(set_to_none=True)
                loss.backward()
                opt_a.step()

        it = make_loop(wl_loop, n, samples, neus, eik, a.unroll)
        routes = {"tier_a": tier_a, "loop": it.run}
        iters = {}
        for name, fn in routes.items():  # warm-up (the loop captures its graphs here), then a window's iteration count
            fn(2 * a.unroll + 1)
            fn(10)
            torch.cuda.synchronize()
            iters[name] = max(10, math.ceil(a.window / (window(fn, 20) / 20)))
        windows = {name: [] for name in routes}
        for _ in range(a.rounds):
            for name, fn in routes.items():
                sec = window(fn, iters[name])
                while sec < a.window:  # (a window that came out short is taken again, longer; the short one is kept too)
                    windows[name].append({"iterations": iters[name], "seconds": sec, "ms_per_iteration": sec / iters[name] * 1e3,
                                          "short": True})
                    iters[name] *= 2
                    sec = window(fn, iters[name])
                windows[name].append({"iterations": iters[name], "seconds": sec, "ms_per_iteration": sec / iters[name] * 1e3})
        full = {k: [w["ms_per_iteration"] for w in ws if not w.get("short")] for k, ws in windows.items()}
        med = {k: statistics.median(v) for k, v in full.items()}
        loss = float(it.loss)
        assert loss == loss, "the loop's loss is NaN"
        cell = {"rays": n, "samples": samples, "mode": mode, "term": term, "windows": windows, "median_ms_per_iteration": med,
                "tier_a_fastest_ms": min(full["tier_a"]), "loop_slowest_ms": max(full["loop"]),
                "tier_a_over_loop": med["tier_a"] / med["loop"], "loop_wins": max(full["loop"]) < min(full["tier_a"]),
                "loop_loss_after": loss, "sigma_size_after": float(wl_loop.sigma_size)}
        cells.append(cell)
        print(json.dumps({k: v for k, v in cell.items() if k != "windows"}), flush=True)
        del it
    return cells, torch.cuda.get_device_name(0), torch.__version__


def trace_child(a):
    """(under rocprofv3) the ray loop at one cell's shape"""
    import torch

    n, samples, mode, term = int(a.trace_child[0]), int(a.trace_child[1]), a.trace_child[2], a.trace_child[3]
    wl, _ = build(a.frames, samples, a.pool_rays)
    it = make_loop(wl, n, samples, mode == "dr_neus", term == "eikonal", 1)
    it.run(a.trace_iters)
    torch.cuda.synchronize()
    assert float(it.loss) == float(it.loss)
    print(json.dumps({"ok": True}))


def kernel_stats(a, cell):
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="ray_loop_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", "timeout", "-k", "10", "300",
               sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--pool-rays", str(a.pool_rays),
               "--trace-iters", str(a.trace_iters), "--trace-child", str(cell["rays"]), str(cell["samples"]), cell["mode"],
               cell["term"]]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            return {"error": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1500:],
                    "fatal": (r.returncode in FATAL_EXITS or r.returncode < 0 or "illegal memory access" in r.stderr
                              or "HSA_STATUS_ERROR" in r.stderr)}
        rows = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if any(k in name for k in KERNELS):
                    rows[name[:160]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                        "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        return rows or {"error": "no kernel-stats rows found"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x6,8192x9", help="rays x samples per ray, comma separated")
    ap.add_argument("--modes", default="dr,dr_neus")
    ap.add_argument("--terms", default="plain,eikonal")
    ap.add_argument("--rounds", type=int, default=3, help="how often the routes alternate")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds of iterations per timed window")
    ap.add_argument("--unroll", type=int, default=5, help="iterations per captured graph of the loop")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--pool-rays", type=int, default=262144)
    ap.add_argument("--trace-iters", type=int, default=200)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", nargs=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_loop_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ray_loop_bench needs a GPU: nothing here is measured on the CPU")
    if a.trace_child:
        return trace_child(a)
    cells, device, version = measure(a)
    doc = {"what": "one training iteration of a ray-rendering map (dr / dr_neus): the Tier A iteration (query_feature -> sdf -> "
                   "sigmoid(pred / sigma_size) -> batch_ray_rendering_loss [+ get_gradient + eikonal] -> backward -> fused Adam) "
                   "against the graphed ray loop ({sorted draw of rays, k_ray_step, graph-safe Adam} as a captured graph), "
                   "alternating in one process; device-event time per window; a cell is won when the loop's slowest window is "
                   "below Tier A's fastest",
           "workload": "synth.build_workload('kitti', frames=%d, seed=42, tree_level_feat=3), %d rays of 3 surface + (S - 3) free "
                       "samples" % (a.frames, a.pool_rays),
           "device": device, "torch": version, "window_seconds_at_least": a.window, "rounds": a.rounds, "unroll": a.unroll,
           "cells": cells}

    def finish(code):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        print("wrote", a.out)
        sys.exit(code)

    if not a.no_trace:
        torch.cuda.synchronize()
        for cell in cells:
            cell["kernel_stats"] = ks = kernel_stats(a, cell)
            print("%d x %d %s %s kernels: %s" % (cell["rays"], cell["samples"], cell["mode"], cell["term"], json.dumps(ks)), flush=True)
            if ks.get("fatal"):
                doc["stopped"] = "%d x %d %s %s: %s; the sweep ends here" % (cell["rays"], cell["samples"], cell["mode"],
                                                                             cell["term"], ks["error"])
                finish(1)
    finish(0)


if __name__ == "__main__":
    main()
