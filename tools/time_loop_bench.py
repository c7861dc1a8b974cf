#!/usr/bin/env python
"""A training iteration of a time-conditioned map, two routes on the synthetic KITTI-like map of tools/time_decoder_bench.py:

    tier_a   query_feature -> time_conditionded_sdf -> sdf_bce_loss [+ get_gradient + eikonal] -> backward -> fused Adam: the split
             Tier A nodes with the HIP decoder (autograd_ops.FusedTimeMLP), a batch drawn with torch.randint — the only route before
             the graphed loop took the time head;
    loop     loop.GraphedIteration with the time-conditioned decoder: {sorted draw, k_time_step (ops.fused_time_step), graph-safe
             Adam} replayed as a captured stream graph (--unroll iterations per graph).

Four cells — N = 4096 and N = 2^18, BCE alone and with the eikonal term.  In one process the two routes alternate --rounds times;
every window is at least --window seconds of iterations after warm-up, timed with device events, and every window is recorded.
Then, per cell, one child process under `rocprofv3 --kernel-trace --stats` (no counters) replays the loop for --trace-iters
iterations and, on the same map with the plain decoder, the two-launch native loop: the kernel-stats rows of k_time_step and of
the fused k_step_v3 at the same shape (the known gap of a lane-per-point kernel), k_finish and k_adam* go into the document.  A
child that ends on a time limit, an abort or a fault ends the sweep: nothing more is started on that card.

    python tools/time_loop_bench.py --out profiles/time_loop_bench.json
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
KERNELS = ("k_time_step", "k_step_v3", "k_finish", "k_adam")


def build(frames):
    import torch

    from shine_mapping_amd import Decoder, synth

    wl = synth.build_workload("kitti", frames=frames, device="cuda", seed=42, tree_level_feat=3)
    cfg = wl.cfg
    cfg.opt_adam, cfg.adam_eps, cfg.lr_level_reduce_ratio = True, 1e-15, 1.0
    torch.manual_seed(0)
    wl.time_decoder = Decoder(cfg, is_time_conditioned=True)
    assert wl.time_decoder.time_fusable
    gen = torch.Generator(device="cuda").manual_seed(1)
    wl.ts = torch.randint(0, frames, (wl.pool.coord.shape[0],), device="cuda", generator=gen).float()  # a frame id per sample
    return wl, gen


def make_loop(wl, n, eik, unroll, timed=True):
    from shine_mapping_amd import StepOptions, optim
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.sampler import SortedPool

    cfg, pl = wl.cfg, wl.pool
    dec = wl.time_decoder if timed else wl.decoder
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3, ts=wl.ts if timed else None)
    opt = optim.setup_optimizer(cfg, list(wl.octree.parameters()), dec.time_params() if timed else dec.fused_params())
    opts = StepOptions(sigma=cfg.sigma_sigmoid, ekional_loss_on=eik, weight_e=cfg.weight_e)
    return GraphedIteration(wl.octree, dec, pool, opt, opts, n, unroll=unroll)


def window(fn, iters):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn(iters)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / 1e3


def measure(a):
    import torch

    from shine_mapping_amd import losses, optim

    # the same map twice, a copy per route: a captured graph holds the addresses of its parameters' .grad tensors, which the
    # Tier A route's zero_grad(set_to_none=True) would free under it
    wl, gen = build(a.frames)
    wl_loop, _ = build(a.frames)
    octree, cfg, dec = wl.octree, wl.cfg, wl.time_decoder
    sigma = cfg.sigma_sigmoid
    opt_a = optim.setup_optimizer(cfg, list(octree.parameters()), list(dec.parameters()))
    cells = []
    for n in [int(s) for s in a.sizes.split(",")]:
        for mode in a.modes.split(","):
            eik = mode == "eikonal"

            def tier_a(iters):
                for _ in range(iters):
                    idx = torch.randint(0, wl.pool.sdf_label.shape[0], (n,), device="cuda", generator=gen)
                    coord, label, weight, ts = wl.pool.coord[idx, :], wl.pool.sdf_label[idx], wl.pool.weight[idx], wl.ts[idx]
                    if eik:
                        coord.requires_grad_(True)
                    pred = dec.time_conditionded_sdf(octree.query_feature(coord), ts)
                    loss = losses.sdf_bce_loss(pred, label, sigma, torch.abs(weight), False, cfg.loss_reduction)
                    if eik:
                        g = losses.get_gradient(coord, pred) * sigma
                        loss = loss + cfg.weight_e * ((g[weight > 0].norm(2, dim=-1) - 1.0) ** 2).mean()
                    opt_a.zero_grad(set_to_none=True)
                    loss.backward()
                    opt_a.step()

            it = make_loop(wl_loop, n, eik, a.unroll)
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
            med = {k: statistics.median(w["ms_per_iteration"] for w in ws if not w.get("short")) for k, ws in windows.items()}
            loss = float(it.loss)
            assert loss == loss, "the loop's loss is NaN"
            cell = {"n": n, "mode": mode, "windows": windows, "median_ms_per_iteration": med,
                    "tier_a_over_loop": med["tier_a"] / med["loop"], "loop_wins": med["loop"] < med["tier_a"],
                    "loop_loss_after": loss}
            cells.append(cell)
            print(json.dumps({k: v for k, v in cell.items() if k != "windows"}), flush=True)
            del it
    return cells, torch.cuda.get_device_name(0), torch.__version__


def trace_child(a):
    """(under rocprofv3) the time loop, then the plain two-launch loop, at one cell's shape"""
    import torch

    n, eik = int(a.trace_child[0]), a.trace_child[1] == "eikonal"
    wl, _ = build(a.frames)
    for timed in (True, False):
        it = make_loop(wl, n, eik, 1, timed=timed)
        it.run(a.trace_iters)
        torch.cuda.synchronize()
        assert float(it.loss) == float(it.loss)
        del it
    print(json.dumps({"ok": True}))


def kernel_stats(a, n, mode):
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="time_loop_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", "timeout", "-k", "10", "300",
               sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--trace-iters", str(a.trace_iters),
               "--trace-child", str(n), mode]
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
    ap.add_argument("--sizes", default="4096,262144")
    ap.add_argument("--modes", default="bce,eikonal")
    ap.add_argument("--rounds", type=int, default=3, help="how often the routes alternate")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds of iterations per timed window")
    ap.add_argument("--unroll", type=int, default=5, help="iterations per captured graph of the loop")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--trace-iters", type=int, default=200)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", nargs=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_loop_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_loop_bench needs a GPU: nothing here is measured on the CPU")
    if a.trace_child:
        return trace_child(a)
    cells, device, version = measure(a)
    doc = {"what": "one training iteration of a time-conditioned map: the Tier A nodes (query_feature -> time_conditionded_sdf -> BCE "
                   "[+ get_gradient + eikonal] -> backward -> fused Adam) against the graphed loop ({sorted draw, k_time_step, "
                   "graph-safe Adam} as a captured graph), alternating in one process; device-event time per window",
           "workload": "synth.build_workload('kitti', frames=%d, seed=42, tree_level_feat=3), a frame id per pool sample" % a.frames,
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
            cell["kernel_stats"] = ks = kernel_stats(a, cell["n"], cell["mode"])
            print("N=%d %s kernels: %s" % (cell["n"], cell["mode"], json.dumps(ks)), flush=True)
            if ks.get("fatal"):
                doc["stopped"] = "N=%d %s: %s; the sweep ends here" % (cell["n"], cell["mode"], ks["error"])
                finish(1)
    finish(0)


if __name__ == "__main__":
    main()
