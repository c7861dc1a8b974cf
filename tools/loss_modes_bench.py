"""Tier A iteration time per training objective: the HIP losses (csrc/shine_loss_modes.hip, losses.py) against the torch
composites they replace (SHINE_DROPIN_FUSED_LOSS=0), in the drivers' loop body (shine_batch.py:115-209: query_feature -> sdf
-> loss -> zero_grad -> backward -> optimiser step) on the drop-in's classes, with the fused optimiser in both cases (ray modes:
with the learnable sigma_size group).

    python tools/loss_modes_bench.py [--iters 200] [--warmup 30] [--rocprof] [--out profiles/loss_modes_bench.json]

Every (mode, batch, implementation) runs in a fresh child process under its own `timeout -k`; with --rocprof the HIP children
run a second time under `rocprofv3 --kernel-trace --stats` and the loss kernels' rows of the stats are recorded.
  ray modes (dr, dr_neus):   4096 rays x 6 samples, 8192 rays x 9 samples
  point modes (sdf_bce, sdf_l1, sdf_l2): 4096 and 8192 points
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_BATCHES = ((4096, 6), (8192, 9))
POINT_BATCHES = (4096, 8192)
MODES = ("sdf_bce", "sdf_l1", "sdf_l2", "dr", "dr_neus")
REPEATS = 5
LOSS_KERNELS = ("k_ray_render_loss", "k_sdf_diff_loss", "k_bce_loss")


def child(mode, rays, samples, iters, warmup):
    sys.path.insert(0, ROOT)
    import torch

    from shine_mapping_amd import autograd_ops, losses, optim, synth

    hip = os.environ.get("SHINE_DROPIN_FUSED_LOSS", "1") != "0"
    ray_mode = mode in ("dr", "dr_neus")
    ns = 3
    wl = synth.build_workload("maicity", frames=20, beams=32, azimuths=180, device="cuda", seed=3, surface_sample_n=ns,
                              free_sample_n=samples - ns)
    cfg = wl.cfg
    cfg.ray_loss, cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.semantic_on, cfg.lr_level_reduce_ratio = ray_mode, 0.01, 1e-15, True, \
        False, 1.0
    octree, dec = wl.octree, wl.decoder
    sigma_size = torch.nn.Parameter(torch.ones(1, device="cuda"))
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), list(dec.parameters()), None, sigma_size)
    autograd_ops.FUSE_WITH_COORD_GRAD = True
    gen = torch.Generator(device="cuda").manual_seed(5)
    batches = []
    if ray_mode:
        pts = wl.pool.coord[wl.pool.weight > 0]
        origin = pts.mean(0) + torch.tensor([0.0, 0.0, 1.8 * cfg.scale], device="cuda")
        for _ in range(8):
            hit = pts[torch.randint(0, pts.shape[0], (rays,), device="cuda", generator=gen)]
            coord, _, _ = synth.sample_rays(hit, origin, cfg, gen)
            batches.append((coord, (coord - origin).norm(dim=1), (hit - origin).norm(dim=1)))
    else:
        for _ in range(8):
            batches.append(synth.draw_batch(wl.pool, rays, gen))
    ray_fn = losses.batch_ray_rendering_loss if hip else losses.batch_ray_rendering_loss_composite
    diff_fn = losses.sdf_diff_loss if hip else losses.sdf_diff_loss_composite
    bce_fn = losses.sdf_bce_loss if hip else losses._bce_composite

    def iteration(k):
        b = batches[k % len(batches)]
        pred = dec.sdf(octree.query_feature(b[0]))
        if ray_mode:
            pred_ray = torch.sigmoid(pred / sigma_size).reshape(rays, -1)
            loss = ray_fn(b[1].reshape(rays, -1), pred_ray, b[2], mode == "dr_neus")
        else:
            weight = torch.abs(b[2])
            if mode == "sdf_bce":
                loss = bce_fn(pred, b[1], cfg.sigma_sigmoid, weight, False, "mean")
            else:
                loss = diff_fn(pred, b[1], weight, cfg.scale, mode == "sdf_l2")
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    first_loss = float(iteration(0))  # (the same parameters and batch on both sides: the two losses agree here)
    for k in range(1, warmup):
        iteration(k)
    torch.cuda.synchronize()
    blocks = []
    for rep in range(REPEATS):  # the host is the bound at these sizes: the best of a few blocks, and their median
        t0 = time.perf_counter()
        for k in range(iters):
            loss = iteration(k)
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) / iters * 1e6)
    blocks.sort()
    print(json.dumps(dict(mode=mode, rays=rays, samples=samples, impl="hip" if hip else "composite", iter_us=blocks[0],
                          iter_us_median=blocks[len(blocks) // 2], first_loss=first_loss, last_loss=float(loss))))


def _run_child(args, mode, rays, samples, hip, prof_dir=None):
    env = dict(os.environ, SHINE_DROPIN_FUSED_LOSS="1" if hip else "0")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, str(rays), str(samples), "--iters", str(args.iters),
           "--warmup", str(args.warmup)]
    if prof_dir is not None:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "run", "--"] + cmd
    cmd = ["timeout", "-k", "10", str(args.timeout)] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError("child %s %d x %d (%s) failed with %d:\n%s" % (mode, rays, samples, "hip" if hip else "composite",
                                                                         r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def _kernel_stats(prof_dir):
    rows = []
    for path in glob.glob(os.path.join(prof_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                kernel = [k for k in LOSS_KERNELS if k in name]
                if kernel:
                    rows.append(dict(kernel=kernel[0], name=name[:160], calls=int(row.get("Calls", 0)),
                                     avg_us=float(row.get("AverageNs", 0)) / 1e3, min_us=float(row.get("MinNs", 0)) / 1e3,
                                     max_us=float(row.get("MaxNs", 0)) / 1e3))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), int(args.child[2]), args.iters, args.warmup)
        return
    results = []
    for mode in MODES:
        batches = RAY_BATCHES if mode in ("dr", "dr_neus") else [(n, 6) for n in POINT_BATCHES]
        for rays, samples in batches:
            rec = dict(mode=mode, batch="%d rays x %d samples" % (rays, samples) if mode in ("dr", "dr_neus") else
                       "%d points" % rays)
            hip = _run_child(args, mode, rays, samples, True)
            comp = _run_child(args, mode, rays, samples, False)
            rec.update(hip_iter_us=round(hip["iter_us"], 1), composite_iter_us=round(comp["iter_us"], 1),
                       saved_us=round(comp["iter_us"] - hip["iter_us"], 1),
                       hip_iter_us_median=round(hip["iter_us_median"], 1),
                       composite_iter_us_median=round(comp["iter_us_median"], 1),
                       first_loss_hip=hip["first_loss"], first_loss_composite=comp["first_loss"],
                       last_loss_hip=hip["last_loss"], last_loss_composite=comp["last_loss"])
            if args.rocprof:
                d = tempfile.mkdtemp(prefix="loss_modes_prof_")
                try:
                    _run_child(args, mode, rays, samples, True, prof_dir=d)
                    rec["loss_kernels"] = _kernel_stats(d)
                finally:
                    shutil.rmtree(d, ignore_errors=True)
            print(json.dumps(rec), flush=True)
            results.append(rec)
    out = dict(tool="tools/loss_modes_bench.py", iters=args.iters, warmup=args.warmup, repeats=REPEATS,
               iter_us="best of the repeats' per-iteration means (wall clock, synchronised per block)", results=results)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
