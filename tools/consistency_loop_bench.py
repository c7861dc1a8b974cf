"""The training loop with the gradient-consistency term (consistency_loss_on) on one GPU: loop.GraphedIteration(consistency=...) —
Tier B, {fused step, consistency step (csrc/shine_consistency_step.hip), tail} replayed as a HIP graph — against the Tier A
composite iteration.

    python tools/consistency_loop_bench.py [--iters 200] [--warmup 40] [--out profiles/consistency_loop_bench.json]

Per batch size (4096 and 2^16 points of the `maicity` synthetic workload, L = 3), K = 1000 pairs, shifts of up to half a
finest-level cell, in ONE run on the same pool:
  tier_a              (a) the Tier A composite iteration with the term, the reference's lines: the drop-in nodes (query_feature ->
                      sdf, get_gradient) on the batch AND on the K shifted points + sdf_bce_loss + losses.consistency_loss ->
                      zero_grad -> backward -> fused Adam
  tier_b_consistency  (b) Tier B with consistency=ConsistencyTerm(weight_c, K, shift_scale)
  tier_b_plain        (c) Tier B without it (its launches are untouched by the term)
  kernel              the consistency kernel's average time from one `rocprofv3 --kernel-trace --stats` run of its own (no counters)
Every case runs in a fresh child
process under its own `timeout -k`; iteration times are medians of 5 windows of device-event time (ms per iteration), taken with
the profiler off.  ratio_tier_a_over_tier_b = tier_a / tier_b_consistency.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
WEIGHT_C = 1.0
K_PAIRS = 1000


def _setup():
    sys.path.insert(0, ROOT)
    import torch

    import semantic_bench

    wl, _ = semantic_bench._workload()
    cfg = wl.cfg
    cfg.ray_loss, cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = False, 0.01, 1e-15, True, 1.0
    return wl, cfg, 0.5 * cfg.leaf_vox_size * cfg.scale  # shift_scale: half a finest-level cell of the [-1,1] space


def child_tier_b(n, mode, iters, warmup):
    import sem_loop_bench

    wl, cfg, shift_scale = _setup()
    import torch

    from shine_mapping_amd import StepOptions, optim
    from shine_mapping_amd.loop import ConsistencyTerm, GraphedIteration
    from shine_mapping_amd.sampler import SortedPool

    octree, dec, pl = wl.octree, wl.decoder, wl.pool
    pool = SortedPool(octree, pl.coord, pl.sdf_label, pl.weight, seed=5)
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), dec.fused_params(), None, None)
    term = ConsistencyTerm(WEIGHT_C, K_PAIRS, shift_scale, seed=3) if mode == "consistency" else None
    g = GraphedIteration(octree, dec, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), n, consistency=term)
    g.run(warmup)
    torch.cuda.synchronize()
    rec = sem_loop_bench._median_windows(g.run, iters)
    rec.update(native=bool(g.native), levels=int(octree.featured_level_num), loss=float(g.loss),
               consistency_loss=float(g.consistency_loss) if g.consistency_loss is not None else None)
    print(json.dumps(rec))


def child_tier_a(n, iters, warmup):
    import sem_loop_bench

    wl, cfg, shift_scale = _setup()
    import torch

    from shine_mapping_amd import autograd_ops, get_gradient, losses, optim, sdf_bce_loss, synth

    octree, dec = wl.octree, wl.decoder
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), dec.fused_params(), None, None)
    autograd_ops.FUSE_WITH_COORD_GRAD = True
    gen = torch.Generator(device="cuda").manual_seed(5)
    batches = []
    for _ in range(8):
        idx = torch.randint(0, wl.pool.coord.shape[0], (n,), device="cuda", generator=gen)
        batches.append((wl.pool.coord[idx].contiguous(), wl.pool.sdf_label[idx].contiguous(), wl.pool.weight[idx].contiguous()))
    state = {"k": 0}

    def run(iters):
        for _ in range(iters):
            coord, sdf_label, weight = batches[state["k"] % len(batches)]
            state["k"] += 1
            coord = coord.detach().requires_grad_(True)
            pred = dec.sdf(octree.query_feature(coord))
            g = get_gradient(coord, pred) * cfg.sigma_sigmoid
            # shine_batch.py:150-158
            near_index = torch.randint(0, coord.shape[0], (min(K_PAIRS, coord.shape[0]),), device=coord.device)
            random_shift = torch.rand_like(coord) * 2 * shift_scale - shift_scale
            coord_near = (coord.detach() + random_shift)[near_index, :]
            coord_near.requires_grad_(True)
            g_near = get_gradient(coord_near, dec.sdf(octree.query_feature(coord_near))) * cfg.sigma_sigmoid
            loss = sdf_bce_loss(pred, sdf_label, cfg.sigma_sigmoid, torch.abs(weight), False, "mean")
            loss = loss + WEIGHT_C * losses.consistency_loss(g[near_index, :], g_near)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return loss

    loss = run(warmup)
    torch.cuda.synchronize()
    rec = sem_loop_bench._median_windows(run, iters)
    rec.update(levels=int(octree.featured_level_num), loss=float(loss))
    print(json.dumps(rec))


def kernel_stats(n, iters, warmup):
    """one profiled run of the loop with the term; the kernel-stats rows of k_consistency_step, k_step_v3 and k_finish"""
    import csv
    import glob
    import shutil
    import tempfile

    import sem_loop_bench

    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="consistency_loop_prof_")
    try:
        r = run_child(["tier_b", n, "consistency", "--iters", iters, "--warmup", warmup], 900,
                      prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"])
        if "error" in r:
            return r
        rows, keys = {}, ("k_consistency_step", "k_step_v3", "k_finish")
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key in keys:
                    if key in row.get("Name", ""):
                        rows[key] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                     "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        return rows or {"error": "no kernel-stats rows found"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def run_child(args, timeout, prefix=()):
    import subprocess

    import sem_loop_bench

    cmd = list(prefix) + ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--child"] + \
        [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        rec = {"error": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1500:]}
        # a time limit, an abort, a segmentation fault or a GPU fault: nothing more is started on that card
        rec["fatal"] = (r.returncode in sem_loop_bench.FATAL_EXITS or r.returncode < 0
                        or "illegal memory access" in r.stderr or "HSA_STATUS_ERROR" in r.stderr)
        return rec
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_loop_bench.json"))
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child is not None:
        if a.child[0] == "tier_b":
            child_tier_b(int(a.child[1]), a.child[2], a.iters, a.warmup)
        else:
            child_tier_a(int(a.child[1]), a.iters, a.warmup)
        return
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("consistency_loop_bench needs a GPU: nothing is measured without one")
    rec = {"device": torch.cuda.get_device_name(0), "workload": "maicity (synthetic), K = %d pairs, shifts up to half a finest cell, weight_c %g" % (K_PAIRS, WEIGHT_C),
           "iters": a.iters, "warmup": a.warmup, "sizes": {}}

    def finish(code):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print("wrote", a.out)
        sys.exit(code)

    for n in (4096, 1 << 16):
        it = max(20, a.iters // (8 if n > 4096 else 1))
        row = rec["sizes"][str(n)] = {}
        for key, args in (("tier_a", ["tier_a", n]), ("tier_b_consistency", ["tier_b", n, "consistency"]),
                          ("tier_b_plain", ["tier_b", n, "plain"]), ("kernel", None)):
            # (a replayed Tier B iteration is tens of microseconds: ten times the iterations for windows of comparable length)
            if key == "kernel":
                row[key] = kernel_stats(n, it * 10, a.warmup)
            else:
                row[key] = run_child(args + ["--iters", it * (10 if key != "tier_a" else 1), "--warmup", a.warmup], 600)
            print("N=%d %s: %s" % (n, key, row[key]), flush=True)
            if row[key].get("fatal"):
                rec["stopped"] = "N=%d %s: %s; the sweep ends here" % (n, key, row[key]["error"])
                finish(1)
        if "ms_per_iter" in row["tier_a"] and "ms_per_iter" in row["tier_b_consistency"]:
            row["ratio_tier_a_over_tier_b"] = row["tier_a"]["ms_per_iter"] / row["tier_b_consistency"]["ms_per_iter"]
    finish(0)


if __name__ == "__main__":
    main()
