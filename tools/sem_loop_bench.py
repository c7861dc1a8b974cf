"""The semantic training loop (semantic_on) on one GPU: loop.GraphedIteration(sem=...) — Tier B, {fused step, semantic step
(csrc/shine_sem_step.hip), tail [, the head's Adam]} replayed as a HIP graph — against the Tier A iteration it replaces.

    python tools/sem_loop_bench.py [--iters 200] [--warmup 40] [--out profiles/sem_loop_bench.json]

Per batch size (4096 and 2^16 points of the `maicity` synthetic workload), in ONE run:
  tier_b_train / tier_b_frozen   the semantic Tier B iteration, head training / head frozen (freeze_model, shine_incre.py:94-97)
  tier_a                         the Tier A iteration exactly as tools/semantic_bench.py measures it ("hip": query_feature -> sdf ->
                                 sem_label_prob -> BCE + NLL -> zero_grad -> backward -> fused Adam with the semantic group)
  tier_b_plain                   the non-semantic GraphedIteration on the same pool (its launches are untouched by semantic_on)
  kernel                         the semantic kernel's average time from one `rocprofv3 --kernel-trace --stats` run of its own
Every case runs in a fresh child process under its own `timeout -k`; iteration times are medians of 5 windows of device-event
time (ms per iteration), taken with the profiler off.  ratio_tier_a_over_tier_b = tier_a / tier_b_train.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REPEATS = 5
N_CLASS = 21
FATAL_EXITS = (124, 137, 134, 139)  # timeout's two, SIGABRT, SIGSEGV


def _median_windows(run, iters):
    import torch

    times = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(REPEATS):
        ev[0].record()
        run(iters)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / iters)
    times.sort()
    return {"ms_per_iter": times[len(times) // 2], "windows_ms": times}


def child_tier_b(n, mode, iters, warmup):
    sys.path.insert(0, ROOT)
    import torch

    import semantic_bench
    from shine_mapping_amd import StepOptions, optim, synth
    from shine_mapping_amd.loop import GraphedIteration, SemTerm
    from shine_mapping_amd.sampler import SortedPool

    wl, sem = semantic_bench._workload()
    cfg = wl.cfg
    cfg.semantic_on, cfg.ray_loss, cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = True, False, 0.01, 1e-15, True, 1.0
    octree, dec, pl = wl.octree, wl.decoder, wl.pool
    if mode == "frozen":
        for p in sem.parameters():
            p.requires_grad_(False)
    labels = synth.semantic_labels(pl.coord, pl.weight, N_CLASS)
    pool = SortedPool(octree, pl.coord, pl.sdf_label, pl.weight, seed=5, sem_label=labels, n_class=N_CLASS)
    if mode == "plain":
        opt = optim.setup_optimizer(cfg, list(octree.parameters()), dec.fused_params(), None, None)
        term = None
    else:
        opt = optim.setup_optimizer(cfg, list(octree.parameters()), list(dec.parameters()), list(sem.parameters()), None)
        term = SemTerm(sem, float(getattr(cfg, "weight_s", 1.0)), 1)
    g = GraphedIteration(octree, dec, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), n, sem=term)
    g.run(warmup)
    torch.cuda.synchronize()
    rec = _median_windows(g.run, iters)
    rec.update(native=bool(g.native), levels=int(octree.featured_level_num), loss=float(g.loss),
               sem_loss=float(g.sem_loss) if g.sem_loss is not None else None)
    print(json.dumps(rec))


def child_tier_a(n, iters, warmup):
    import semantic_bench

    semantic_bench.child_iteration(n, "hip", iters, warmup)  # (prints its own record)


def run_child(args, timeout, prefix=()):
    cmd = list(prefix) + ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--child"] + \
        [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        rec = {"error": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1500:]}
        # a time limit, an abort, a segmentation fault or a GPU fault: nothing more is started on that card
        rec["fatal"] = (r.returncode in FATAL_EXITS or r.returncode < 0
                        or "illegal memory access" in r.stderr or "HSA_STATUS_ERROR" in r.stderr)
        return rec
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(n, iters, warmup):
    """one profiled run of the training-head loop; the kernel-stats rows of k_sem_step, k_step_v3, k_finish and k_adam"""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="sem_loop_prof_")
    try:
        r = run_child(["tier_b", n, "train", "--iters", iters, "--warmup", warmup], 900,
                      prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"])
        if "error" in r:
            return r
        rows, keys = {}, ("k_sem_step", "k_step_v3", "k_finish", "k_adam")
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key in keys:
                    if key in row.get("Name", ""):
                        rows[key] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                     "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        if not rows:  # (no stats table: the same figures from the trace's start / end timestamps)
            spans = {}
            for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    for key in keys:
                        if key in row.get("Kernel_Name", ""):
                            spans.setdefault(key, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
            for key, v in spans.items():
                rows[key] = {"calls": len(v), "avg_us": sum(v) / len(v) / 1e3, "min_us": min(v) / 1e3, "max_us": max(v) / 1e3}
        return rows or {"error": "no kernel-stats rows found"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sem_loop_bench.json"))
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
        raise SystemExit("sem_loop_bench needs a GPU: nothing is measured without one")
    rec = {"device": torch.cuda.get_device_name(0), "workload": "maicity (synthetic), %d classes" % N_CLASS, "iters": a.iters,
           "warmup": a.warmup, "sizes": {}}
    def finish(code):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
        print("wrote", a.out)
        sys.exit(code)

    for n in (4096, 1 << 16):
        it = max(20, a.iters // (8 if n > 4096 else 1))
        row = rec["sizes"][str(n)] = {}
        for key, args in (("tier_b_train", ["tier_b", n, "train"]), ("tier_b_frozen", ["tier_b", n, "frozen"]),
                          ("tier_a", ["tier_a", n]), ("tier_b_plain", ["tier_b", n, "plain"]), ("kernel", None)):
            # (a replayed Tier B iteration is tens of microseconds: ten times the iterations for windows of comparable length)
            if key == "kernel":
                row[key] = kernel_stats(n, it * 10, a.warmup)
            else:
                row[key] = run_child(args + ["--iters", it * (10 if key != "tier_a" else 1), "--warmup", a.warmup], 600)
            print("N=%d %s: %s" % (n, key, row[key]), flush=True)
            if row[key].get("fatal"):
                rec["stopped"] = "N=%d %s: %s; the sweep ends here" % (n, key, row[key]["error"])
                finish(1)
        if "ms_per_iter" in row["tier_a"] and "ms_per_iter" in row["tier_b_train"]:
            row["ratio_tier_a_over_tier_b"] = row["tier_a"]["ms_per_iter"] / row["tier_b_train"]["ms_per_iter"]
    finish(0)


if __name__ == "__main__":
    main()
