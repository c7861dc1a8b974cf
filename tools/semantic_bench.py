"""The semantic head (semantic_on) on one GPU: csrc/shine_semantic.hip against the torch composite it replaces.

    python tools/semantic_bench.py [--iters 100] [--warmup 20] [--out profiles/semantic_bench.json]

  iteration   the Tier A loop body of shine_batch.py:119-209 with semantic_on (query_feature -> sdf -> sem_label_prob -> BCE +
              NLL -> zero_grad -> backward -> fused Adam with the semantic group) at N = 4096 and 2^16 points; "hip" runs
              Decoder.sem_label_prob, "composite" Decoder._sem_composite (three Linear, two ReLU, log_softmax and their backward)
  mesh        Mesher.query_points labels (query_sem=True, one chunk of 2^20 grid points): shine_sem_query_labels against
              query_feature + the composite's argmax — points per second
Every case runs in a fresh child process under its own `timeout -k`; times are medians of 5 windows (ms per iteration / s).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 5


def _workload():
    import torch

    from shine_mapping_amd import Decoder, synth

    wl = synth.build_workload("maicity", frames=20, beams=32, azimuths=180, device="cuda", seed=3)
    torch.manual_seed(0)
    return wl, Decoder(wl.cfg, is_geo_encoder=False)


def child_iteration(n, impl, iters, warmup):
    sys.path.insert(0, ROOT)
    import torch

    from shine_mapping_amd import autograd_ops, optim, sdf_bce_loss, synth

    wl, sem = _workload()
    cfg = wl.cfg
    cfg.semantic_on, cfg.ray_loss, cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = True, False, 0.01, 1e-15, True, 1.0
    octree, dec = wl.octree, wl.decoder
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), list(dec.parameters()), list(sem.parameters()), None)
    autograd_ops.FUSE_WITH_COORD_GRAD = True
    gen = torch.Generator(device="cuda").manual_seed(5)
    batches = []
    for _ in range(8):
        coord, sdf_label, weight = synth.draw_batch(wl.pool, n, gen)
        batches.append((coord, sdf_label, torch.abs(weight), synth.semantic_labels(coord, weight, 21)))
    head = sem.sem_label_prob if impl == "hip" else sem._sem_composite
    nll = torch.nn.NLLLoss(reduction="mean")

    def step(k):
        coord, sdf_label, weight, sem_label = batches[k % len(batches)]
        feature = octree.query_feature(coord)
        pred = dec.sdf(feature)
        sem_pred = head(feature)
        loss = sdf_bce_loss(pred, sdf_label, cfg.sigma_sigmoid, weight, False, "mean")
        loss = loss + getattr(cfg, "weight_s", 1.0) * nll(sem_pred, sem_label)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    for k in range(warmup):
        step(k)
    torch.cuda.synchronize()
    times = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(REPEATS):
        ev[0].record()
        for k in range(iters):
            step(k)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) / iters)
    times.sort()
    print(json.dumps({"ms_per_iter": times[len(times) // 2], "windows_ms": times}))


def child_mesh(impl, iters, warmup):
    sys.path.insert(0, ROOT)
    import torch

    from shine_mapping_amd.mesher import Mesher, query_labels_device

    wl, sem = _workload()
    octree = wl.octree
    lo, hi = wl.pool.coord.min(0).values, wl.pool.coord.max(0).values
    side = 102
    axes = [torch.linspace(float(lo[k]), float(hi[k]), side, device="cuda") for k in range(3)]
    coord = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    n = coord.shape[0]

    def once():
        with torch.no_grad():
            if impl == "hip":
                return query_labels_device(octree, sem, coord)
            return torch.argmax(sem._sem_composite(octree.query_feature(coord, True)), dim=1)

    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rates = []
    for _ in range(REPEATS):
        ev[0].record()
        for _ in range(iters):
            once()
        ev[1].record()
        torch.cuda.synchronize()
        rates.append(n * iters / (ev[0].elapsed_time(ev[1]) * 1e-3))
    rates.sort()
    # the public path as the mesher runs it (numpy result), once, for the record
    Mesher(wl.cfg, octree, wl.decoder, sem).query_points(coord, n + 1, False, True, False)
    print(json.dumps({"points": n, "points_per_s": rates[len(rates) // 2], "windows_points_per_s": rates}))


def run_child(args, timeout):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        return {"error": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1500:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_bench.json"))
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child is not None:
        kind = a.child[0]
        if kind == "iteration":
            child_iteration(int(a.child[1]), a.child[2], a.iters, a.warmup)
        else:
            child_mesh(a.child[1], max(1, a.iters // 20), max(1, a.warmup // 10))
        return
    import torch

    rec = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "iters": a.iters,
           "warmup": a.warmup, "iteration": {}, "mesh_labels": {}}
    for n in (4096, 1 << 16):
        for impl in ("hip", "composite"):
            r = run_child(["iteration", n, impl, "--iters", a.iters, "--warmup", a.warmup], 600)
            rec["iteration"]["%d/%s" % (n, impl)] = r
            print("iteration N=%d %s: %s" % (n, impl, r), flush=True)
    for impl in ("hip", "composite"):
        r = run_child(["mesh", impl, "--iters", a.iters, "--warmup", a.warmup], 600)
        rec["mesh_labels"][impl] = r
        print("mesh labels %s: %s" % (impl, r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
