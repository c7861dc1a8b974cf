#!/usr/bin/env python
"""Tier A iteration time with a time-conditioned decoder: the reference's loop body with config.time_conditioned
(shine_batch.py:115-210, :127-130) on this package's classes —

    query_feature -> time_conditionded_sdf -> sdf_bce_loss                                   -> backward -> fused Adam   ("bce")
    query_feature -> time_conditionded_sdf -> sdf_bce_loss + get_gradient + eikonal term     -> backward -> fused Adam   ("eikonal")

on the synthetic KITTI-like map of tools/tier_a_bench.py, at N = 4096 and N = 2^18, with the decoder on the HIP path
(autograd_ops.FusedTimeMLP, csrc/shine_time_mlp.hip) and as the reference's torch composite (--paths; the composite is
Decoder._time_composite called by this tool, there is no switch in the library).  Same process, the two paths alternating
--rounds times; every window is --window seconds of iterations after warm-up, timed with device events, and every window is
recorded.  Writes one JSON document (--out).

    python tools/time_decoder_bench.py --out profiles/time_decoder_bench.json
    python tools/time_decoder_bench.py --sizes 4096 --paths hip --rounds 1 --window 0.2 --out /tmp/x.json   (a run to profile)
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shine_mapping_amd import Decoder, losses, optim, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,262144")
    ap.add_argument("--paths", default="hip,composite", help="which decoder paths to time: hip, composite or both")
    ap.add_argument("--modes", default="bce,eikonal")
    ap.add_argument("--rounds", type=int, default=3, help="how often the paths alternate")
    ap.add_argument("--window", type=float, default=0.6, help="seconds of iterations per timed window")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_decoder_bench needs a GPU: nothing here is measured on the CPU")
    paths = a.paths.split(",")
    wl = synth.build_workload("kitti", frames=a.frames, device="cuda", seed=42, tree_level_feat=3)
    octree, cfg = wl.octree, wl.cfg
    cfg.opt_adam, cfg.adam_eps, cfg.lr_level_reduce_ratio = True, 1e-15, 1.0
    torch.manual_seed(0)
    dec = Decoder(cfg, is_time_conditioned=True)
    assert dec.time_fusable
    sigma = cfg.sigma_sigmoid
    gen = torch.Generator(device="cuda").manual_seed(1)
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), list(dec.parameters()))
    results = []
    for n in [int(s) for s in a.sizes.split(",")]:
        for mode in a.modes.split(","):
            eik = mode == "eikonal"

            def iteration(path):
                coord, label, weight = synth.draw_batch(wl.pool, n, gen)
                ts = torch.randint(0, a.frames, (n,), device="cuda", generator=gen).float()  # a frame id per sample (time_pool)
                if eik:
                    coord.requires_grad_(True)
                feature = octree.query_feature(coord)
                decode = dec.time_conditionded_sdf if path == "hip" else dec._time_composite
                pred = decode(feature, ts)
                loss = losses.sdf_bce_loss(pred, label, sigma, torch.abs(weight), False, cfg.loss_reduction)
                if eik:
                    g = losses.get_gradient(coord, pred) * sigma
                    loss = loss + cfg.weight_e * ((g[weight > 0].norm(2, dim=-1) - 1.0) ** 2).mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                return pred

            def window(path, iters):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(iters):
                    iteration(path)
                end.record()
                end.synchronize()
                return start.elapsed_time(end) / 1e3

            # the two paths compute the same function: one batch through both, before anything is timed
            with torch.no_grad():
                coord, _, _ = synth.draw_batch(wl.pool, n, gen)
                ts = torch.randint(0, a.frames, (n,), device="cuda", generator=gen).float()
                feature = octree.query_feature(coord)
                diff = float((dec.time_conditionded_sdf(feature, ts) - dec._time_composite(feature, ts)).abs().max())
            iters = {}
            for path in paths:  # warm-up, then the iteration count of a window from a short timed run
                for _ in range(10):
                    iteration(path)
                torch.cuda.synchronize()
                iters[path] = max(10, math.ceil(a.window / (window(path, 20) / 20)))
            windows = {path: [] for path in paths}
            for _ in range(a.rounds):
                for path in paths:
                    sec = window(path, iters[path])
                    while sec < a.window * 0.9:  # (a window that came out short is taken again, longer; the short one is kept too)
                        windows[path].append({"iterations": iters[path], "seconds": sec, "ms_per_iteration": sec / iters[path] * 1e3,
                                              "short": True})
                        iters[path] *= 2
                        sec = window(path, iters[path])
                    windows[path].append({"iterations": iters[path], "seconds": sec, "ms_per_iteration": sec / iters[path] * 1e3})
            med = {p: statistics.median(w["ms_per_iteration"] for w in ws if not w.get("short")) for p, ws in windows.items()}
            rec = {"n": n, "mode": mode, "max_abs_pred_difference_between_paths": diff, "windows": windows,
                   "median_ms_per_iteration": med}
            if "hip" in med and "composite" in med:
                rec["composite_over_hip"] = med["composite"] / med["hip"]
            results.append(rec)
            print(json.dumps({k: v for k, v in rec.items() if k != "windows"}), flush=True)
    doc = {"what": "Tier A iteration with a time-conditioned decoder (query_feature -> time_conditionded_sdf -> BCE [+ get_gradient + "
                   "eikonal] -> backward -> fused Adam), HIP decoder path against the torch composite in one process, alternating; "
                   "device-event time per window",
           "workload": "synth.build_workload('kitti', frames=%d, seed=42, tree_level_feat=3)" % a.frames,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_seconds": a.window, "rounds": a.rounds,
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
