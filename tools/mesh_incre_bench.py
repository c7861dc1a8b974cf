"""Incremental meshing measurements: Mesher.update_octree_mesh against recon_octree_mesh(sparse=True) — the route
every mesh took before — on the same state, frame by frame.

    python tools/mesh_incre_bench.py [--out profiles/mesh_incre_bench.json] [--frames 32] [--mc-res 0.1,0.05] [--reps 3]

Every resolution of --mc-res has a Mesher (and so a cache) of its own on the one map; the query level is the top featured level.

  (a) frames   the synthetic incremental run of tools/incre_bench.py (the `ncd` preset, 50 iterations of 4096 samples per frame,
               regulariser and importance sweep, decoder frozen after frame 20 as in BASELINE config 4).  After every frame, in ONE
               process and on the same state, the two routes ALTERNATE --reps times: full, update, full, update, ...  The update is
               repeatable because the cache it starts from (the state the previous frame left) is cloned before every call.
  (b) sweep    on the final map: a growing prefix of every level's feature rows is changed by hand (rows are appended frame by
               frame, so a prefix is a region), which makes the update query a chosen share of the blocks; both routes are timed
               the same way at every share, and a least-squares line through the update's medians gives the share at which the
               two cost the same — end to end, and for the query side alone.

Per state and route three kinds of call, each --reps times, medians and all values recorded:
  file     the call as a driver makes it, writing its PLY (every resolution and route has a file of its own);
  nofile   mesh_path=None: the mesh stays on the device and in the returned object, nothing is written;
  phases   the `file` call with a device synchronisation and a time stamp at the phase boundaries, set from outside by wrapping
           mesher.rows_diff_device, Mesher._query_blocks, mesher.marching_cubes_sparse and Mesher._finish: diff (layout, host
           tables, decoder compare, rows diff), mark (node tables, sort, mark, index), query (cache growth, query, scatter,
           brick split), mc, finish for the update; layout, query (allocation, query, assembly, brick split), mc, finish for the
           full route.  "query side" = everything before marching cubes, the same boundary in both.
Times are a host clock around work that ends in a device synchronisation.  The two routes' files are compared at every state.
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Phases:
    """time stamps at the phase boundaries of either route, taken by wrappers around the mesher's own pieces"""

    def __init__(self):
        self.on, self.stamps = False, []

    def stamp(self, name):
        if self.on:
            torch.cuda.synchronize()
            self.stamps.append((name, time.perf_counter()))

    def install(self):
        import shine_mapping_amd.mesher as M

        rows_diff, mc_sparse = M.rows_diff_device, M.marching_cubes_sparse
        query_blocks, finish = M.Mesher._query_blocks, M.Mesher._finish
        ph = self

        def rows_diff_w(*a, **k):
            out = rows_diff(*a, **k)
            ph.stamp("diff")
            return out

        def query_blocks_w(self, *a, **k):  # (a generator function: the stamp is taken when the generator is made)
            ph.stamp("mark")
            return query_blocks(self, *a, **k)

        def mc_sparse_w(*a, **k):
            ph.stamp("query")
            out = mc_sparse(*a, **k)
            ph.stamp("mc")
            return out

        def finish_w(self, *a, **k):
            out = finish(self, *a, **k)
            ph.stamp("finish")
            return out

        M.rows_diff_device, M.marching_cubes_sparse = rows_diff_w, mc_sparse_w
        M.Mesher._query_blocks, M.Mesher._finish = query_blocks_w, finish_w

    def run(self, fn):
        """-> (total ms, {phase: ms}, ms before marching cubes)"""
        torch.cuda.synchronize()
        self.stamps, self.on = [("start", time.perf_counter())], True
        try:
            fn()
        finally:
            self.on = False
        st = self.stamps
        split = {b[0]: (b[1] - a[1]) * 1e3 for a, b in zip(st, st[1:])}
        before_mc = [t for name, t in st if name == "query"][0]
        return (st[-1][1] - st[0][1]) * 1e3, split, (before_mc - st[0][1]) * 1e3


PH = Phases()


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def clone_cache(c):
    """a copy of a Mesher's block cache that a later update cannot change: the update writes into the snapshots, the blocks and
    the device node tables in place, and replaces the other members"""
    if c is None:
        return None
    n = copy.copy(c)
    for name in ("snaps", "dev_keys", "dev_ids"):
        setattr(n, name, [t.clone() if t is not None else None for t in getattr(c, name)])
    n.values = c.values.clone() if c.values is not None else None
    n.masks = c.masks.clone() if c.masks is not None else None
    for name in ("snap_rows", "dev_nodes", "sorted", "node_keys", "node_ids"):
        setattr(n, name, list(getattr(c, name)))
    return n


def med(v):
    return float(np.median(v))


def both_routes(m, level, res, tmp, reps):
    """-> record of one state: both routes in alternation, `reps` calls of each kind"""
    pf, pu = os.path.join(tmp, "full_%g.ply" % res), os.path.join(tmp, "update_%g.ply" % res)
    before = clone_cache(m._mesh_cache)

    def full(path):
        m.recon_octree_mesh(level, res, path, None, sparse=True)

    def update(path):
        m._mesh_cache = clone_cache(before)
        torch.cuda.synchronize()
        return lambda: m.update_octree_mesh(level, res, path)

    t = {k: [] for k in ("full", "update", "full_nofile", "update_nofile", "full_phases", "update_phases")}
    for _ in range(reps):
        t["full"].append(clock(lambda: full(pf)))
        t["update"].append(clock(update(pu)))
    with open(pf, "rb") as a, open(pu, "rb") as b:
        equal = a.read() == b.read()
    stats = dict(m.last_update_stats)
    for _ in range(reps):
        t["full_nofile"].append(clock(lambda: full(None)))
        t["update_nofile"].append(clock(update(None)))
    for _ in range(reps):
        t["full_phases"].append(PH.run(lambda: full(pf)))
        t["update_phases"].append(PH.run(update(pu)))
    assert dict(m.last_update_stats) == stats, "a repeated update must do what the first one did"
    rec = dict(equal=equal, share=stats["requeried_nodes"] / max(stats["nodes"], 1), faces=int(m.last_mesh_device[1].shape[0]))
    rec.update(stats)
    for route in ("full", "update"):
        rec[route + "_ms"], rec[route + "_ms_all"] = med(t[route]), t[route]
        rec[route + "_nofile_ms"], rec[route + "_nofile_ms_all"] = med(t[route + "_nofile"]), t[route + "_nofile"]
        ph = t[route + "_phases"]
        # (the full route's time up to _query_blocks is its layout; the update has spent its diff and mark phases by then)
        rec[route + "_split_ms"] = {("layout" if route == "full" and k == "mark" else k): med([p[1][k] for p in ph]) for k in ph[0][1]}
        rec[route + "_query_side_ms"], rec[route + "_query_side_ms_all"] = med([p[2] for p in ph]), [p[2] for p in ph]
    return rec


def line(tag, r):
    fmt = lambda d: " ".join("%s %.2f" % kv for kv in d.items())
    print("%s: %5d nodes, share %.3f, %s | file: full %.2f update %.2f | nofile: full %.2f update %.2f | query side: full %.2f "
          "update %.2f | full (%s) | update (%s) | equal %s"
          % (tag, r["nodes"], r["share"], r["reason"], r["full_ms"], r["update_ms"], r["full_nofile_ms"], r["update_nofile_ms"],
             r["full_query_side_ms"], r["update_query_side_ms"], fmt(r["full_split_ms"]), fmt(r["update_split_ms"]), r["equal"]),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_incre_bench.json"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--bs", type=int, default=4096)
    ap.add_argument("--freeze-after", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mc-res", default="0.1,0.05", help="comma-separated marching-cubes resolutions (m), each with its own cache")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_incre_bench.py measures on the GPU; none is visible")

    from shine_mapping_amd import Decoder, FeatureOctree, StepOptions, fused_train_step, synth
    from shine_mapping_amd.incre_learning import cal_feature_importance
    from shine_mapping_amd.mesher import Mesher
    from shine_mapping_amd.ops import fused_regularization, touched_flags
    from shine_mapping_amd.optim import setup_optimizer
    from shine_mapping_amd.sampler import SortedPool

    PH.install()
    cfg = synth.make_config("ncd", device="cuda", lr=0.01, opt_adam=True, adam_eps=1e-15, lr_level_reduce_ratio=1.0)
    cfg.mc_mask_on = True
    frames = list(synth.make_frames(cfg, frames=a.frames, beams=64, azimuths=900, seed=42, device="cuda"))
    torch.manual_seed(0)
    octree, dec = FeatureOctree(cfg), Decoder(cfg).cuda()
    opts = StepOptions(sigma=cfg.sigma_sigmoid, loss_reduction="sum")
    resolutions = [float(v) for v in a.mc_res.split(",")]
    meshers = {res: Mesher(cfg, octree, dec) for res in resolutions}
    level = octree.max_level - octree.featured_level_num + 1
    tmp = tempfile.mkdtemp()
    rec = dict(device=torch.cuda.get_device_name(0), preset="ncd", frames=a.frames, iters=a.iters, bs=a.bs, reps=a.reps,
               freeze_after=a.freeze_after, query_level=level, mc_res_m=resolutions, runs={})
    for res in resolutions:
        rec["runs"]["%g" % res] = dict(per_frame=[], sweep=[])

    for fi, (coord, label, weight) in enumerate(frames):
        octree.update(coord[weight > 0], incremental_on=True)
        octree._require_tables(with_ranks=True)
        if fi == a.freeze_after:
            for p in dec.parameters():
                p.requires_grad_(False)
            opts.decoder_grad_on = False
        opt = setup_optimizer(cfg, list(octree.parameters()), dec.fused_params())
        pool = SortedPool(octree, coord, label, weight, seed=fi)
        touched = touched_flags(octree)
        for _ in range(a.iters):
            idx = pool.draw(a.bs)
            fused_train_step(octree, dec, None, None, None, opts, pool=pool, idx=idx, touched=touched)
            fused_regularization(octree, cfg.lambda_forget, touched)
            opt.step(zero_grad=True)
        data = type("Pool", (), {"coord_pool": coord, "sdf_label_pool": label})()
        cal_feature_importance(data, octree, dec, cfg.sigma_sigmoid, a.bs, 2, "sum")
        torch.cuda.synchronize()
        for res, m in meshers.items():
            r = both_routes(m, level, res, tmp, a.reps)
            r["frame"] = fi
            rec["runs"]["%g" % res]["per_frame"].append(r)
            line("res %g frame %2d" % (res, fi), r)

    # (b) a chosen share of the blocks, on the final map
    rows = [int(p.shape[0]) - 1 for p in octree.hier_features]
    for frac in (0.0, 0.01, 0.03, 0.1, 0.2, 0.35, 0.5, 0.75, 1.0):
        with torch.no_grad():
            for p, n in zip(octree.hier_features, rows):
                p.data[:int(n * frac)] *= 1.0001
        for res, m in meshers.items():
            r = both_routes(m, level, res, tmp, a.reps)
            r["rows_changed_fraction"] = frac
            rec["runs"]["%g" % res]["sweep"].append(r)
            line("res %g sweep %.2f" % (res, frac), r)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:  # (the records first: the fits and medians below are derived from them)
        json.dump(rec, fh, indent=1)
    for run in rec["runs"].values():
        share = np.array([r["share"] for r in run["sweep"]])
        fit = {}
        for name in ("", "_nofile", "_query_side"):
            slope, base = np.polyfit(share, np.array([r["update%s_ms" % name] for r in run["sweep"]]), 1)
            full = med([r["full%s_ms" % name] for r in run["sweep"]])
            even = (full - base) / slope if slope > 0 else None
            fit["file" if name == "" else name[1:]] = dict(update_ms_at_share_0=float(base), update_ms_per_unit_share=float(slope),
                                                           full_ms=full, break_even_share=None if even is None else float(even))
        run["fit"] = fit
        inc = [r for r in run["per_frame"] if not r["full"]]
        spread = lambda k: med([(max(r[k]) - min(r[k])) for r in inc])
        run["summary"] = dict(
            frames_incremental=len(inc), all_equal=all(r["equal"] for r in run["per_frame"] + run["sweep"]),
            block_edge=int(round((run["per_frame"][0]["requeried_points"] / run["per_frame"][0]["nodes"]) ** (1 / 3))),
            median_share=med([r["share"] for r in inc]),
            median_ms={k: med([r[k] for r in inc]) for k in ("full_ms", "update_ms", "full_nofile_ms", "update_nofile_ms",
                                                              "full_query_side_ms", "update_query_side_ms")},
            median_update_minus_full_ms={k: med([r["update" + k] - r["full" + k] for r in inc])
                                         for k in ("_ms", "_nofile_ms", "_query_side_ms")},
            median_spread_of_reps_ms={k: spread(k) for k in ("full_ms_all", "update_ms_all", "full_nofile_ms_all",
                                                             "update_nofile_ms_all")},
            median_full_split_ms={k: med([r["full_split_ms"][k] for r in inc]) for k in inc[0]["full_split_ms"]},
            median_update_split_ms={k: med([r["update_split_ms"][k] for r in inc]) for k in inc[0]["update_split_ms"]})
        print(json.dumps(dict(fit=run["fit"], summary=run["summary"])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
