"""Brick-route meshing measurements: marching cubes over the occupied bricks against the dense route.

    python tools/mesh_sparse_bench.py [--out profiles/mesh_sparse_bench.json] [--stats profiles/mesh_sparse_kernel_stats.txt] [--quick]

  (a) fits     the two synthetic-maicity cases of tools/mesh_bench.py (0.2 m and 0.1 m; 100 frames, 400 training steps), where the
               dense grid fits: recon_octree_mesh and recon_bbx_mesh by both routes in the SAME process — the query (dense grid
               assembly / brick assembly), the marching cubes (marching_cubes / marching_cubes_sparse), the call end to end,
               and torch.cuda.max_memory_allocated over the call.  The two routes' meshes are compared (they must be equal).
  (b) large    a synthetic kitti_large octree (8.4 km serpentine, leaf 0.3 m) at mc_res_m = 0.1, query level = the top featured
               level: what the dense route would need, then the brick route: bricks, V, F, times, peak memory.  The features are
               untrained (the decoder's bias is shifted so that level 0 crosses the masked points): the surface of a random
               field, denser than a trained map's.
  (c) stats    `rocprofv3 --kernel-trace --stats` over a --quick run of (a): per-kernel times.

Every section is a fresh child process under its own `timeout -k`; after a child that was killed or crashed nothing more is
started.  Times are device events around synchronised work, warm, median of --reps.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _peak(fn):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def _same(a, b):
    import numpy as np

    return all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))) for k in ("triangles", "vertices", "vertex_normals"))


def child_fits(reps, quick):
    import numpy as np
    import torch

    from mesh_bench import Box, timed, train
    from shine_mapping_amd import synth
    from shine_mapping_amd.mesher import Mesher, marching_cubes, marching_cubes_sparse

    t0 = time.time()
    wl = synth.build_workload("maicity", frames=20 if quick else 100, device="cuda", seed=42)
    train(wl, 100 if quick else 400)
    cfg = wl.cfg
    cfg.mc_mask_on = True
    cfg.min_cluster_vertices = 300
    res = {"map": dict(kind="maicity", frames=20 if quick else 100, build_and_train_s=time.time() - t0,
                       nodes=[int(t.shape[0]) - 1 for t in wl.octree.hier_features])}
    m = Mesher(cfg, wl.octree, wl.decoder, None)
    box = Box((wl.pool.coord.min(0).values / cfg.scale).cpu().numpy(), (wl.pool.coord.max(0).values / cfg.scale).cpu().numpy())
    tmp = tempfile.mkdtemp()
    level = wl.octree.max_level - wl.octree.featured_level_num + 1
    e2e_reps = max(1, reps // 2)
    for vox in ((0.2,) if quick else (0.2, 0.1)):
        # ---- recon_octree_mesh
        tq_d, (sdf, mask, _, _) = timed(lambda: m.octree_grid_device(level, vox), reps)
        tm_d, (v, f) = timed(lambda: marching_cubes(sdf, mask), reps)
        grid = list(sdf.shape)
        del sdf, mask
        tq_s, (vals, bmask, org, shape, _, _) = timed(lambda: m.octree_bricks_device(level, vox), reps)
        tm_s, (v2, f2) = timed(lambda: marching_cubes_sparse(vals, bmask, org, shape), reps)
        bricks, B = int(vals.shape[0]), int(vals.shape[1])
        equal = bool(torch.equal(v, v2) and torch.equal(f, f2))
        del vals, bmask
        te_d, md = timed(lambda: m.recon_octree_mesh(level, vox, os.path.join(tmp, "od.ply"), None, sparse=False), e2e_reps)
        te_s, ms = timed(lambda: m.recon_octree_mesh(level, vox, os.path.join(tmp, "os.ply"), None, sparse=True), e2e_reps)
        pk_d, _ = _peak(lambda: m.recon_octree_mesh(level, vox, os.path.join(tmp, "od.ply"), None, sparse=False))
        pk_s, _ = _peak(lambda: m.recon_octree_mesh(level, vox, os.path.join(tmp, "os.ply"), None, sparse=True))
        res["recon_octree_mesh_%g" % vox] = dict(
            query_level=level, grid=grid, points=int(np.prod(grid)), bricks=bricks, brick_edge=B, brick_points=bricks * B ** 3,
            verts=int(v.shape[0]), faces=int(f.shape[0]), meshes_equal=equal and _same(md, ms),
            dense=dict(query_ms=tq_d, mc_ms=tm_d, end_to_end_ms=te_d, peak_bytes=int(pk_d)),
            sparse=dict(query_ms=tq_s, mc_ms=tm_s, end_to_end_ms=te_s, peak_bytes=int(pk_s)))
        # ---- recon_bbx_mesh
        def dense_query():
            coord, num, _ = m.get_query_from_bbx(box, vox)
            return m._fill_grid(coord, tuple(int(n) for n in num), m._check_level(), True)

        tq_d, (sdf, mask) = timed(dense_query, reps)
        tm_d, (v, f) = timed(lambda: marching_cubes(sdf, mask), reps)
        grid = list(sdf.shape)
        del sdf, mask
        tq_s, (vals, bmask, org, shape, _) = timed(lambda: m.bbx_bricks_device(box, vox), reps)
        tm_s, (v2, f2) = timed(lambda: marching_cubes_sparse(vals, bmask, org, shape), reps)
        bricks, B = int(vals.shape[0]), int(vals.shape[1])
        equal = bool(torch.equal(v, v2) and torch.equal(f, f2))
        del vals, bmask
        te_d, md = timed(lambda: m.recon_bbx_mesh(box, vox, os.path.join(tmp, "bd.ply"), None, sparse=False), e2e_reps)
        te_s, ms = timed(lambda: m.recon_bbx_mesh(box, vox, os.path.join(tmp, "bs.ply"), None, sparse=True), e2e_reps)
        pk_d, _ = _peak(lambda: m.recon_bbx_mesh(box, vox, os.path.join(tmp, "bd.ply"), None, sparse=False))
        pk_s, _ = _peak(lambda: m.recon_bbx_mesh(box, vox, os.path.join(tmp, "bs.ply"), None, sparse=True))
        res["recon_bbx_mesh_%g" % vox] = dict(
            grid=grid, points=int(np.prod(grid)), bricks=bricks, brick_edge=B, brick_points=bricks * B ** 3,
            verts=int(v.shape[0]), faces=int(f.shape[0]), meshes_equal=equal and _same(md, ms),
            dense=dict(query_ms=tq_d, mc_ms=tm_d, end_to_end_ms=te_d, peak_bytes=int(pk_d)),
            sparse=dict(query_ms=tq_s, mc_ms=tm_s, end_to_end_ms=te_s, peak_bytes=int(pk_s)))
    print(json.dumps(res))


def child_large(reps, quick):
    import torch

    from mesh_bench import timed
    from shine_mapping_amd import Decoder, FeatureOctree, synth
    from shine_mapping_amd.mesher import Mesher, dense_grid_bytes, marching_cubes_sparse

    t0 = time.time()
    cfg = synth.make_config("kitti_large", device="cuda")
    cfg.mc_mask_on = True
    torch.manual_seed(42)
    octree = FeatureOctree(cfg)
    dec = Decoder(cfg).cuda()
    frames = 300 if quick else 2800
    for c, _, w in synth.make_frames(cfg, frames, 64, 300, 42, "cuda"):
        octree.update(c[w > 0], False)
    torch.cuda.synchronize()
    m = Mesher(cfg, octree, dec, None)
    level, mc_res = octree.max_level - octree.featured_level_num + 1, 0.1
    lay = m.octree_grid_layout(level, mc_res)
    res = dict(kind="kitti_large", frames=frames, build_s=time.time() - t0, nodes=[int(t.shape[0]) - 1 for t in octree.hier_features],
               query_level=level, mc_res_m=mc_res, block_edge=int(lay[2]), grid=[int(v) for v in lay[4]],
               dense_grid_bytes=int(dense_grid_bytes(lay[4])), free_bytes=int(torch.cuda.mem_get_info()[0]))
    res["dense_fits"] = res["dense_grid_bytes"] <= res["free_bytes"]
    vals, bmask, org, shape, _, _ = m.octree_bricks_device(level, mc_res)
    with torch.no_grad():  # an untrained map: move level 0 into the masked values
        dec.fused_params()[5].add_(float(vals[bmask.bool()][::97].median()))
    del vals, bmask
    tq, (vals, bmask, org, shape, _, _) = timed(lambda: m.octree_bricks_device(level, mc_res), reps)
    tm, (v, f) = timed(lambda: marching_cubes_sparse(vals, bmask, org, shape), reps)
    res.update(bricks=int(vals.shape[0]), brick_edge=int(vals.shape[1]), brick_points=int(vals.numel()), verts=int(v.shape[0]),
               faces=int(f.shape[0]), query_ms=tq, mc_ms=tm)
    del vals, bmask, v, f
    tmp = tempfile.mkdtemp()
    # (the drivers' call: no keyword; normals on, the cluster filter on)
    te, mesh = timed(lambda: m.recon_octree_mesh(level, mc_res, os.path.join(tmp, "large.ply"), None), 1)
    pk, _ = _peak(lambda: m.recon_octree_mesh(level, mc_res, os.path.join(tmp, "large.ply"), None, estimate_normal=False,
                                              filter_isolated_mesh=False))
    res.update(end_to_end_ms=te, faces_after_filter=int(len(mesh.triangles)), peak_bytes_mesh_only=int(pk),
               ply_bytes=os.path.getsize(os.path.join(tmp, "large.ply")))
    print(json.dumps(res))


BAD_EXITS = (124, 137, 134, 139, -6, -9, -11)  # killed at the limit, aborted or crashed: nothing more goes to the device


def run_child(args, timeout, prefix=()):
    cmd = ["timeout", "-k", "10", str(timeout)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        return {"error": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1500:]}, r.returncode
    return json.loads(r.stdout.strip().splitlines()[-1]), 0


def kernel_stats(out_path, timeout):
    """per-kernel times of a --quick run of (a), from rocprofv3's kernel_stats csv (a run of its own: no counters, no other
    tracing)"""
    d = tempfile.mkdtemp()
    rec, rc = run_child(["fits", "--quick", "--reps", 1], timeout, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "sparse",
                                                                          "--output-format", "csv", "--"])
    found = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    lines = ["rocprofv3 --kernel-trace --stats over `tools/mesh_sparse_bench.py --child fits --quick --reps 1`", ""]
    if found:
        with open(found[-1]) as fh:
            rows = fh.read().splitlines()
        lines += rows[:41]
    else:
        lines.append("no kernel_stats csv was written (%s)" % rec.get("error", "?"))
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sparse_bench.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "mesh_sparse_kernel_stats.txt"))
    ap.add_argument("--quick", action="store_true", help="smaller maps, one timed rep")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out: fits, large, stats")
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    if a.child is not None:
        {"fits": child_fits, "large": child_large}[a.child[0]](reps, a.quick)
        return
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mesh_sparse_bench.py measures on the GPU; none is visible")
    from shine_mapping_amd import build

    build.build(verbose=False)
    rec = dict(device=torch.cuda.get_device_name(0), reps=reps, quick=bool(a.quick))
    skip = set(a.skip.split(","))
    flags = ["--reps", reps] + (["--quick"] if a.quick else [])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, limit in (("fits", 900), ("large", 1500)):
        if name in skip:
            continue
        rec[name], rc = run_child([name] + flags, limit)
        print("%s: %s" % (name, json.dumps(rec[name])[:2000]), flush=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
        if rc in BAD_EXITS:
            raise SystemExit("section %s ended with exit %d: stopping here" % (name, rc))
    if "stats" not in skip:
        kernel_stats(a.stats, 600)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
