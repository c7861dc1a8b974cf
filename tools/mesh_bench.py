"""Meshing measurements (DESIGN.md "Meshing"): marching cubes on a 1024 x 1024 x 256 grid holding a sparse terrain-like surface,
and the Mesher's recon_bbx_mesh / recon_octree_mesh end to end on a synthetic maicity-sized map (briefly trained, so that its
SDF has a surface), with the query and the marching cubes timed apart.

    python tools/mesh_bench.py [--out profiles/mesh_bench.json] [--quick]

Times are device events around synchronised work (CUDA-graph-free, warm: every shape runs once before it is timed).  Kernel
times and the kernel share come from a separate `rocprofv3 --kernel-trace --stats` run of `--quick`.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # MI355X_MICROARCH.md: spec peak; ~6.3 TB/s achievable (float4 copy)


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


def terrain(X=1024, Y=1024, Z=256):
    """negated-SDF-like field in voxel units: a rolling ground, a few buildings and spheres (positive inside)"""
    x = torch.arange(X, device="cuda", dtype=torch.float32)[:, None, None]
    y = torch.arange(Y, device="cuda", dtype=torch.float32)[None, :, None]
    z = torch.arange(Z, device="cuda", dtype=torch.float32)[None, None, :]
    h = 60.0 + 12.0 * torch.sin(x / 53.0) * torch.cos(y / 71.0) + 4.0 * torch.sin((x + 2 * y) / 17.0)
    v = h - z
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(24):
        cx, cy = (torch.rand(2, generator=g) * torch.tensor([X - 100.0, Y - 100.0]) + 50).tolist()
        w, d, hh = (torch.rand(3, generator=g) * torch.tensor([40.0, 40.0, 120.0]) + torch.tensor([10.0, 10.0, 20.0])).tolist()
        box = torch.minimum(torch.minimum(w / 2 - (x - cx).abs(), d / 2 - (y - cy).abs()), (60.0 + hh) - z)
        v = torch.maximum(v, box)
    return v.contiguous()


def mc_section(res, reps, quick):
    from shine_mapping_amd.mesher import marching_cubes

    shape = (512, 512, 256) if quick else (1024, 1024, 256)
    sdf = terrain(*shape)
    n = sdf.numel()
    t, (v, f) = timed(lambda: marching_cubes(sdf), reps)
    res["marching_cubes"] = dict(grid=list(shape), points=n, verts=int(v.shape[0]), faces=int(f.shape[0]), ms=t,
                                 points_per_s=n / (t * 1e-3), output_bytes=int(v.numel() * 4 + f.numel() * 4))
    mask = torch.ones(shape, dtype=torch.bool, device="cuda")
    t2, _ = timed(lambda: marching_cubes(sdf, mask), reps)
    res["marching_cubes"]["ms_with_mask"] = t2
    res["marching_cubes"]["grid_bytes_per_ms"] = n * 4 / t
    res["marching_cubes"]["hbm_peak_GBps"] = HBM_PEAK / 1e9


def train(wl, iters):
    from shine_mapping_amd import StepOptions, fused_train_step

    cfg, octree, dec, pool = wl.cfg, wl.octree, wl.decoder, wl.pool
    params = list(octree.hier_features) + list(dec.fused_params())
    opt = torch.optim.Adam(params, lr=0.01)
    opts = StepOptions(sigma=cfg.sigma_sigmoid)
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(iters):
        idx = torch.randint(0, pool.coord.shape[0], (8192,), device="cuda", generator=g)
        fused_train_step(octree, dec, pool.coord[idx], pool.sdf_label[idx], pool.weight[idx], opts)
        opt.step()
        opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()


class Box:
    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def get_min_bound(self):
        return np.asarray(self.lo, np.float64)

    def get_max_bound(self):
        return np.asarray(self.hi, np.float64)


def mesher_section(res, reps, quick):
    from shine_mapping_amd import synth
    from shine_mapping_amd.mesher import Mesher, marching_cubes

    t0 = time.time()
    wl = synth.build_workload("maicity", frames=20 if quick else 100, device="cuda", seed=42)
    train(wl, 100 if quick else 400)
    cfg = wl.cfg
    cfg.mc_mask_on = True
    cfg.min_cluster_vertices = 300
    res["map"] = dict(kind="maicity", frames=20 if quick else 100, build_and_train_s=time.time() - t0,
                      nodes=[int(t.shape[0]) - 1 for t in wl.octree.hier_features])
    m = Mesher(cfg, wl.octree, wl.decoder, None)
    lo = (wl.pool.coord.min(0).values / cfg.scale).cpu().numpy()
    hi = (wl.pool.coord.max(0).values / cfg.scale).cpu().numpy()
    box = Box(lo, hi)
    tmp = tempfile.mkdtemp()
    for vox in ((0.2,) if quick else (0.2, 0.1)):
        coord, num, _ = m.get_query_from_bbx(box, vox)
        shape = tuple(int(v) for v in num)
        tq, (sdf, mask) = timed(lambda: m._fill_grid(coord, shape, m._check_level(), True), reps)
        tm, (v, f) = timed(lambda: marching_cubes(sdf, mask), reps)
        del coord, sdf, mask
        te, mesh = timed(lambda: m.recon_bbx_mesh(box, vox, os.path.join(tmp, "b.ply"), None), max(1, reps // 2))
        res["recon_bbx_mesh_%g" % vox] = dict(grid=list(shape), points=int(np.prod(shape)), query_ms=tq, mc_ms=tm,
                                              mc_over_query=tm / tq, end_to_end_ms=te, verts=int(v.shape[0]),
                                              faces=int(f.shape[0]), faces_after_filter=int(len(np.asarray(mesh.triangles))))
    level = wl.octree.max_level - wl.octree.featured_level_num + 1
    for mc_res in ((0.2,) if quick else (0.2, 0.1)):
        tg, (sdf, mask, _, _) = timed(lambda: m.octree_grid_device(level, mc_res), reps)
        tm, (v, f) = timed(lambda: marching_cubes(sdf, mask), reps)
        shape = list(sdf.shape)
        del sdf, mask
        te, mesh = timed(lambda: m.recon_octree_mesh(level, mc_res, os.path.join(tmp, "o.ply"), None), max(1, reps // 2))
        res["recon_octree_mesh_%g" % mc_res] = dict(query_level=level, grid=shape, points=int(np.prod(shape)),
                                                    grid_assembly_ms=tg, mc_ms=tm, end_to_end_ms=te, verts=int(v.shape[0]),
                                                    faces=int(f.shape[0]),
                                                    faces_after_filter=int(len(np.asarray(mesh.triangles))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mesh_bench.json")
    ap.add_argument("--quick", action="store_true", help="smaller grid and map, one timed rep (for the profiler run)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench.py measures on the GPU; none is visible")
    from shine_mapping_amd import build

    build.build(verbose=False)
    reps = 1 if a.quick else a.reps
    res = dict(device=torch.cuda.get_device_name(0), reps=reps)
    mc_section(res, reps, a.quick)
    mesher_section(res, reps, a.quick)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
