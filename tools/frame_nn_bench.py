"""Frame clean-up measurements: LiDARDataset.process_frame on a synthetic scan of KITTI size (64 beams x 1800
azimuths, `kitti` preset) with neither of config.filter_noise / config.estimate_normal, with each, and with both; the three entry
points of csrc/shine_frame_nn.hip alone on one frame's clouds (the search grid built beforehand); and the number of search
launches the unbounded searches needed (the widening rounds).

    python tools/frame_nn_bench.py [--out profiles/frame_nn_bench.json] [--frames 6] [--quick]

Times are host clocks around work that ends in a device synchronise, warm (the first two frames of a drive are not counted: code
objects load there), median over the counted frames.  The kernels' own times come from a separate
`rocprofv3 --kernel-trace --stats` run of `--quick` (profiles/frame_nn_kernel_stats.txt).  There is no earlier device path to
compare with: the numbers are recorded, not judged.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARAMS = dict(sor_nn=25, sor_std=2.5, normal_radius_m=0.2, normal_max_nn=20)  # the reference's defaults (utils/config.py)


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def frames_ms(drive, frames, skip, **over):
    from shine_mapping_amd import synth
    from shine_mapping_amd.dataset import LiDARDataset

    cfg = synth.dataset_config("kitti", drive, **dict(PARAMS, **over))
    ds = LiDARDataset(cfg, None)
    times = [sync_time(lambda f=f: ds.process_frame(f, incremental_on=True))[0] for f in range(frames)]
    counted = times[skip:]
    return {"ms_per_frame": float(np.median(counted)), "min_max": [float(min(counted)), float(max(counted))],
            "frames_counted": len(counted), "rays_last_frame": int(ds.coord_pool.shape[0] // ds.sampler.S)}


def entry_points_alone(drive, frame_id, reps):
    """each entry point on the cloud process_frame hands it: normals on the cropped frame, SOR and k-NN on the down-sampled one"""
    from shine_mapping_amd import _lib, synth
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd.dataset import LiDARDataset, _frame_grid, frame_filter

    cfg = synth.dataset_config("kitti", drive, **PARAMS)
    ds = LiDARDataset(cfg, None)
    raw = ds.read_point_cloud(os.path.join(cfg.pc_path, ds.pc_filenames[frame_id]))
    cropped = frame_filter(raw, cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius)
    down = ev.voxel_down_sample(cropped, cfg.vox_down_m)
    lib, st = _lib.lib(), _lib.current_stream_handle()
    out = {"points_cropped": int(cropped.shape[0]), "points_down_sampled": int(down.shape[0])}

    def timed(fn):
        ts = []
        for _ in range(reps + 2):
            ts.append(sync_time(fn)[0])
        return float(np.median(ts[2:]))

    for name, cloud in (("grid_build_cropped", cropped), ("grid_build_down_sampled", down)):
        out[name + "_ms"] = timed(lambda: ev.NNGrid(cloud))
    rounds, need = C.c_int32(0), C.c_size_t(0)

    grid, args = _frame_grid(cropped, "bench")
    n = grid.n
    nrm = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    lib.shine_frame_normals(None, *args[1:], cfg.normal_radius_m, cfg.normal_max_nn, None, None, C.byref(need), None, st)
    ws = _lib.workspace(need.value, nrm.device)
    vp = (C.c_double * 3)(0.0, 0.0, 0.0)
    out["shine_frame_normals_ms"] = timed(lambda: _lib.check(lib.shine_frame_normals(
        *args, cfg.normal_radius_m, cfg.normal_max_nn, vp, ws.data_ptr(), C.byref(need), nrm.data_ptr(), st), "shine_frame_normals"))
    out["shine_frame_normals_bytes_written"] = n * 24

    grid, args = _frame_grid(down, "bench")
    n = grid.n
    avg = torch.empty(n, dtype=torch.float64, device="cuda")
    stats = torch.empty(2, dtype=torch.float64, device="cuda")
    lib.shine_sor_mean_dist(None, *args[1:], cfg.sor_nn, None, C.byref(need), None, None, None, st)
    ws = _lib.workspace(need.value, avg.device)
    out["shine_sor_mean_dist_ms"] = timed(lambda: _lib.check(lib.shine_sor_mean_dist(
        *args, cfg.sor_nn, ws.data_ptr(), C.byref(need), avg.data_ptr(), stats.data_ptr(), C.byref(rounds), st), "shine_sor_mean_dist"))
    out["shine_sor_mean_dist_launches"] = int(rounds.value)
    out["shine_sor_mean_dist_bytes_written"] = n * 8 + 16
    k = int(cfg.sor_nn)
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    d2 = torch.empty((n, k), dtype=torch.float64, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    out["shine_knn_search_ms"] = timed(lambda: _lib.check(lib.shine_knn_search(
        *args, k, -1.0, ws.data_ptr(), C.byref(need), idx.data_ptr(), d2.data_ptr(), cnt.data_ptr(), C.byref(rounds), st),
        "shine_knn_search"))
    out["shine_knn_search_launches"] = int(rounds.value)
    out["shine_knn_search_bytes_written"] = n * (12 * k + 4)
    out["grid_bytes_read_at_least"] = n * 28  # every point and its index once; cells and neighbours come from the caches
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "frame_nn_bench.json"))
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--quick", action="store_true", help="3 frames, 2 repetitions of the entry points, no file written")
    a = ap.parse_args()
    from shine_mapping_amd import synth

    frames = 3 if a.quick else a.frames
    skip = 1 if a.quick else 2
    with tempfile.TemporaryDirectory() as tmp:
        drive = synth.write_kitti_drive(tmp, synth.make_config("kitti", device="cuda"), frames=frames, beams=64, azimuths=1800,
                                        device="cuda")
        res = {"scan": "64 x 1800 beams, kitti preset", "frames": frames, "warm_frames_skipped": skip, "parameters": PARAMS,
               "process_frame": {
                   "neither": frames_ms(drive, frames, skip),
                   "filter_noise": frames_ms(drive, frames, skip, filter_noise=True),
                   "estimate_normal": frames_ms(drive, frames, skip, estimate_normal=True),
                   "both": frames_ms(drive, frames, skip, filter_noise=True, estimate_normal=True)},
               "entry_points_one_frame": entry_points_alone(drive, frames - 1, 2 if a.quick else 10)}
    print(json.dumps(res, indent=1))
    if not a.quick:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
