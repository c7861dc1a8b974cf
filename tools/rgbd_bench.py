"""RGB-D front-end measurements: RGBDDataset.process_frame on 640 x 480 depth frames of the synthetic room
(synth.write_rgbd_drive, the `rgbd` preset = config/rgbd/rgbd_batch.yaml's values), per frame, next to the only route the parent
commit allowed for the same frames — numpy back-projection on the host (tests/rgbd_oracle.py's function, every valid pixel as
the converter keeps them), mesher.write_ply, LiDARDataset.process_frame on the written file — on the same box, in the same
process, frame by frame in turn.

    python tools/rgbd_bench.py [--out profiles/rgbd_bench.json] [--frames 8] [--reps 2] [--quick]

Times are host clocks around work that ends in a device synchronise, warm (the first two frames of a drive are not counted: code
objects load there), median over the counted frames of `reps` drives.  The stage split runs the stages of one frame one by one
with a synchronise after each (its sum is larger than a frame's time, which synchronises less).  shine_depth_unproject alone:
device events around 200 launches.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of `--quick`
(profiles/rgbd_kernel_stats.txt).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12  # MI355X: specified peak


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class HostRoute:
    """what a user of the parent commit could do with a depth frame: back-project on the host, write the .ply, read it back"""

    def __init__(self, cfg, intrinsics, lidar, folder):
        self.cfg, self.k, self.lidar, self.folder = cfg, intrinsics, lidar, folder

    def process_frame(self, frame_id, names, incremental_on):
        import rgbd_oracle as ro
        from shine_mapping_amd.mesher import write_ply

        k = self.k
        raw = np.load(os.path.join(self.cfg.depth_path, names[frame_id]))
        pts, _ = ro.unproject(raw, k.fx, k.fy, k.cx, k.cy, k.depth_scale, self.cfg.max_depth_m, k.cam_to_sensor)
        write_ply(os.path.join(self.folder, "%06d.ply" % frame_id),
                  [("x", pts[:, 0], "double"), ("y", pts[:, 1], "double"), ("z", pts[:, 2], "double")])
        self.lidar.process_frame(frame_id, incremental_on)


def stage_split(cfg, ds, frame_id):
    """the device route's stages one by one, a synchronise after each"""
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd.dataset import ray_sample, transform_points
    from shine_mapping_amd.rgbd import unproject_depth

    out = {}
    out["read_ms"], raw = sync_time(lambda: ds.read_depth_frame(frame_id))
    out["upload_ms"], dev = sync_time(lambda: torch.from_numpy(raw.view(np.int16)).to(cfg.device))
    box = (cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius)
    out["unproject_ms"], kept = sync_time(lambda: unproject_depth(dev, ds.intrinsics, max_depth_m=ds.max_depth_m, filter=box))
    out["voxel_down_ms"], pts = sync_time(lambda: ev.voxel_down_sample(kept, cfg.vox_down_m))
    out["transform_ms"], pts = sync_time(lambda: transform_points(pts, ds.poses_ref[frame_id]))
    out["map_copy_and_box_ms"], _ = sync_time(lambda: ev.bounds(ev.voxel_down_sample(pts, cfg.map_vox_down_m)))
    out["scale_cast_ms"], pts_s = sync_time(lambda: (pts * cfg.scale).float())
    origin = (ds.poses_ref[frame_id][:3, 3] * cfg.scale).astype(np.float32)
    out["ray_sample_ms"], res = sync_time(lambda: ray_sample(pts_s, origin, ds.sampler, seed=1, stream_id=frame_id, depths=False))
    if ds.octree is not None:
        surf = res["coord"].view(int(pts_s.shape[0]), ds.sampler.S, 3)[:, :ds.sampler.ns].reshape(-1, 3)
        out["octree_update_ms"], _ = sync_time(lambda: ds.octree.update(surf, False))
    out["pixels"], out["points_kept"], out["rays"] = int(raw.size), int(kept.shape[0]), int(pts_s.shape[0])
    return out, dev


def kernel_alone(dev, ds, cfg, reps=200):
    from shine_mapping_amd.rgbd import unproject_depth

    box = (cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius)

    def fn():
        return unproject_depth(dev, ds.intrinsics, max_depth_m=ds.max_depth_m, filter=box, return_index=True)

    for _ in range(10):
        pts, _ = fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / reps * 1e3
    read, written = dev.numel() * dev.element_size(), int(pts.shape[0]) * (24 + 4)
    return dict(pixels=int(dev.numel()), points=int(pts.shape[0]), us_per_call=us, bytes_read=read, bytes_written=written,
                rate_TB_s=(read + written) / (us * 1e-6) / 1e12, share_of_hbm_peak_8TB_s=(read + written) / (us * 1e-6) / HBM_PEAK,
                note="a call = two output allocations, the workspace query, a memset, the launch, an 8-byte copy back and a stream "
                     "synchronise (the count goes to the host); the kernel's own time is in profiles/rgbd_kernel_stats.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "rgbd_bench.json"))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="one short drive, no file written (the profiler's run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_bench.py measures on the GPU only")
    from types import SimpleNamespace

    from shine_mapping_amd import FeatureOctree, synth
    from shine_mapping_amd.dataset import LiDARDataset
    from shine_mapping_amd.rgbd import RGBDDataset, write_poses_kitti

    frames, reps = (4, 1) if args.quick else (args.frames, args.reps)
    folder = tempfile.mkdtemp(prefix="rgbd_bench_")
    drive = synth.write_rgbd_drive(folder, frames=frames, width=640, height=480, focal=525.0, step_m=0.1, yaw_per_frame=0.05)
    host_folder = os.path.join(folder, "host_route", "rgbd_ply")
    os.makedirs(host_folder)
    write_poses_kitti(os.path.join(folder, "host_route", "poses.txt"), drive.poses)
    for f in range(frames):  # (LiDARDataset lists its folder when it is built: the files are rewritten frame by frame below)
        open(os.path.join(host_folder, "%06d.ply" % f), "wb").close()
    result = dict(frame="640 x 480 uint16 depth, rgbd preset (config/rgbd/rgbd_batch.yaml's values), synthetic room", frames=frames,
                  reps=reps, warm_frames_skipped=2)
    for mode, incremental in (("batch", False), ("incremental", True)):
        for with_octree in (False, True):
            ours, theirs = [], []
            for rep in range(reps):
                cfg = synth.rgbd_config("rgbd", drive)
                cfg_h = SimpleNamespace(**vars(cfg))
                cfg_h.__dict__.update(pc_path=host_folder, pose_path=os.path.join(folder, "host_route", "poses.txt"), calib_path="")
                torch.manual_seed(rep)
                ds = RGBDDataset(cfg, FeatureOctree(cfg) if with_octree else None)
                host = HostRoute(cfg, ds.intrinsics, LiDARDataset(cfg_h, FeatureOctree(cfg_h) if with_octree else None), host_folder)
                for f in range(frames):  # interleaved: the same frame on both routes in turn
                    t_ours, _ = sync_time(lambda: ds.process_frame(f, incremental))
                    t_host, _ = sync_time(lambda: host.process_frame(f, ds.pc_filenames, incremental))
                    if f >= 2:
                        ours.append(t_ours)
                        theirs.append(t_host)
                same = len(ds) == len(host.lidar) and torch.equal(ds.coord_pool, host.lidar.coord_pool)
            key = "%s_%s" % (mode, "with_octree" if with_octree else "front_end")
            result[key] = dict(device_ms_per_frame=float(np.median(ours)), host_route_ms_per_frame=float(np.median(theirs)),
                               device_min_max=[float(min(ours)), float(max(ours))],
                               host_min_max=[float(min(theirs)), float(max(theirs))], frames_counted=len(ours),
                               pool_samples_at_end=len(ds), both_routes_gave_the_same_pool=bool(same))
            print(key, json.dumps(result[key]), flush=True)
    cfg = synth.rgbd_config("rgbd", drive)
    ds = RGBDDataset(cfg, FeatureOctree(cfg))
    stage_split(cfg, ds, 0)  # warm
    split, dev = stage_split(cfg, ds, min(3, frames - 1))
    result["stage_split_one_frame"] = split
    result["shine_depth_unproject"] = kernel_alone(dev, ds, cfg, reps=20 if args.quick else 200)
    print(json.dumps(result["stage_split_one_frame"]), flush=True)
    print(json.dumps(result["shine_depth_unproject"]), flush=True)
    if not args.quick:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
