"""Frame front-end measurements: LiDARDataset.process_frame on the 64 x 450-beam synthetic scan of config 4
(the `ncd` preset), per frame, in incremental and in batch mode (window replay on), against the only way the parent commit had
to do the same on the device — torch expressions for filter, crop and window filter, evaluation.voxel_down_sample,
synth.sample_rays, torch.cat for the pools — on the same box, in the same process, frame by frame in turn.

    python tools/frame_bench.py [--out profiles/frame_bench.json] [--frames 12] [--reps 3] [--quick]

Times are host clocks around work that ends in a device synchronise, warm (the first two frames of a drive are not counted: code
objects load there), median over the counted frames of `reps` drives.  `front_end`: the dataset without an octree (the front-end
alone); `with_octree`: with FeatureOctree.update, which is the same call on both sides.  The stage split runs the stages one by
one with a synchronise after each (its sum is larger than a frame's time, which synchronises once).  shine_ray_sample alone:
device events around 200 launches.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of `--quick`
(profiles/frame_kernel_stats.txt).
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

HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12  # MI355X: specified peak / achievable copy rate


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class TorchFrontEnd:
    """the torch composite: what a user of the parent commit could write on the device"""

    def __init__(self, cfg, ds, octree=None):
        self.cfg, self.ds, self.octree = cfg, ds, octree  # (ds: poses and file names only)
        self.gen = torch.Generator(device="cuda").manual_seed(1)
        self.pools = None

    def points(self, frame_id):
        from shine_mapping_amd import evaluation as ev

        cfg = self.cfg
        raw = self.ds.read_point_cloud(os.path.join(cfg.pc_path, self.ds.pc_filenames[frame_id]))
        p = raw[:, :3].double()
        p = p[p[:, 2] > cfg.min_z]
        p = p[torch.linalg.norm(p, dim=1) >= cfg.min_range]
        lo = torch.tensor([-cfg.pc_radius, -cfg.pc_radius, cfg.min_z], dtype=torch.float64, device=p.device)
        hi = torch.tensor([cfg.pc_radius, cfg.pc_radius, cfg.max_z], dtype=torch.float64, device=p.device)
        p = p[((p >= lo) & (p <= hi)).all(1)]
        return ev.voxel_down_sample(p, cfg.vox_down_m)

    def process_frame(self, frame_id, incremental_on):
        from shine_mapping_amd import evaluation as ev
        from shine_mapping_amd import synth
        from shine_mapping_amd.dataset import transform_points

        cfg = self.cfg
        pose = self.ds.poses_ref[frame_id]
        pts = transform_points(self.points(frame_id), pose)
        cur = ev.voxel_down_sample(pts, cfg.map_vox_down_m)
        ev.bounds(cur)
        origin = torch.tensor(pose[:3, 3] * cfg.scale, dtype=torch.float32, device=pts.device)
        coord, label, weight = synth.sample_rays((pts * cfg.scale).float(), origin, cfg, self.gen)
        origin_rep = origin.repeat(coord.shape[0], 1)
        time_rep = torch.tensor(float(frame_id), device=pts.device).repeat(coord.shape[0])
        if self.octree is not None:
            self.octree.update(coord[weight > 0, :], incremental_on)
        new = [coord, weight, label, origin_rep, time_rep]
        if incremental_on or self.pools is None:
            self.pools = new
            return
        mask = (self.pools[0] - origin).norm(2, dim=-1) < cfg.window_radius * cfg.scale
        self.pools = [torch.cat((p[mask], n), 0) for p, n in zip(self.pools, new)]


def stage_split(cfg, ds, frame_id):
    """the device front-end's stages one by one, a synchronise after each"""
    from shine_mapping_amd import evaluation as ev
    from shine_mapping_amd.dataset import frame_filter, ray_sample, transform_points

    out = {}
    out["read_ms"], raw = sync_time(lambda: ds.read_point_cloud(os.path.join(cfg.pc_path, ds.pc_filenames[frame_id])))
    out["filter_ms"], kept = sync_time(lambda: frame_filter(raw, cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius))
    out["voxel_down_ms"], pts = sync_time(lambda: ev.voxel_down_sample(kept, cfg.vox_down_m))
    out["transform_ms"], pts = sync_time(lambda: transform_points(pts, ds.poses_ref[frame_id]))
    out["map_copy_and_box_ms"], _ = sync_time(lambda: ev.bounds(ev.voxel_down_sample(pts, cfg.map_vox_down_m)))
    out["scale_cast_ms"], pts_s = sync_time(lambda: (pts * cfg.scale).float())
    origin = (ds.poses_ref[frame_id][:3, 3] * cfg.scale).astype(np.float32)
    out["ray_sample_ms"], res = sync_time(lambda: ray_sample(pts_s, origin, ds.sampler, seed=1, stream_id=frame_id, depths=False))
    out["points_raw"], out["points_kept"], out["rays"] = int(raw.shape[0]), int(kept.shape[0]), int(pts_s.shape[0])
    return out, pts_s, origin


def sampler_alone(pts_s, origin, ds, reps=200):
    from shine_mapping_amd import synth
    from shine_mapping_amd.dataset import ray_sample

    m, S = int(pts_s.shape[0]), ds.sampler.S
    out = {k: torch.empty(s, device="cuda") for k, s in (("coord", (m * S, 3)), ("sdf_label", (m * S,)), ("weight", (m * S,)),
                                                         ("origin", (m * S, 3)), ("time", (m * S,)))}

    def run(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    us = run(lambda: ray_sample(pts_s, origin, ds.sampler, seed=1, stream_id=0, out=out, depths=False))
    o = torch.tensor(origin, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    us_torch = run(lambda: synth.sample_rays(pts_s, o, ds.config, gen))
    written = m * S * (12 + 4 + 4 + 12 + 4)
    read = m * 12
    return dict(rays=m, samples=m * S, us_per_call_back_to_back=us, bytes_written=written, bytes_read=read,
                write_rate_TB_s=written / (us * 1e-6) / 1e12, share_of_hbm_peak_8TB_s=written / (us * 1e-6) / HBM_PEAK,
                share_of_achievable_copy_6p3TB_s=written / (us * 1e-6) / HBM_COPY,
                note="back-to-back launches of one frame's size: the call time includes the launch overhead and the outputs "
                     "(%.1f MB) stay in the Infinity Cache, so this is a call rate, not an HBM measurement; the kernel's own time "
                     "is in profiles/frame_kernel_stats.txt" % (written / 1e6),
                torch_sample_rays_us_per_call=us_torch, torch_sample_rays_outputs="coord, sdf_label, weight only (20 B / sample)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "frame_bench.json"))
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="one short drive per mode, no file written (the profiler's run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_bench.py measures on the GPU only")
    from shine_mapping_amd import FeatureOctree, synth
    from shine_mapping_amd.dataset import LiDARDataset

    frames, reps = (5, 1) if args.quick else (args.frames, args.reps)
    folder = tempfile.mkdtemp(prefix="frame_bench_")
    drive = synth.write_kitti_drive(folder, synth.make_config("ncd"), frames=frames, beams=64, azimuths=450, device="cuda")
    result = dict(scan="64 x 450 beams, ncd preset (config 4)", frames=frames, reps=reps, warm_frames_skipped=2)
    for mode, incremental in (("incremental", True), ("batch_window_replay", False)):
        for with_octree in (False, True):
            ours, theirs = [], []
            for rep in range(reps):
                cfg = synth.dataset_config("ncd", drive, window_replay_on=not incremental, window_radius=50.0)
                torch.manual_seed(rep)
                ds = LiDARDataset(cfg, FeatureOctree(cfg) if with_octree else None)
                base = TorchFrontEnd(cfg, LiDARDataset(cfg), FeatureOctree(cfg) if with_octree else None)
                for f in range(frames):  # interleaved: the same frame on both sides in turn
                    t_ours, _ = sync_time(lambda: ds.process_frame(f, incremental))
                    t_base, _ = sync_time(lambda: base.process_frame(f, incremental))
                    if f >= 2:
                        ours.append(t_ours)
                        theirs.append(t_base)
                base_pool = int(base.pools[0].shape[0])  # (other random samples: the window keeps a slightly different number)
            key = "%s_%s" % (mode, "with_octree" if with_octree else "front_end")
            result[key] = dict(device_ms_per_frame=float(np.median(ours)), torch_composite_ms_per_frame=float(np.median(theirs)),
                               device_min_max=[float(min(ours)), float(max(ours))],
                               torch_min_max=[float(min(theirs)), float(max(theirs))], frames_counted=len(ours),
                               pool_samples_at_end=len(ds), torch_pool_samples_at_end=base_pool)
            print(key, json.dumps(result[key]), flush=True)
    cfg = synth.dataset_config("ncd", drive)
    ds = LiDARDataset(cfg)
    stage_split(cfg, ds, 0)  # warm
    split, pts_s, origin = stage_split(cfg, ds, min(3, frames - 1))
    result["stage_split_one_frame"] = split
    result["shine_ray_sample"] = sampler_alone(pts_s, origin, ds, reps=20 if args.quick else 200)
    print(json.dumps(result["stage_split_one_frame"]), flush=True)
    print(json.dumps(result["shine_ray_sample"]), flush=True)
    if not args.quick:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
