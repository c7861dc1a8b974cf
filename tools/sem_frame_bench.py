"""Semantic frame front-end measurements: LiDARDataset.process_frame with semantic_on on the 64 x 450-beam
labelled synthetic scan (the `ncd` preset), per frame, against
  * the non-semantic front-end on the same scans (what the labels cost), and
  * the host route for the stages read -> filter -> voxel labels — tests/sem_frame_oracle.py's numpy plus the upload of the points and
    classes — which is what a user had before: the device took per-ray labels, but nothing produced them from a scan.

    python tools/sem_frame_bench.py [--out profiles/sem_frame_bench.json] [--frames 12] [--reps 3]
    python tools/sem_frame_bench.py --plain-only [--root <another checkout>]     # the non-semantic frame alone, e.g. on the parent commit

tools/frame_bench.py's method: host clocks around work that ends in a device synchronise, warm (the first two frames of a drive are
not counted), median over the counted frames of `reps` drives, the sides interleaved frame by frame.  No octree: the front-end alone.
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


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_route(so, fo, cfg, ds, frame_id):
    """read -> filter + crop -> voxel classes in numpy, then the upload: the points and classes shine_ray_sample takes"""
    name = ds.pc_filenames[frame_id]
    raw = fo.read_kitti_bin(os.path.join(cfg.pc_path, name)).astype(np.float64)
    words = so.read_labels(os.path.join(cfg.label_path, name.replace("bin", "label")))
    kept, cls = so.sem_filter(raw, words, ds.label_map.lut, cfg.min_z, cfg.filter_moving_object, bool(cfg.min_range), cfg.min_z,
                              cfg.max_z, cfg.pc_radius)
    sensor, _, classes = so.voxel_classes(raw[kept], cls, cfg.vox_down_m)
    return torch.from_numpy(sensor).cuda(), torch.from_numpy(classes).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sem_frame_bench.json"))
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true", help="time the non-semantic front-end alone and print it (no file written)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose shine_mapping_amd is measured (with --plain-only: any commit)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sem_frame_bench.py measures on the GPU only")
    sys.path.insert(0, os.path.abspath(args.root))
    from shine_mapping_amd import synth
    from shine_mapping_amd.dataset import LiDARDataset

    frames, reps = args.frames, args.reps
    folder = tempfile.mkdtemp(prefix="sem_frame_bench_")
    result = dict(scan="64 x 450 beams, ncd preset, labelled", frames=frames, reps=reps, warm_frames_skipped=2)
    if args.plain_only:
        drive = synth.write_kitti_drive(folder, synth.make_config("ncd"), frames=frames, beams=64, azimuths=450, device="cuda")
        for mode, incremental in (("incremental", True), ("batch_window_replay", False)):
            plain = []
            for rep in range(reps):
                ds = LiDARDataset(synth.dataset_config("ncd", drive, window_replay_on=not incremental, window_radius=50.0))
                for f in range(frames):
                    t, _ = sync_time(lambda: ds.process_frame(f, incremental))
                    if f >= 2:
                        plain.append(t)
            result[mode + "_front_end"] = dict(plain_ms_per_frame=float(np.median(plain)), plain_min_max=[float(min(plain)), float(max(plain))],
                                               frames_counted=len(plain))
        print(json.dumps(result), flush=True)
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frame_oracle as fo
    import sem_frame_oracle as so

    drive = synth.write_kitti_drive(folder, synth.make_config("ncd"), frames=frames, beams=64, azimuths=450, device="cuda", labels=True)
    for mode, incremental in (("incremental", True), ("batch_window_replay", False)):
        sem_t, plain_t = [], []
        for rep in range(reps):
            over = dict(window_replay_on=not incremental, window_radius=50.0)
            sem = LiDARDataset(synth.dataset_config("ncd", drive, semantic_on=True, **over))
            plain = LiDARDataset(synth.dataset_config("ncd", drive, **over))
            for f in range(frames):  # interleaved: the same frame on both sides in turn
                t_sem, _ = sync_time(lambda: sem.process_frame(f, incremental))
                t_plain, _ = sync_time(lambda: plain.process_frame(f, incremental))
                if f >= 2:
                    sem_t.append(t_sem)
                    plain_t.append(t_plain)
        result[mode + "_front_end"] = dict(
            semantic_ms_per_frame=float(np.median(sem_t)), plain_ms_per_frame=float(np.median(plain_t)),
            semantic_min_max=[float(min(sem_t)), float(max(sem_t))], plain_min_max=[float(min(plain_t)), float(max(plain_t))],
            frames_counted=len(sem_t), pool_samples_at_end=len(sem), plain_pool_samples_at_end=len(plain))
        print(mode, json.dumps(result[mode + "_front_end"]), flush=True)
    # stages read -> filter -> voxel labels: the device against the host route, frame by frame in turn
    cfg = synth.dataset_config("ncd", drive, semantic_on=True)
    ds = LiDARDataset(cfg)
    dev_t, host_t = [], []
    for f in range(frames):
        t_dev, (pts, classes) = sync_time(lambda: ds.sem_frame_points(f))
        t_host, (hp, hc) = sync_time(lambda: host_route(so, fo, cfg, ds, f))
        assert torch.equal(classes, hc) and pts.shape == hp.shape  # (both routes label the same voxels)
        if f >= 2:
            dev_t.append(t_dev)
            host_t.append(t_host)
    result["read_filter_voxel_labels"] = dict(device_ms_per_frame=float(np.median(dev_t)), host_numpy_plus_upload_ms_per_frame=float(np.median(host_t)),
                                              device_min_max=[float(min(dev_t)), float(max(dev_t))],
                                              host_min_max=[float(min(host_t)), float(max(host_t))], frames_counted=len(dev_t),
                                              points_after_down_sampling=int(pts.shape[0]))
    print(json.dumps(result["read_filter_voxel_labels"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
