"""Write tests/golden/sem_frame.pt: the reference's own LiDARDataset.preprocess_sem_kitti (dataset/lidar_dataset.py:341-362) on CPU, on
stored points and raw label words, plus its learning map as an int32 LUT and its colour table as an array.

    python tools/make_sem_frame_golden.py            # (re)write the fixture
    python tools/make_sem_frame_golden.py --check    # regenerate in memory, exit 1 unless it is bit-identical to the stored one

Needs the reference checkout (oracle/ref_import.py, read-only).  The method reads nothing of `self`, so it is called unbound.

The fixture holds recorded inputs and outputs only:
  lut      int32 [65536]: the reference's sem_kitti_learning_map, -1 where it has no entry
  colors   fp64 [21, 3]: sem_kitti_color_map / 255
  cases[i]: points [n,3] float32 (as a .bin file gives them; the reference is handed their fp64 values), labels [n] int32 (the
            bit patterns of the uint32 words: lower 16 bits an id of the reference's map, upper 16 a random instance id),
            min_range, filter_outlier, filter_moving, and the outputs points_out [k,3] (stored as float32 after checking that
            this loses nothing: the reference only selects rows) and classes [k] int32 — exact values
Cases: n = 1, 777, 2047, 2048, 2049, 3 * 2048 + 5 (a tile of shine_sem_frame_filter is 8 x 256 points) over filter_moving x
filter_outlier, with a min_range that cuts (2.5 m in a cloud of 0.5-30 m ranges) and, once, one that does not (-3.0: the value the
reference's positional call passes, config.min_z); one point of every multi-point case lies exactly at r == min_range (3-4-0
scaled), and ids 99, 252 (the map has no 100) and 1 are always present.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "sem_frame.pt")
CASES = (  # n, min_range, filter_outlier, filter_moving, seed
    (1, 2.5, True, True, 1),
    (2047, 2.5, True, True, 2),
    (2048, 2.5, False, True, 3),
    (2049, 2.5, True, False, 4),
    (3 * 2048 + 5, 2.5, False, False, 5),
    (777, 2.5, True, True, 6),
    (2049, -3.0, True, True, 7),
)


def _inputs(n, min_range, seed, ids):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * rng.uniform(0.5, 30.0, size=(n, 1))).astype(np.float32)
    raw = np.asarray(ids, np.int64)[rng.integers(0, len(ids), n)]
    if n >= 8:
        p[3] = [0.6 * abs(min_range), 0.8 * abs(min_range), 0.0]  # (|p| == |min_range| exactly: 1.5, 2.0 -> 2.5)
        raw[4], raw[5], raw[6] = 99, 252, 1
        p[4], p[5], p[6] = [10.0, 0.0, 0.0], [0.0, 10.0, 0.0], [0.0, 0.0, 10.0]
    words = (rng.integers(0, 1 << 16, n).astype(np.int64) << 16) | raw
    return p.astype(np.float64), words


def generate(preprocess, learning_map, color_map):
    lut = np.full(1 << 16, -1, np.int32)
    for k, v in learning_map.items():
        lut[int(k)] = int(v)
    colors = np.zeros((max(color_map) + 1, 3), np.float64)
    for k, v in color_map.items():
        colors[int(k)] = np.asarray(v, np.float64) / 255.0
    ids = sorted(int(k) for k in learning_map)
    cases = []
    for n, min_range, filter_outlier, filter_moving, seed in CASES:
        p, words = _inputs(n, min_range, seed, ids)
        pts, cls = preprocess(None, p.copy(), words.astype(np.uint32), min_range, filter_outlier, filter_moving)
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
        cases.append(dict(points=torch.from_numpy(p.astype(np.float32)),
                          labels=torch.from_numpy(words.astype(np.uint32).view(np.int32).copy()), min_range=float(min_range),
                          filter_outlier=bool(filter_outlier), filter_moving=bool(filter_moving),
                          points_out=torch.from_numpy(pts.astype(np.float32)),
                          classes=torch.from_numpy(np.asarray(cls, np.int64).reshape(-1).astype(np.int32))))
    return dict(lut=torch.from_numpy(lut), colors=torch.from_numpy(colors), cases=cases)


def identical(a, b):
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(identical(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(identical(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


def main():
    from oracle import ref_import

    ref_import.install()
    from dataset.lidar_dataset import LiDARDataset
    from utils.semantic_kitti_utils import sem_kitti_color_map, sem_kitti_learning_map

    fx = generate(LiDARDataset.preprocess_sem_kitti, sem_kitti_learning_map, sem_kitti_color_map)
    if "--check" in sys.argv:
        stored = torch.load(PATH, map_location="cpu", weights_only=False)
        ok = identical(fx, stored)
        print("identical" if ok else "DIFFERENT")
        sys.exit(0 if ok else 1)
    torch.save(fx, PATH)
    print("wrote", PATH, os.path.getsize(PATH), "bytes; kept", [int(c["classes"].numel()) for c in fx["cases"]])


if __name__ == "__main__":
    main()
