"""RGB-D input: depth images + intrinsics + camera poses in, points out — on the device, without open3d.

    from shine_mapping_amd.rgbd import RGBDDataset
    dataset = RGBDDataset(config, octree)            # LiDARDataset's attributes and methods; config.depth_path instead of pc_path
    for frame_id in ...:
        dataset.process_frame(frame_id, incremental_on=False)

replaces the reference's detour dataset/rgbd_to_kitti_format.py (open3d back-projects every depth image and writes one .ply per
frame, which dataset/lidar_dataset.py reads back): a frame runs
    read (.npy / 16-bit .png) -> one upload -> shine_depth_unproject (back-projection, camera-to-sensor matrix, z / range / crop
    box; ONE launch, fp64, compacted in pixel order) -> LiDARDataset's down-sampling and everything behind it, unchanged
(csrc/shine_frame.hip).  The rules of the back-projection are those of include/shine_hip.h; they restate
open3d's RGBDImage.create_from_color_and_depth + PointCloud.create_from_rgbd_image as the converter calls them (:78-81).

The converter itself is here too, for the reference's workflow and as an exact cross-check of the direct route:
    python -m shine_mapping_amd.rgbd --depth_img_folder D --pose_file P --output_root OUT [--intrinsic_file F]
        [--is_focal_file B] [--already_kitti_format_pose B] [--max_depth_m 5.0] [--rgb_img_folder C]
writes OUT/rgbd_ply/%06d.ply (binary, double x y z [+ uchar red green blue]) and OUT/poses.txt (KITTI format): a folder the
existing LiDARDataset reads (calib_path = "").  Colour is not read by RGBDDataset: nothing in the training path reads it.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from .dataset import LiDARDataset, _rows_to_pose, csv_odom_to_transforms, natural_key

FLIP = np.diag([1.0, -1.0, -1.0, 1.0])  # the converter's extrinsic for PrimeSense / Neural-RGBD frames (:42,55)
FILTER_OFF = (-np.inf, np.inf, 0.0, np.inf)  # min_z, max_z, min_range, pc_radius that keep every valid pixel


class Intrinsics:
    """a pinhole camera: image size, focal lengths, principal point, raw depth units per metre, and the converter's `extrinsic`
    (open3d applies its INVERSE to the back-projected points: cam_to_sensor)"""

    def __init__(self, width, height, fx, fy, cx, cy, depth_scale=1000.0, extrinsic=None):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.depth_scale = float(depth_scale)
        self.extrinsic = np.eye(4) if extrinsic is None else np.asarray(extrinsic, dtype=np.float64).reshape(4, 4).copy()

    @property
    def cam_to_sensor(self):
        return np.linalg.inv(self.extrinsic)

    def __repr__(self):
        return "Intrinsics(%d x %d, fx %r, fy %r, cx %r, cy %r, scale %r, flip %s)" % (
            self.width, self.height, self.fx, self.fy, self.cx, self.cy, self.depth_scale, bool(self.extrinsic[1, 1] < 0))


def read_intrinsics(path="", is_focal_file=True, image_size=None):
    """the converter's three cases (dataset/rgbd_to_kitti_format.py:33-67).  path == "": the PrimeSense default (640 x 480,
    fx = fy = 525, cx = 319.5, cy = 239.5, scale 1000, flip).  is_focal_file: a text file whose first line is one focal length
    (Neural-RGBD): cx = (W - 1) / 2, cy = (H - 1) / 2 from image_size = (W, H), scale 1000, flip.  Otherwise a JSON
    {"camera": {w, h, fx, fy, cx, cy, scale}} (Replica): no flip."""
    if path == "":
        return Intrinsics(640, 480, 525.0, 525.0, 319.5, 239.5, 1000.0, FLIP)
    if is_focal_file:
        if image_size is None:
            raise ValueError("read_intrinsics: %s holds a focal length only; image_size = (width, height) is needed" % path)
        with open(path) as fh:
            line = fh.readline()
        try:
            focal = float(line)
        except ValueError:
            raise ValueError("%s: the first line is not a focal length (%r); is it a JSON file (is_focal_file = False)?"
                             % (path, line.strip()[:40])) from None
        w, h = int(image_size[0]), int(image_size[1])
        return Intrinsics(w, h, focal, focal, (w - 1.0) / 2.0, (h - 1.0) / 2.0, 1000.0, FLIP)
    with open(path) as fh:
        try:
            cam = json.load(fh)["camera"]
        except (ValueError, KeyError, TypeError) as e:
            raise ValueError("%s: not a JSON file with a \"camera\" entry (%s); is it a focal-length file (is_focal_file = True)?"
                             % (path, e)) from None
    missing = [k for k in ("w", "h", "fx", "fy", "cx", "cy", "scale") if k not in cam]
    if missing:
        raise ValueError("%s: the camera entry lacks %s" % (path, ", ".join(missing)))
    return Intrinsics(cam["w"], cam["h"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["scale"], np.eye(4))


def read_depth(path):
    """one depth frame on the host: [H,W] uint16 (raw units) or float32.  .npy (uint16 / float32) or 16-bit .png (through PIL,
    imported here)"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        img = np.load(path)
        if img.ndim != 2 or img.dtype not in (np.uint16, np.float32):
            raise ValueError("%s: a depth frame must be a [H,W] uint16 or float32 array, got %s %s" % (path, img.shape, img.dtype))
        return np.ascontiguousarray(img)
    if ext == ".png":
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("%s: reading a .png depth frame needs PIL, which cannot be imported (%s); store the frames as .npy "
                              "(uint16 or float32 [H,W]) instead" % (path, e)) from None
        with Image.open(path) as im:
            img = np.array(im)
        if img.ndim != 2 or img.dtype.kind not in "ui" or img.min() < 0 or img.max() > 65535:
            raise ValueError("%s: a .png depth frame must be a single-channel 16-bit image, got %s %s" % (path, img.shape, img.dtype))
        return np.ascontiguousarray(img.astype(np.uint16))
    raise ValueError("%s: unknown depth frame format %r (read: .png, 16-bit, and .npy, uint16 or float32)" % (path, ext))


def read_poses(path, kitti_format=False):
    """camera poses in the world frame, a list of [4,4] float64.  kitti_format: 12 values per line (rows 0-2); otherwise the text of
    Neural-RGBD, four lines of four values per matrix (dataset/rgbd_to_kitti_format.py:123-139); *.csv as LiDARDataset reads it"""
    if path.endswith("csv"):
        return csv_odom_to_transforms(path)
    with open(path) as fh:
        rows = [[float(v) for v in line.split()] for line in fh if line.strip()]
    if kitti_format:
        bad = [k for k, r in enumerate(rows) if len(r) != 12]
        if bad:
            raise ValueError("%s: line %d holds %d values, a KITTI pose line holds 12 (pose_kitti_format = False reads 4-line "
                             "matrices)" % (path, bad[0] + 1, len(rows[bad[0]])))
        return [_rows_to_pose(r) for r in rows]
    if len(rows) % 4 or any(len(r) != 4 for r in rows):
        raise ValueError("%s: expected four lines of four values per pose (%d non-empty lines; pose_kitti_format = True reads "
                         "12-value lines)" % (path, len(rows)))
    return [np.array(rows[k:k + 4], dtype=np.float64) for k in range(0, len(rows), 4)]


def write_poses_kitti(path, poses):
    """KITTI pose lines that read back bit for bit (repr of every float)"""
    with open(path, "w") as fh:
        for P in poses:
            fh.write(" ".join(repr(float(v)) for v in np.asarray(P, dtype=np.float64)[:3].reshape(-1)) + "\n")


def _device_image(depth, device):
    """-> (2-D device tensor whose rows are contiguous, is_float32)"""
    if isinstance(depth, np.ndarray):
        if depth.ndim != 2 or depth.dtype not in (np.uint16, np.float32):
            raise ValueError("unproject_depth: depth must be [H,W] uint16 or float32, got %s %s" % (depth.shape, depth.dtype))
        host = np.ascontiguousarray(depth)
        depth = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(device)  # (one upload)
    sixteen = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ())
    if depth.dim() != 2 or depth.dtype not in sixteen + (torch.float32,):
        raise ValueError("unproject_depth: depth must be [H,W] uint16 (or its int16 bit pattern) or float32, got %s %s"
                         % (tuple(depth.shape), depth.dtype))
    if not depth.is_cuda:
        raise _lib.ShineHipError("unproject_depth runs on the device only (there is no CPU path)")
    if depth.numel() and (depth.stride(1) != 1 or depth.stride(0) < depth.shape[1]):
        depth = depth.contiguous()
    return depth, depth.dtype == torch.float32


def unproject_depth(depth, intrinsics, cam_to_sensor=None, max_depth_m=5.0, filter=None, return_index=False, device="cuda"):
    """shine_depth_unproject: one depth image -> the points of its valid pixels, fp64 [n,3] on the device in ascending pixel index
    (the rules: include/shine_hip.h).  depth: [H,W] numpy array (uploaded once) or device tensor, uint16 or float32; a device
    tensor may be a view with a row stride (columns contiguous) and any base offset.  cam_to_sensor: the 4x4 applied to the
    back-projected points; None = the intrinsics' own (the inverse of the converter's extrinsic: the y / z flip, or the identity).
    filter: None (every valid pixel) or (min_z, max_z, min_range, pc_radius) — shine_frame_filter's test.  return_index: also the
    int32 pixel indices v * width + u of the points."""
    img, is_f32 = _device_image(depth, device)
    h, w = int(img.shape[0]), int(img.shape[1])
    if (w, h) != (intrinsics.width, intrinsics.height):
        raise ValueError("unproject_depth: the image is %d x %d, the intrinsics are for %d x %d" % (w, h, intrinsics.width, intrinsics.height))
    M = np.ascontiguousarray(intrinsics.cam_to_sensor if cam_to_sensor is None else np.asarray(cam_to_sensor, dtype=np.float64))
    if M.shape != (4, 4):
        raise ValueError("unproject_depth: cam_to_sensor must be 4 x 4")
    m16 = (C.c_double * 16)(*[float(v) for v in M.reshape(-1)])
    min_z, max_z, min_range, pc_radius = FILTER_OFF if filter is None else [float(v) for v in filter]
    n = w * h
    pts = torch.empty((n, 3), dtype=torch.float64, device=img.device)
    idx = torch.empty((n,), dtype=torch.int32, device=img.device) if return_index else None
    if n == 0:
        return (pts, idx) if return_index else pts
    pitch = int(img.stride(0)) if h > 1 else w
    kept = C.c_int64(0)
    _lib.call_with_workspace(
        _lib.lib().shine_depth_unproject, img.device, img.data_ptr(), int(is_f32), w, h, pitch, intrinsics.fx, intrinsics.fy,
        intrinsics.cx, intrinsics.cy, intrinsics.depth_scale, float(max_depth_m), m16, min_z, max_z, min_range, pc_radius,
        _lib.WS, _lib.WS_BYTES, pts.data_ptr(), idx.data_ptr() if return_index else None, C.byref(kept),
        _lib.current_stream_handle())
    k = int(kept.value)
    return (pts[:k], idx[:k]) if return_index else pts[:k]


class RGBDDataset(LiDARDataset):
    """LiDARDataset whose frames are depth images.  Reads, next to LiDARDataset's fields (pc_path and calib_path are not used):
    depth_path, intrinsic_path (""), is_focal_file (True), pose_path, pose_kitti_format (False), max_depth_m (5.0) — the cases and
    defaults of dataset/rgbd_to_kitti_format.py:33-67,161-167."""

    def _reads_labels(self, config):
        return False  # (depth frames carry no label files: semantic_on stays refused)

    def _read_poses(self, config):
        self.calib = {"Tr": np.eye(4)}
        return read_poses(config.pose_path, bool(getattr(config, "pose_kitti_format", False)))

    def _list_frames(self, config):
        names = sorted(os.listdir(config.depth_path), key=natural_key)
        self.max_depth_m = float(getattr(config, "max_depth_m", 5.0))
        path, focal = getattr(config, "intrinsic_path", ""), bool(getattr(config, "is_focal_file", True))
        size = None
        if path != "" and focal:  # (the converter's "example image": the first frame gives the size the principal point is set from)
            if not names:
                raise ValueError("%s holds no depth frame to take the image size from" % config.depth_path)
            first = read_depth(os.path.join(config.depth_path, names[0]))
            size = (first.shape[1], first.shape[0])
        self.intrinsics = read_intrinsics(path, focal, size)
        return names

    def read_depth_frame(self, frame_id):
        path = os.path.join(self.config.depth_path, self.pc_filenames[frame_id])
        depth = read_depth(path)
        k = self.intrinsics
        if depth.shape != (k.height, k.width):
            raise ValueError("%s: the frame is %d x %d, the intrinsics (%s) are for %d x %d" % (
                path, depth.shape[1], depth.shape[0], self.config.intrinsic_path or "PrimeSense default", k.width, k.height))
        return depth

    def frame_points(self, frame_id):
        """stages 1-3 of process_frame: read, one upload, shine_depth_unproject with the config's filter, down-sampling"""
        cfg = self.config
        pts = unproject_depth(self.read_depth_frame(frame_id), self.intrinsics, max_depth_m=self.max_depth_m,
                              filter=(cfg.min_z, cfg.max_z, cfg.min_range, cfg.pc_radius), device=self.device)
        return self._down_sample(pts, frame_id)


# ---- the converter (dataset/rgbd_to_kitti_format.py without open3d) --------------------------------------------------------------
def _str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    import argparse

    raise argparse.ArgumentTypeError("Boolean value expected.")


def rgbd_to_kitti_format(depth_img_folder, pose_file, output_root, intrinsic_file="", is_focal_file=True,
                         already_kitti_format_pose=False, max_depth_m=5.0, rgb_img_folder=None, device="cuda"):
    """every depth frame -> output_root/rgbd_ply/%06d.ply (every valid pixel, no range or box filter), the poses ->
    output_root/poses.txt.  -> the number of frames written"""
    from .mesher import write_ply

    ply_path = os.path.join(output_root, "rgbd_ply")
    os.makedirs(ply_path, exist_ok=True)
    write_poses_kitti(os.path.join(output_root, "poses.txt"), read_poses(pose_file, already_kitti_format_pose))
    depth_files = sorted(os.listdir(depth_img_folder), key=natural_key)
    if not depth_files:
        raise ValueError("%s holds no depth frame" % depth_img_folder)
    rgb_files, Image = None, None
    if rgb_img_folder:
        try:
            from PIL import Image
        except ImportError as e:
            print("PIL cannot be imported (%s): the clouds are written without colour" % e)
        else:
            rgb_files = sorted(os.listdir(rgb_img_folder), key=natural_key)
            if len(rgb_files) != len(depth_files):
                raise ValueError("%s holds %d images, %s %d depth frames" % (rgb_img_folder, len(rgb_files), depth_img_folder, len(depth_files)))
    first = read_depth(os.path.join(depth_img_folder, depth_files[0]))
    print("Image size:", first.shape[0], "x", first.shape[1])
    k = read_intrinsics(intrinsic_file, is_focal_file, (first.shape[1], first.shape[0]))
    for frame, name in enumerate(depth_files):
        path = os.path.join(depth_img_folder, name)
        depth = read_depth(path)
        if depth.shape != (k.height, k.width):
            raise ValueError("%s: the frame is %d x %d, the intrinsics (%s) are for %d x %d" % (
                path, depth.shape[1], depth.shape[0], intrinsic_file or "PrimeSense default", k.width, k.height))
        pts, idx = unproject_depth(depth, k, max_depth_m=max_depth_m, return_index=True, device=device)
        pts = pts.cpu().numpy()
        props = [("x", pts[:, 0], "double"), ("y", pts[:, 1], "double"), ("z", pts[:, 2], "double")]
        if rgb_files is not None:
            cpath = os.path.join(rgb_img_folder, rgb_files[frame])
            with Image.open(cpath) as im:
                rgb = np.array(im.convert("RGB"))
            if rgb.shape[:2] != depth.shape:
                raise ValueError("%s is %d x %d, its depth frame %s %d x %d" % (cpath, rgb.shape[1], rgb.shape[0], path,
                                                                               depth.shape[1], depth.shape[0]))
            rgb = rgb.reshape(-1, 3)[idx.cpu().numpy()]
            props += [("red", rgb[:, 0], "uchar"), ("green", rgb[:, 1], "uchar"), ("blue", rgb[:, 2], "uchar")]
        write_ply(os.path.join(ply_path, "%06d.ply" % frame), props)
    print("The rgbd dataset in KITTI format has been saved at %s" % output_root)
    return len(depth_files)


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m shine_mapping_amd.rgbd",
                                 description="depth images + poses -> a KITTI-format folder (rgbd_ply/*.ply, poses.txt)")
    ap.add_argument("--depth_img_folder", required=True, help="folder of depth frames (.png 16-bit, or .npy uint16 / float32)")
    ap.add_argument("--rgb_img_folder", default=None, help="folder of colour images (optional; needs PIL)")
    ap.add_argument("--intrinsic_file", default="", help="focal-length text file or camera JSON; empty: PrimeSense default")
    ap.add_argument("--pose_file", required=True, help="camera pose of every frame")
    ap.add_argument("--output_root", required=True, help="folder the KITTI-format data is written to")
    ap.add_argument("--max_depth_m", type=float, default=5.0, help="depths at or beyond this are dropped")
    ap.add_argument("--is_focal_file", type=_str2bool, nargs="?", default=True,
                    help="the intrinsic file holds one focal length (Neural-RGBD), not a camera JSON (Replica)")
    ap.add_argument("--already_kitti_format_pose", type=_str2bool, nargs="?", default=False,
                    help="the pose file holds 12-value KITTI lines (Replica), not 4-line matrices (Neural-RGBD)")
    a = ap.parse_args(argv)
    rgbd_to_kitti_format(a.depth_img_folder, a.pose_file, a.output_root, a.intrinsic_file, a.is_focal_file,
                         a.already_kitti_format_pose, a.max_depth_m, a.rgb_img_folder)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
