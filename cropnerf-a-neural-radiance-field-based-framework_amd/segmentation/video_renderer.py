"""Views of a (labelled) point cloud without a window -- counterpart of the reference's two viewers, which go through an
open3d window: the orbit video of ``crop_nerf/evaluation/generate_video.py:17-117`` and the saved camera trajectory of
``crop_nerf/segmentation/video_renderer.py``.  Frames are drawn by ``ops.splat_points`` (``csrc/splat.hip``) and written
as PNG files; no video container is written (encode ``frame_%05d.png`` elsewhere).

    python -m cropnerf_amd.segmentation.video_renderer orbit --pcd X.ply [--cluster-info all_super_cluster_info_nsub_2.npy]
        --output-dir D [--num-frames 180 --radius 1.0 --height 0.7 --tilt-deg 10 --width 1920 --height-px 1080 --point-size 2]
    python -m cropnerf_amd.segmentation.video_renderer path --pcd X.ply --camera-json J --output-dir D
"""

from __future__ import annotations

import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import result_cloud

FRAME_PATTERN = "frame_%05d.png"
CONTEXT_GREY = 155  # generate_video.py:42
CONTEXT_VOXEL = 5 * 10e-4  # sic (:40): 5 mm


def default_intrinsics(width: int = 1920, height: int = 1080, fov_deg: float = 60.0) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) of the orbit: vertical field of view ``fov_deg``, square pixels, principal point at the centre of
    the pixel grid (pixel centres sit at integer coordinates)."""
    f = (height / 2.0) / np.tan(np.radians(fov_deg) / 2.0)
    return float(f), float(f), (width - 1) / 2.0, (height - 1) / 2.0


def orbit_cameras(center, num_frames: int = 180, radius: float = 1.0, height: float = 0.7, tilt_deg: float = 10.0) -> np.ndarray:
    """World-to-camera matrices [num_frames,4,4] (float64) of the reference's orbit (``generate_video.py:61-99``): the camera
    sits on a circle of ``radius`` in the xy-plane, ``height`` above ``center``, and looks at the point ``tan(tilt) *
    radius`` below the centre.  ``right = forward x (0, 0, -1)``, ``up = right x forward``; the camera-to-world rotation has
    the columns ``[right, up, forward]`` and its inverse is the extrinsic.  That frame is LEFT-handed (determinant -1): it is
    kept as the reference builds it -- the renderer only applies the matrix, so the frames show what the reference's call
    shows (camera y, drawn downwards, points towards world -z)."""
    center = np.asarray(center, dtype=np.float64).reshape(3)
    target = center - np.array([0.0, 0.0, np.tan(np.radians(tilt_deg)) * radius])
    out = np.zeros((num_frames, 4, 4))
    for i in range(num_frames):
        angle = 2.0 * np.pi * i / num_frames
        cam_pos = center + np.array([radius * np.cos(angle), radius * np.sin(angle), height])
        forward = target - cam_pos
        forward /= np.linalg.norm(forward)
        right = np.cross(forward, np.array([0.0, 0.0, -1.0]))
        right /= np.linalg.norm(right)
        up = np.cross(right, forward)
        up /= np.linalg.norm(up)
        c2w = np.eye(4)
        c2w[:3, :3] = np.stack([right, up, forward], axis=1)
        c2w[:3, 3] = cam_pos
        out[i] = np.linalg.inv(c2w)
    return out


def pack_cameras(extrinsics: np.ndarray, intrinsics) -> np.ndarray:
    """[F,4,4] world-to-camera + (fx, fy, cx, cy) (one tuple, or [F,4]) -> the [F,16] float32 rows ``ops.splat_points``
    takes: the 3x4 row-major, then fx, fy, cx, cy."""
    ext = np.asarray(extrinsics, dtype=np.float64).reshape(-1, 4, 4)
    intr = np.broadcast_to(np.asarray(intrinsics, dtype=np.float64).reshape(-1, 4), (len(ext), 4))
    return np.concatenate([ext[:, :3, :].reshape(len(ext), 12), intr], axis=1).astype(np.float32)


def load_camera_trajectory(path) -> Dict[str, object]:
    """open3d's ``PinholeCameraTrajectory`` JSON: ``parameters[i].extrinsic`` is 16 values, COLUMN-major;
    ``parameters[i].intrinsic`` holds ``{width, height, intrinsic_matrix}`` with ``intrinsic_matrix`` 9 values, column-major.
    Returns ``{"extrinsics" [F,4,4], "intrinsics" [F,4] (fx, fy, cx, cy), "width", "height"}`` (size of the first camera;
    a trajectory whose cameras differ in size is refused)."""
    with open(path) as f:
        doc = json.load(f)
    params = doc["parameters"]
    if not params:
        raise ValueError(f"{path}: the trajectory holds no camera")
    ext, intr, sizes = [], [], set()
    for p in params:
        ext.append(np.asarray(p["extrinsic"], dtype=np.float64).reshape(4, 4).T)
        k = np.asarray(p["intrinsic"]["intrinsic_matrix"], dtype=np.float64).reshape(3, 3).T
        intr.append([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
        sizes.add((int(p["intrinsic"]["width"]), int(p["intrinsic"]["height"])))
    if len(sizes) != 1:
        raise ValueError(f"{path}: cameras of different sizes {sorted(sizes)}")
    (width, height), = sizes
    return {"extrinsics": np.stack(ext), "intrinsics": np.asarray(intr), "width": width, "height": height}


def _save_png(path: str, frame: np.ndarray) -> None:
    from PIL import Image

    Image.fromarray(frame).save(path)


def pointcloud_to_frames(points, colors=None, labels=None, full_tree=None, output_dir: str = "frames", point_size: int = 2,
                         background: Sequence[int] = (255, 255, 255), cameras: Optional[np.ndarray] = None,
                         width: int = 1920, height: int = 1080, num_frames: int = 180, radius: float = 1.0,
                         orbit_height: float = 0.7, tilt_deg: float = 10.0, normalise: bool = False,
                         near_plane: float = 1e-3, frames_per_chunk: int = 8, workers: int = 4, device="cuda") -> List[str]:
    """``pointcloud_to_video`` (``generate_video.py:17-117``) as PNG frames: ``points`` [N,3] drawn with ``colors`` (uint8
    [N,3], or floats in [0,1]), or with ``label_colors(labels, normalise)`` when ``labels`` are given, grey when neither is.
    ``full_tree`` ([M,3] points) adds a grey cloud as context, voxel-down-sampled at 5 * 10e-4 as the reference's viewers
    do.  ``cameras`` [F,16] (``pack_cameras``) selects the views; without it, the reference's orbit around the mean of
    ``points`` with ``default_intrinsics(width, height)``.  Frames are written to ``output_dir/frame_%05d.png`` on a few
    worker threads while the next chunk renders; returns the paths."""
    import torch

    from .. import ops

    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if labels is not None:
        cols = result_cloud.label_colors(labels, normalise)
    elif colors is None:
        cols = np.full((len(pts), 3), CONTEXT_GREY, dtype=np.uint8)
    else:
        cols = np.asarray(colors)
        if cols.dtype != np.uint8:
            cols = np.floor(np.clip(cols.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
    if cols.shape != pts.shape:
        raise ValueError(f"pointcloud_to_frames: {cols.shape} colours for {pts.shape} points")
    if cameras is None:
        center = pts.mean(axis=0) if len(pts) else np.zeros(3)  # open3d get_center
        cameras = pack_cameras(orbit_cameras(center, num_frames, radius, orbit_height, tilt_deg),
                               default_intrinsics(width, height))
    cams = torch.as_tensor(np.ascontiguousarray(cameras, dtype=np.float32)).reshape(-1, 16).to(device)
    d_pts = torch.as_tensor(pts, dtype=torch.float32).to(device).contiguous()
    d_cols = torch.as_tensor(np.ascontiguousarray(cols)).to(device)
    if full_tree is not None and len(full_tree):
        tree = torch.as_tensor(np.asarray(full_tree, dtype=np.float32).reshape(-1, 3)).to(device).contiguous()
        tree, _ = ops.voxel_down_sample(tree, CONTEXT_VOXEL)
        d_pts = torch.cat([d_pts, tree]).contiguous()
        d_cols = torch.cat([d_cols, torch.full((tree.shape[0], 3), CONTEXT_GREY, dtype=torch.uint8, device=device)]).contiguous()
    os.makedirs(output_dir, exist_ok=True)
    paths, jobs = [], []
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        for f0 in range(0, cams.shape[0], max(1, frames_per_chunk)):
            chunk = cams[f0:f0 + max(1, frames_per_chunk)].contiguous()
            frames = ops.splat_points(d_pts, d_cols, chunk, height, width, point_size, near_plane, background).cpu().numpy()
            for k in range(frames.shape[0]):
                paths.append(os.path.join(output_dir, FRAME_PATTERN % (f0 + k)))
                jobs.append(pool.submit(_save_png, paths[-1], frames[k]))
        for j in jobs:
            j.result()
    print(f"{len(paths)} frames: {os.path.join(output_dir, FRAME_PATTERN)}")
    return paths


def _load_cloud(a):
    """The CLI's cloud: (points, colours or None, labels or None, context points or None)."""
    from ..fruit_nerf.ply import read_ply

    pts, cols = read_ply(a.pcd)
    if cols is not None:
        cols = np.rint(cols * 255.0).astype(np.uint8)  # the file's own bytes back
    if getattr(a, "cluster_info", None):
        # view_super_clusters: the clusters coloured by super-cluster index + 1, the .ply as grey context
        pcd_data = np.load(a.cluster_info, allow_pickle=True)
        p, l = result_cloud.super_cluster_labels(pcd_data)
        return p, None, l, pts
    return pts, cols, None, None


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)
    orbit = sub.add_parser("orbit", help="the reference's orbit around the cloud's centre")
    orbit.add_argument("--pcd", required=True)
    orbit.add_argument("--cluster-info", default=None, help="all_super_cluster_info*.npy: colour by super-cluster")
    orbit.add_argument("--output-dir", required=True)
    orbit.add_argument("--num-frames", type=int, default=180)
    orbit.add_argument("--radius", type=float, default=1.0)
    orbit.add_argument("--height", type=float, default=0.7)
    orbit.add_argument("--tilt-deg", type=float, default=10.0)
    orbit.add_argument("--width", type=int, default=1920)
    orbit.add_argument("--height-px", type=int, default=1080)
    orbit.add_argument("--point-size", type=int, default=2)
    path = sub.add_parser("path", help="a saved open3d PinholeCameraTrajectory")
    path.add_argument("--pcd", required=True)
    path.add_argument("--camera-json", required=True)
    path.add_argument("--output-dir", required=True)
    path.add_argument("--point-size", type=int, default=2)
    a = ap.parse_args(argv)
    pts, cols, labels, context = _load_cloud(a)
    if a.command == "orbit":
        paths = pointcloud_to_frames(pts, cols, labels, context, a.output_dir, a.point_size, width=a.width, height=a.height_px,
                                     num_frames=a.num_frames, radius=a.radius, orbit_height=a.height, tilt_deg=a.tilt_deg)
    else:
        traj = load_camera_trajectory(a.camera_json)
        paths = pointcloud_to_frames(pts, cols, labels, context, a.output_dir, a.point_size,
                                     cameras=pack_cameras(traj["extrinsics"], traj["intrinsics"]), width=traj["width"],
                                     height=traj["height"])
    return 0 if paths else 1


if __name__ == "__main__":
    raise SystemExit(main())
