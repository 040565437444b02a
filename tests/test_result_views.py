"""The views of the merger's result: the labelled cloud (``segmentation/result_cloud.py``), the cameras and PNG frames of
``segmentation/video_renderer.py`` and ``merger.main --visualize``."""

import json
import os

import numpy as np
import pytest

from cropnerf_amd.segmentation import result_cloud as RC
from cropnerf_amd.segmentation import video_renderer as VR


# ------------------------------------------------------------------------------------------------------------------
# CPU tier
# ------------------------------------------------------------------------------------------------------------------

def test_orbit_cameras_frame_zero_closed_form_and_every_frame_looks_at_the_target():
    c = np.array([0.1, -0.2, 0.3])
    ext = VR.orbit_cameras(c)
    assert ext.shape == (180, 4, 4)
    # frame 0 by hand: the camera at c + (1, 0, 0.7), the target at c - (0, 0, tan 10 deg); with a = 0.7 + tan 10 deg and
    # L = sqrt(1 + a^2): forward = (-1, 0, -a) / L; right = forward x (0, 0, -1) = (0, fx, 0) -> (0, -1, 0) as fx < 0;
    # up = right x forward = (-fz, 0, fx) = (a, 0, -1) / L.  The extrinsic has these as ROWS, and t = -R pos.
    a = 0.7 + np.tan(np.radians(10.0))
    L = np.sqrt(1.0 + a * a)
    R0 = np.array([[0.0, -1.0, 0.0], [a / L, 0.0, -1.0 / L], [-1.0 / L, 0.0, -a / L]])
    pos0 = c + np.array([1.0, 0.0, 0.7])
    assert np.allclose(ext[0, :3, :3], R0, atol=1e-12) and np.allclose(ext[0, :3, 3], -R0 @ pos0, atol=1e-12)
    assert np.array_equal(ext[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (180, 1)))
    target = c - np.array([0.0, 0.0, np.tan(np.radians(10.0))])
    for i, e in enumerate(ext):
        R = e[:3, :3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) == pytest.approx(-1.0, abs=1e-12), i
        t = R @ target + e[:3, 3]  # the target in camera space: on the optical axis, in front
        assert abs(t[0]) < 1e-12 and abs(t[1]) < 1e-12 and t[2] == pytest.approx(L, abs=1e-12), i
        pos = -R.T @ e[:3, 3]  # on the circle above the centre
        ang = 2 * np.pi * i / 180
        assert np.allclose(pos, c + [np.cos(ang), np.sin(ang), 0.7], atol=1e-12)
    # other arguments; intrinsics; the packed rows
    e5 = VR.orbit_cameras([0, 0, 0], 5, radius=2.0, height=0.5, tilt_deg=0.0)
    assert e5.shape == (5, 4, 4) and np.allclose(-e5[0, :3, :3].T @ e5[0, :3, 3], [2.0, 0.0, 0.5])
    fx, fy, cx, cy = VR.default_intrinsics()
    assert fx == fy == pytest.approx(540.0 / np.tan(np.radians(30.0))) and (cx, cy) == (959.5, 539.5)
    rows = VR.pack_cameras(e5, VR.default_intrinsics(96, 64))
    assert rows.shape == (5, 16) and rows.dtype == np.float32
    assert np.allclose(rows[2, :12].reshape(3, 4), e5[2, :3], atol=1e-6) and np.allclose(rows[2, 12:], [32 / np.tan(np.radians(30)), 32 / np.tan(np.radians(30)), 47.5, 31.5])


def test_load_camera_trajectory_reads_column_major_matrices(tmp_path):
    ext0 = np.array([[0.0, -1.0, 0.0, 0.5], [0.6, 0.0, -0.8, -0.25], [-0.8, 0.0, -0.6, 2.0], [0.0, 0.0, 0.0, 1.0]])  # asymmetric
    ext1 = np.eye(4)
    ext1[:3, 3] = [1.0, 2.0, 3.0]
    K0 = np.array([[600.0, 0.0, 319.5], [0.0, 610.0, 239.5], [0.0, 0.0, 1.0]])
    K1 = np.array([[500.0, 0.0, 300.0], [0.0, 505.0, 200.0], [0.0, 0.0, 1.0]])
    cam = lambda e, k: {"class_name": "PinholeCameraParameters", "extrinsic": e.T.reshape(-1).tolist(),
                        "intrinsic": {"width": 640, "height": 480, "intrinsic_matrix": k.T.reshape(-1).tolist()},
                        "version_major": 1, "version_minor": 0}
    doc = {"class_name": "PinholeCameraTrajectory", "parameters": [cam(ext0, K0), cam(ext1, K1)], "version_major": 1, "version_minor": 0}
    assert doc["parameters"][0]["extrinsic"][12:15] == [0.5, -0.25, 2.0]  # column-major: the translation is the last column
    path = tmp_path / "trajectory.json"
    path.write_text(json.dumps(doc))
    traj = VR.load_camera_trajectory(path)
    assert traj["width"] == 640 and traj["height"] == 480
    assert np.array_equal(traj["extrinsics"], np.stack([ext0, ext1]))
    assert np.array_equal(traj["intrinsics"], [[600.0, 610.0, 319.5, 239.5], [500.0, 505.0, 300.0, 200.0]])
    rows = VR.pack_cameras(traj["extrinsics"], traj["intrinsics"])
    assert np.allclose(rows[0], np.r_[ext0[:3].reshape(-1), 600.0, 610.0, 319.5, 239.5])
    doc["parameters"][1]["intrinsic"]["width"] = 320
    path.write_text(json.dumps(doc))
    with pytest.raises(ValueError):
        VR.load_camera_trajectory(path)


def test_label_colors_match_matplotlib_in_both_modes():
    import matplotlib
    from matplotlib import cm

    cmap = matplotlib.colors.ListedColormap(cm.tab20.colors + cm.tab20c.colors, name="tab40")
    labels = np.array([0, 1, 2, 7, 19, 20, 39, 40, 57, -1, 3, -4], dtype=np.float64)
    # normalised: the map called with the float labels / max, negatives painted black afterwards
    want = cmap(labels / labels.max())[:, :3]
    want[labels < 0] = 0
    got = RC.label_colors(labels, normalise=True)
    assert got.dtype == np.uint8 and got.shape == (12, 3)
    assert np.array_equal(got, np.floor(want * 255.0).astype(np.uint8))
    assert np.array_equal(got[8], np.floor(np.asarray(cm.tab20c.colors[-1]) * 255))  # the largest label: the last entry
    # by index: the map called with the integer label (entries past the end take the last one)
    want = cmap(labels.astype(np.int64))[:, :3]
    want[labels < 0] = 0
    got = RC.label_colors(labels, normalise=False)
    assert np.array_equal(got, np.floor(want * 255.0).astype(np.uint8))
    assert np.array_equal(got[7], got[6]) and np.array_equal(got[8], got[6]) and not np.array_equal(got[5], got[6])
    assert np.array_equal(got[5], np.floor(np.asarray(cm.tab20c.colors[0]) * 255))  # entry 20 is the first of tab20c
    assert not got[9].any() and not got[11].any()
    # nothing positive: divided by 1
    assert np.array_equal(RC.label_colors(np.array([0.0, -1.0]), True), np.floor(np.array([cm.tab20.colors[0], (0, 0, 0)]) * 255))
    assert RC.label_colors(np.zeros(0), True).shape == (0, 3)


def _two_super_clusters():
    rng = np.random.default_rng(0)
    a0, a1, a2 = rng.normal(size=(4, 3)), rng.normal(size=(2, 3)), rng.normal(size=(3, 3))
    b0, b1 = rng.normal(size=(5, 3)), rng.normal(size=(1, 3))
    # dict order is not key order in the first entry: the concatenation follows the dict
    return [{"pcd": {2: a2, 0: a0, 1: a1}, "aabb": np.zeros((3, 6))}, {"pcd": {0: b0, 1: b1}, "aabb": np.zeros((2, 6))}], (a0, a1, a2, b0, b1)


def test_create_pcd_with_labels_and_labelled_result():
    data, (a0, a1, a2, b0, b1) = _two_super_clusters()
    pts, lab = RC.create_pcd_with_labels(data, 0, np.array([5.0, 6.0, 5.0]))
    assert np.array_equal(pts, np.concatenate([a2, a0, a1])) and lab.tolist() == [5.0] * 3 + [5.0] * 4 + [6.0] * 2
    pts, lab = RC.labelled_result(data, [np.array([1.0, 2.0, 1.0]), np.array([3.0, 0.0])])
    assert np.array_equal(pts, np.concatenate([a2, a0, a1, b0, b1]))
    assert lab.tolist() == [1.0] * 3 + [1.0] * 4 + [2.0] * 2 + [3.0] * 5 + [0.0]
    pts, lab = RC.labelled_result(data, [np.array([1.0, 2.0, 1.0])])  # only the super-clusters that were labelled
    assert len(pts) == 9
    pts, lab = RC.super_cluster_labels(data)
    assert len(pts) == 15 and lab.tolist() == [1.0] * 9 + [2.0] * 6


# ------------------------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_pointcloud_to_frames_writes_what_the_op_renders(tmp_path, capsys):
    import torch
    from PIL import Image

    from cropnerf_amd import ops

    rng = np.random.default_rng(2)
    blobs = np.concatenate([rng.normal(size=(400, 3)) * 0.04 + [0.0, 0.0, 0.15], rng.normal(size=(400, 3)) * 0.04 - [0.0, 0.0, 0.15]])
    labels = np.r_[np.full(400, 3), np.full(400, 24)]
    H, W = 48, 64
    cams = VR.pack_cameras(VR.orbit_cameras(blobs.mean(0), 3), VR.default_intrinsics(W, H))
    out = tmp_path / "frames"
    paths = VR.pointcloud_to_frames(blobs, labels=labels, output_dir=str(out), point_size=2, width=W, height=H, num_frames=3,
                                    frames_per_chunk=2)
    assert paths == [str(out / f"frame_{i:05d}.png") for i in range(3)] and all(os.path.exists(p) for p in paths)
    assert "frame_%05d.png" in capsys.readouterr().out
    colors = RC.label_colors(labels, False)
    dev = "cuda"
    want = ops.splat_points(torch.as_tensor(blobs, dtype=torch.float32).to(dev), torch.from_numpy(colors).to(dev),
                            torch.from_numpy(cams).to(dev), H, W, 2).cpu().numpy()
    c3, c24 = RC.label_colors(np.array([3, 24]), False)
    assert not np.array_equal(c3, c24)
    for i, p in enumerate(paths):
        frame = np.asarray(Image.open(p))
        assert frame.shape == (H, W, 3) and np.array_equal(frame, want[i]), i
        seen = {tuple(px) for px in frame.reshape(-1, 3)}
        assert seen == {tuple(c3), tuple(c24), (255, 255, 255)}, i
    # the same cameras handed in, a grey context cloud added: grey pixels appear, the frames keep their names
    tree = rng.uniform(-0.3, 0.3, size=(2000, 3))
    paths2 = VR.pointcloud_to_frames(blobs, labels=labels, full_tree=tree, output_dir=str(tmp_path / "ctx"), cameras=cams, width=W, height=H)
    assert len(paths2) == 3
    assert (155, 155, 155) in {tuple(px) for px in np.asarray(Image.open(paths2[0])).reshape(-1, 3)}


@pytest.mark.gpu
def test_video_renderer_cli_orbit_and_path(tmp_path, capsys):
    """``orbit`` with ``--cluster-info``: the clusters in the colours of super-cluster index + 1, the ``.ply`` as grey context;
    ``path``: the ``.ply`` in its own colours along a saved trajectory."""
    from PIL import Image

    from cropnerf_amd.fruit_nerf.ply import write_ply

    rng = np.random.default_rng(4)
    info = np.empty(2, dtype=object)
    for sc in range(2):
        info[sc] = {"pcd": {c: rng.normal(size=(300, 3)) * 0.03 + [0.0, 0.1 * c, 0.3 * sc - 0.15] for c in range(2)}, "aabb": np.zeros((2, 6))}
    np.save(tmp_path / "info.npy", info, allow_pickle=True)
    tree = rng.uniform([-0.2, 0.3, -0.2], [0.2, 0.5, 0.2], size=(3000, 3))  # beside the clusters as frame 0 sees them, not in front
    own = np.tile(np.array([[200, 30, 90]], np.uint8), (len(tree), 1))
    write_ply(str(tmp_path / "tree.ply"), tree, (own + 0.5) / 255.0)
    colours_of = lambda p: {tuple(px) for px in np.asarray(Image.open(p)).reshape(-1, 3)}
    out = tmp_path / "orbit"
    assert VR.main(["orbit", "--pcd", str(tmp_path / "tree.ply"), "--cluster-info", str(tmp_path / "info.npy"), "--output-dir", str(out),
                    "--num-frames", "2", "--width", "64", "--height-px", "48"]) == 0
    assert sorted(os.listdir(out)) == ["frame_00000.png", "frame_00001.png"] and "frame_%05d.png" in capsys.readouterr().out
    c1, c2 = (tuple(c) for c in RC.label_colors(np.array([1, 2]), False))
    assert colours_of(out / "frame_00000.png") == {c1, c2, (155, 155, 155), (255, 255, 255)}
    # a two-camera trajectory: the orbit's own first cameras, written the way open3d does (column-major)
    ext = VR.orbit_cameras(tree.mean(0), 2)
    fx, fy, cx, cy = VR.default_intrinsics(64, 48)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    doc = {"class_name": "PinholeCameraTrajectory", "parameters": [
        {"extrinsic": e.T.reshape(-1).tolist(), "intrinsic": {"width": 64, "height": 48, "intrinsic_matrix": K.T.reshape(-1).tolist()}}
        for e in ext]}
    (tmp_path / "traj.json").write_text(json.dumps(doc))
    out = tmp_path / "path"
    assert VR.main(["path", "--pcd", str(tmp_path / "tree.ply"), "--camera-json", str(tmp_path / "traj.json"), "--output-dir", str(out)]) == 0
    assert sorted(os.listdir(out)) == ["frame_00000.png", "frame_00001.png"]
    assert np.asarray(Image.open(out / "frame_00000.png")).shape == (48, 64, 3)
    assert colours_of(out / "frame_00000.png") == {(200, 30, 90), (255, 255, 255)}


def _projection_tree(base, recording):
    """The small tree of the merger's count test (two fruits, each split into two sub-clusters that carry one instance label
    in every view) plus the ``all_super_cluster_info.npy`` of the segmenter; returns the sub-cluster sizes."""
    from PIL import Image

    H, W, n_cams, k = 64, 96, 12, 2
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(3)
    root = base / "artifacts" / recording
    for sc in range(2):
        for cam in range(n_cams):
            d = root / "projection" / f"super_cluster_{sc}" / f"cam_{cam}"
            d.mkdir(parents=True)
            label = np.zeros((H, W), np.uint8)
            cx = 30 + 3 * cam
            for c in range(k):
                blob = ((yy - 32) ** 2 + (xx - (cx + 14 * c)) ** 2 <= 81) & (rng.uniform(size=(H, W)) > 0.05)
                img = np.repeat((blob * 255).astype(np.uint8)[..., None], 3, -1)
                Image.fromarray(img).save(d / f"wo_occ_cluster_{c}.png")
                Image.fromarray(img).save(d / f"visible_cluster_{c}.png")
                label[(yy - 32) ** 2 + (xx - (cx + 14 * c)) ** 2 <= 144] = 5 + sc
            Image.fromarray(label).save(d / "label_frame_00001.png")
    sizes = [[40, 31], [25, 52]]
    info = np.empty(2, dtype=object)
    for sc in range(2):
        info[sc] = {"pcd": {c: rng.normal(size=(sizes[sc][c], 3)) * 0.03 + [0.2 * sc, 0.05 * c, 0.0] for c in range(k)},
                    "aabb": np.zeros((k, 6))}
    (root / "pcd").mkdir()
    np.save(root / "pcd" / "all_super_cluster_info.npy", info, allow_pickle=True)
    return sum(map(sum, sizes))


@pytest.mark.gpu
def test_merger_visualize_writes_the_labelled_cloud_and_its_frames(tmp_path, capsys):
    from cropnerf_amd.fruit_nerf.ply import read_ply
    from cropnerf_amd.segmentation import merger

    n_points = _projection_tree(tmp_path, "rec")
    pcd_dir = tmp_path / "artifacts" / "rec" / "pcd"
    args = ["--base_dir", str(tmp_path), "--recording_name", "rec", "--frame_sampling_interval", "3"]
    before = sorted(os.listdir(pcd_dir))
    total = merger.main(args)
    assert total == 2 and "Total bool: 2" in capsys.readouterr().out
    assert sorted(os.listdir(pcd_dir)) == before  # without the flag nothing new is written
    total = merger.main(args + ["--visualize", "--vis_num_frames", "3", "--vis_width", "64", "--vis_height", "48"])
    printed = capsys.readouterr().out
    assert total == 2 and "Total bool: 2" in printed
    pts, cols = read_ply(str(pcd_dir / "full_tree_seg_result.ply"))
    assert len(pts) == n_points
    distinct = {tuple(c) for c in np.rint(cols * 255).astype(int)}
    assert len(distinct) == total
    assert distinct == {tuple(c) for c in RC.label_colors(np.array([1.0, 2.0]), True).astype(int)}
    frames = sorted(os.listdir(pcd_dir / "full_tree_seg_result_frames"))
    assert frames == [f"frame_{i:05d}.png" for i in range(3)]
