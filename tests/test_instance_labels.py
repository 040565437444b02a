"""Host side of the instance-label stage: the numpy definition (``_label_ref``), the equivalence it rests on (the merger's
affinity does not depend on WHICH bijection numbers the colours), the conversion command's file handling and the
merger's four ways to a label frame -- all with ``convert=`` the numpy helper, no GPU."""

import itertools

import numpy as np
import pytest
from _label_ref import labels_from_rgb, labels_only


def test_reference_on_a_hand_written_frame():
    """Keys are B << 16 | G << 8 | R: (1,0,0) = 1 < (0,1,0) = 256 < (0,0,1) = 65536 < (255,255,255)."""
    K, R, G, B, Wh = (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (255, 255, 255)
    frame = np.array([[K, R, B, Wh],
                      [B, B, K, G],
                      [Wh, R, G, K]], np.uint8)
    labels, colors, n = labels_from_rgb(frame[None])
    assert labels.dtype == np.uint8 and labels.shape == (1, 3, 4)
    assert labels[0].tolist() == [[0, 1, 3, 4],
                                  [3, 3, 0, 2],
                                  [4, 1, 2, 0]]
    assert n.tolist() == [4]
    assert colors[0, :6].tolist() == [0, 1, 256, 65536, 0xFFFFFF, 0] and not colors[0, 5:].any()


def test_reference_without_a_black_pixel_starts_at_one():
    frame = np.array([[(9, 9, 9), (3, 0, 0)], [(3, 0, 0), (0, 0, 2)]], np.uint8)
    labels, colors, n = labels_from_rgb(frame[None])
    assert labels[0].tolist() == [[3, 1], [1, 2]] and n.tolist() == [3]
    assert colors[0, :5].tolist() == [0, 3, 2 << 16, 9 << 16 | 9 << 8 | 9, 0]


def test_reference_is_per_frame_and_refuses_256_colours():
    a = np.zeros((2, 16, 16, 3), np.uint8)
    a[0, 0, 0] = (5, 0, 0)
    a[1, 0, 0] = (7, 0, 0)
    a[1, 0, 1] = (5, 0, 0)
    labels, _, n = labels_from_rgb(a)
    assert labels[0, 0, 0] == 1 and labels[1, 0, 0] == 2 and labels[1, 0, 1] == 1 and n.tolist() == [1, 2]
    a[0].reshape(-1, 3)[:, 0] = np.arange(256)  # black + 255 colours: fine
    assert labels_from_rgb(a)[2].tolist() == [255, 2]
    a[0, 0, 0] = (0, 1, 0)  # the 256th
    with pytest.raises(ValueError):
        labels_from_rgb(a)


def test_affinity_does_not_depend_on_the_numbering():
    """Every consumer compares labels for equality within one frame and against 0 (``calc_affinity``): any permutation of
    1..n, even a different one in every frame, leaves the affinity unchanged."""
    from cropnerf_amd.segmentation import merger

    rng = np.random.default_rng(0)
    n_cams, k, n = 9, 4, 3
    lab = rng.integers(0, n + 1, size=(k, n_cams))
    lab[0, :3] = lab[1, :3] = 2  # some agreement, some disagreement, some background
    lab[2, 3] = 0
    rel = rng.uniform(0.1, 1.0, size=(k, n_cams))
    prop = lambda L: {i: {"label": L[i].astype(np.float64), "reliability": rel[i]} for i in range(k)}
    want = merger.calc_affinity(prop(lab))
    assert (want > 0).any() and (want < 0).any()
    for perm in itertools.permutations(range(1, n + 1)):
        lut = np.array((0,) + perm)
        assert np.array_equal(merger.calc_affinity(prop(lut[lab])), want), perm
    per_cam = lab.copy()  # another bijection in every camera
    for c in range(n_cams):
        per_cam[:, c] = np.array((0,) + tuple(rng.permutation(np.arange(1, n + 1))))[lab[:, c]]
    assert np.array_equal(merger.calc_affinity(prop(per_cam)), want)


def _mask(h, w, seed, n_colors=5):
    rng = np.random.default_rng(seed)
    palette = np.concatenate([np.zeros((1, 3), np.uint8), rng.integers(1, 256, size=(n_colors, 3)).astype(np.uint8)])
    return palette[rng.integers(0, n_colors + 1, size=(h, w))]


def test_convert_img_to_label_files(tmp_path):
    """PNG, palette PNG, gray and RGBA inputs, two image sizes in one directory -> ``label_<stem>.png``, 8-bit gray, contents
    equal to the helper's on what ``.convert("RGB")`` makes of each file."""
    from PIL import Image

    from cropnerf_amd.fruit_nerf.utils.convert_segmentation_img_to_label import convert_img_to_label

    src, dst = tmp_path / "SegmentationObject", tmp_path / "out" / "SegmentationLabel"
    src.mkdir()
    for i in range(5):  # more than one batch of two, and a rest
        Image.fromarray(_mask(12, 20, i)).save(src / f"frame_{i:05d}.png")
    Image.fromarray(_mask(9, 7, 10)).save(src / "other_size.png")
    Image.fromarray(_mask(12, 20, 11)).convert("P", palette=Image.Palette.ADAPTIVE, colors=8).save(src / "palette.png")
    Image.fromarray((_mask(12, 20, 12)[..., 0] // 64 * 64).astype(np.uint8)).save(src / "gray.png")
    Image.fromarray(np.concatenate([_mask(12, 20, 13), np.full((12, 20, 1), 200, np.uint8)], -1)).save(src / "rgba.png")
    (src / "notes.txt").write_text("not an image")
    calls = []

    def convert(frames):
        calls.append(frames.shape)
        return labels_only(frames)

    written = convert_img_to_label(src, dst, batch_frames=2, convert=convert)
    names = sorted(p.name for p in dst.iterdir())
    assert names == sorted(f"label_{p.stem}.png" for p in src.iterdir() if p.suffix == ".png") and len(names) == 9
    assert sorted(written) == sorted(str(dst / n) for n in names)
    assert all(s[0] <= 2 and s[3] == 3 for s in calls) and {s[1:3] for s in calls} == {(12, 20), (9, 7)}
    for p in src.iterdir():
        if p.suffix != ".png":
            continue
        with Image.open(dst / f"label_{p.stem}.png") as im:
            assert im.mode == "L", p.name
            got = np.asarray(im)
        rgb = np.asarray(Image.open(p).convert("RGB"))
        assert np.array_equal(got, labels_only(rgb[None])[0]), p.name
    assert np.asarray(Image.open(dst / "label_palette.png")).max() >= 2


def test_convert_names_the_frame_that_overflows(tmp_path):
    from PIL import Image

    from cropnerf_amd.fruit_nerf.utils.convert_segmentation_img_to_label import convert_img_to_label

    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for i in range(4):
        Image.fromarray(_mask(16, 17, i)).save(src / f"frame_{i:05d}.png")
    bad = np.zeros((16, 17, 3), np.uint8)
    bad.reshape(-1, 3)[:256, 1] = np.arange(256)
    bad.reshape(-1, 3)[:256, 0] = 1
    Image.fromarray(bad).save(src / "frame_00002.png")
    with pytest.raises(ValueError, match="frame_00002.png"):
        convert_img_to_label(src, dst, batch_frames=3, convert=labels_only)
    assert sorted(p.name for p in dst.iterdir()) == ["label_frame_00000.png", "label_frame_00001.png"]


# ---- the merger's four ways to a label frame (the tree of tests/test_contours.py::test_merger_counts_from_a_projection_tree)

H, W, N_CAMS, K = 64, 96, 12, 2


def _disc(cam, c, r2):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - 32) ** 2 + (xx - (30 + 3 * cam + 14 * c)) ** 2 <= r2


def _label(sc, cam):
    label = np.zeros((H, W), np.uint8)
    for c in range(K):
        label[_disc(cam, c, 144)] = 5 + sc  # one instance covers both halves
    return label


def _tree(root, n_super=1, frame=True):
    from PIL import Image

    rng = np.random.default_rng(3)
    for sc in range(n_super):
        for cam in range(N_CAMS):
            d = root / "projection" / f"super_cluster_{sc}" / f"cam_{cam}"
            d.mkdir(parents=True)
            for c in range(K):  # the two halves of one fruit, side by side
                blob = _disc(cam, c, 81) & (rng.uniform(size=(H, W)) > 0.05)
                img = np.repeat((blob * 255).astype(np.uint8)[..., None], 3, -1)
                Image.fromarray(img).save(d / f"wo_occ_cluster_{c}.png")
                Image.fromarray(img).save(d / f"visible_cluster_{c}.png")
            if frame:
                Image.fromarray(rng.integers(0, 255, size=(H, W, 3)).astype(np.uint8)).save(d / f"frame_{cam + 1:05d}.png")
    return root / "projection" / "super_cluster_0"


def _refuse(frames):
    raise AssertionError("convert must not be called")


def test_rule1_a_label_frame_in_the_cam_directory_wins(tmp_path):
    from PIL import Image

    from cropnerf_amd.segmentation import merger

    sc_dir = _tree(tmp_path)
    label_dir = tmp_path / "SegmentationLabel"
    label_dir.mkdir()
    for cam in range(N_CAMS):
        Image.fromarray(_label(0, cam)).save(sc_dir / f"cam_{cam}" / f"label_frame_{cam + 1:05d}.png")
        Image.fromarray(np.full((H, W), 77, np.uint8)).save(label_dir / f"label_frame_{cam + 1:05d}.png")  # conflicting
    before = sorted(p.name for p in (sc_dir / "cam_3").iterdir())
    wo, vis, lab = merger.load_projection_tree(sc_dir, K, label_dir=label_dir, mask_dir=tmp_path / "nowhere", convert=_refuse)
    assert wo.shape == vis.shape == (N_CAMS, K, H, W) and lab.dtype == np.uint8
    assert all(np.array_equal(lab[cam], _label(0, cam)) for cam in range(N_CAMS))
    plain = merger.load_projection_tree(sc_dir, K)  # both None: as before
    assert all(np.array_equal(a, b) for a, b in zip(plain, (wo, vis, lab)))
    assert sorted(p.name for p in (sc_dir / "cam_3").iterdir()) == before


def test_rule2_reads_and_copies_from_the_label_directory(tmp_path):
    from PIL import Image

    from cropnerf_amd.segmentation import merger

    sc_dir = _tree(tmp_path)
    label_dir = tmp_path / "SegmentationLabel"
    label_dir.mkdir()
    for cam in range(N_CAMS):
        Image.fromarray(_label(0, cam)).save(label_dir / f"label_frame_{cam + 1:05d}.png")
    # a mask directory that would give other labels: rule 2 comes first
    _, _, lab = merger.load_projection_tree(sc_dir, K, label_dir=label_dir, mask_dir=label_dir, convert=_refuse)
    for cam in range(N_CAMS):
        assert np.array_equal(lab[cam], _label(0, cam))
        copied = sc_dir / f"cam_{cam}" / f"label_frame_{cam + 1:05d}.png"
        assert copied.read_bytes() == (label_dir / copied.name).read_bytes()
    _, _, again = merger.load_projection_tree(sc_dir, K)  # rule 1 now
    assert np.array_equal(again, lab)


def test_rule3_converts_masks_and_writes_label_frames(tmp_path, capsys):
    from PIL import Image

    from cropnerf_amd.segmentation import merger

    sc_dir = _tree(tmp_path)
    mask_dir = tmp_path / "SegmentationObject"
    mask_dir.mkdir()
    palette = np.array([(0, 0, 0), (0, 0, 200), (10, 0, 0), (0, 90, 0)], np.uint8)  # keys: 200 << 16, 10, 90 << 8
    index = {}
    for cam in range(N_CAMS):
        idx = np.zeros((H, W), np.int64)
        idx[_disc(cam, 0, 144)] = 1
        idx[_disc(cam, 1, 100)] = 2 + cam % 2
        index[cam] = idx
        ext = ".png" if cam % 3 else ".jpeg"  # same stem, another extension (lossless here: PNG bytes under that name)
        with open(mask_dir / f"frame_{cam + 1:05d}{ext}", "wb") as f:
            Image.fromarray(palette[idx]).save(f, format="PNG")
    calls = []

    def convert(frames):
        calls.append(frames.shape[0])
        return labels_only(frames)

    label_dir = tmp_path / "empty"
    label_dir.mkdir()
    _, _, lab = merger.load_projection_tree(sc_dir, K, label_dir=label_dir, mask_dir=mask_dir, convert=convert)
    assert calls == [N_CAMS] and capsys.readouterr().err == ""
    for cam in range(N_CAMS):
        # ranks WITHIN the frame: even cameras hold colours 1 and 2 (keys 200 << 16 > 10), odd ones 1 and 3 (200 << 16 > 90 << 8)
        rank = np.array([0, 2, 1, 0]) if cam % 2 == 0 else np.array([0, 2, 0, 1])
        assert np.array_equal(lab[cam], rank[index[cam]]) and set(np.unique(lab[cam])) == {0, 1, 2}, cam
        with Image.open(sc_dir / f"cam_{cam}" / f"label_frame_{cam + 1:05d}.png") as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), lab[cam])
    _, _, again = merger.load_projection_tree(sc_dir, K, convert=_refuse)  # a second call no longer needs mask_dir
    assert np.array_equal(again, lab)


def test_rule4_zeros_and_one_line_on_stderr(tmp_path, capsys):
    from PIL import Image

    from cropnerf_amd.segmentation import merger

    sc_dir = _tree(tmp_path)
    label_dir = tmp_path / "SegmentationLabel"
    label_dir.mkdir()
    Image.fromarray(_label(0, 4)).save(label_dir / "label_frame_00005.png")
    _, _, lab = merger.load_projection_tree(sc_dir, K, label_dir=label_dir, mask_dir=tmp_path / "nowhere", convert=_refuse)
    assert np.array_equal(lab[4], _label(0, 4)) and not np.delete(lab, 4, axis=0).any()
    cap = capsys.readouterr()
    lines = cap.err.strip().splitlines()
    assert cap.out == "" and len(lines) == 1
    assert f"{N_CAMS - 1} of {N_CAMS} cameras" in lines[0] and "cannot be merged" in lines[0] and "super_cluster_0" in lines[0]


def test_a_label_frame_of_another_size_raises(tmp_path):
    from PIL import Image

    from cropnerf_amd.segmentation import merger

    sc_dir = _tree(tmp_path)
    label_dir, mask_dir = tmp_path / "SegmentationLabel", tmp_path / "SegmentationObject"
    label_dir.mkdir()
    mask_dir.mkdir()
    Image.fromarray(np.zeros((H // 2, W // 2), np.uint8)).save(label_dir / "label_frame_00001.png")
    with pytest.raises(ValueError, match=rf"{W // 2} x {H // 2}.*{W} x {H}"):
        merger.load_projection_tree(sc_dir, K, label_dir=label_dir)
    Image.fromarray(np.zeros((H, W + 1, 3), np.uint8)).save(mask_dir / "frame_00001.png")
    with pytest.raises(ValueError, match=rf"{W + 1} x {H}.*{W} x {H}"):
        merger.load_projection_tree(sc_dir, K, mask_dir=mask_dir, convert=labels_only)


def test_ops_instance_labels_refuses_bad_input():
    import torch

    from cropnerf_amd import ops

    for bad in (torch.zeros(1, 4, 4, 3, dtype=torch.uint8),  # CPU
                torch.zeros(1, 4, 4, 3, dtype=torch.float32),
                torch.zeros(1, 4, 4, 4, dtype=torch.uint8)):
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            ops.instance_labels(bad)


def test_entry_point_validates_on_the_host():
    """Negative sizes, null pointers and a short workspace are refused before any HIP call; empty batches are no-ops."""
    import ctypes as C

    from cropnerf_amd import _lib

    lib = _lib.load()
    assert lib.cn_instance_labels_workspace_bytes(0) == 0
    per_frame = lib.cn_instance_labels_workspace_bytes(1)
    assert per_frame > 0 and lib.cn_instance_labels_workspace_bytes(7) == 7 * per_frame
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert lib.cn_instance_labels(None, 0, 4, 4, None, None, None, None, 0, None) == 0
    assert lib.cn_instance_labels(p, 3, 0, 4, p, p, p, p, 0, None) == 0
    assert lib.cn_instance_labels(p, -1, 4, 4, p, p, p, p, 64, None) == _lib.CN_ERR_INVALID
    assert lib.cn_instance_labels(p, 1, 4, -4, p, p, p, p, 64, None) == _lib.CN_ERR_INVALID
    assert lib.cn_instance_labels(None, 1, 4, 4, p, p, p, p, per_frame, None) == _lib.CN_ERR_INVALID
    assert b"cn_instance_labels" in lib.cn_last_error()
    assert lib.cn_instance_labels(p, 1, 4, 4, p, p, p, p, per_frame - 1, None) == _lib.CN_ERR_INVALID
    assert b"workspace" in lib.cn_last_error()


def test_convert_command_help_parses(capsys):
    from cropnerf_amd.fruit_nerf.utils import convert_segmentation_img_to_label as cmd

    with pytest.raises(SystemExit) as e:
        cmd.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("recording", "--base-dir", "--input-dir", "--output-dir", "--batch-frames"):
        assert flag in out
