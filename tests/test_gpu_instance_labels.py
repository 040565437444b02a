"""``cn_instance_labels`` (csrc/labels.hip) against its numpy definition (``_label_ref``), bit for bit, and the merger finding
its label frames end to end on the device."""

import shutil

import numpy as np
import pytest
from _label_ref import labels_from_rgb

pytestmark = pytest.mark.gpu


def _run(frames):
    import torch

    from cropnerf_amd import ops

    out = ops.instance_labels(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    assert out["labels"].dtype == torch.uint8 and out["num_colors"].dtype == torch.int32
    return out["labels"].cpu().numpy(), out["colors"].cpu().numpy().astype(np.int64), out["num_colors"].cpu().numpy()


def _check(frames):
    got = _run(frames)
    want = labels_from_rgb(frames)
    for name, g, w in zip(("num_colors", "colors", "labels"), got[::-1], want[::-1]):
        assert g.shape == w.shape and np.array_equal(g, w), name
    return got


def _palette_frames(F, H, W, n_colors, seed):
    rng = np.random.default_rng(seed)
    frames = np.zeros((F, H, W, 3), np.uint8)
    for f in range(F):  # another palette in every frame: nothing may leak across frames
        palette = np.concatenate([np.zeros((1, 3), np.uint8), rng.integers(0, 256, size=(n_colors, 3)).astype(np.uint8)])
        idx = np.concatenate([np.arange(n_colors + 1), rng.integers(0, n_colors + 1, size=H * W - n_colors - 1)])  # each once
        frames[f] = palette[rng.permutation(idx)].reshape(H, W, 3)
    return frames


def test_frames_that_start_off_dword_alignment():
    """A 5 x 7 frame is 105 bytes: frames 1 and 2 start at bytes 105 and 210, heads and tails go through the byte path."""
    frames = _palette_frames(3, 5, 7, 6, seed=1)
    _, _, n = _check(frames)
    assert n.tolist() == [6, 6, 6]


def test_one_pixel():
    labels, colors, n = _check(np.array([[[[0, 3, 0]]]], np.uint8))
    assert labels.tolist() == [[[1]]] and n.tolist() == [1] and colors[0, 1] == 3 << 8


def test_255_colours_and_an_all_black_frame():
    rng = np.random.default_rng(2)
    i = np.arange(1, 256)
    palette = np.concatenate([np.zeros((1, 3), np.int64), np.stack([i, 7 * i % 256, 255 - i], 1)]).astype(np.uint8)
    idx = np.concatenate([np.arange(256), rng.integers(0, 256, size=48 * 64 - 256)])  # each at least once
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    frames[0] = palette[rng.permutation(idx)].reshape(48, 64, 3)
    _, colors, n = _check(frames)
    assert n.tolist() == [255, 0] and not colors[1].any()


def test_colours_that_differ_in_one_channel_only():
    rng = np.random.default_rng(3)
    frames = np.zeros((3, 24, 32, 3), np.uint8)
    idx = rng.permutation(np.concatenate([np.arange(256), rng.integers(0, 256, size=24 * 32 - 256)])).reshape(24, 32)
    frames[0, ..., 0] = idx  # (i, 0, 0)
    frames[1, ..., 2] = idx  # (0, 0, i)
    four = np.array([(0, 0, 0), (255, 255, 255), (0, 0, 255), (255, 0, 0), (0, 255, 0)], np.uint8)
    frames[2] = four[rng.integers(0, 5, size=(24, 32))]
    labels, colors, n = _check(frames)
    assert n.tolist() == [255, 255, 4]
    assert colors[2, 1:5].tolist() == [255, 255 << 8, 255 << 16, 0xFFFFFF]  # red < green < blue < white


@pytest.mark.parametrize("where", ["first", "last"])
def test_a_colour_in_exactly_one_pixel(where):
    frames = _palette_frames(3, 37, 53, 5, seed=4)  # 37 * 53 * 3 bytes per frame: odd, so every alignment of a frame's start occurs
    f, y, x = (1, 0, 0) if where == "first" else (2, 36, 52)
    frames[f, y, x] = (1, 2, 3)
    assert (frames.reshape(-1, 3) == (1, 2, 3)).all(1).sum() == 1
    labels, colors, n = _check(frames)
    assert n[f] == 6 and colors[f, labels[f, y, x]] == 3 << 16 | 2 << 8 | 1


def _disc_frames(F, H, W, n_discs, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.zeros((F, H, W, 3), np.uint8)
    for f in range(F):
        for _ in range(n_discs):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(8, 40)
            frames[f][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, 256, size=3)
    return frames


@pytest.fixture(scope="module")
def discs():
    return _disc_frames(2, 480, 640, 40, seed=5)


def test_many_workgroups_feed_one_table(discs):
    _, _, n = _check(discs)
    assert (n > 20).all()


def test_tables_are_cleared_at_every_call(discs):
    first = _run(discs)
    other = _run(_palette_frames(2, 480, 640, 200, seed=6))  # a different batch in between, same shape, other keys
    assert (other[2] == 200).all()
    second = _run(discs)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert np.array_equal(first[0], labels_from_rgb(discs)[0])


def test_overflow_is_reported_per_frame():
    import ctypes as C

    import torch

    from cropnerf_amd import _lib, ops

    frames = _palette_frames(3, 32, 32, 9, seed=7)
    i = np.random.default_rng(8).permutation(np.arange(1024) % 256)
    frames[1] = np.stack([1 + i % 16, i // 16, np.full(1024, 9)], 1).reshape(32, 32, 3)  # exactly 256 colours, none black
    assert len(np.unique(frames[1].reshape(-1, 3), axis=0)) == 256
    dev = torch.from_numpy(frames).cuda()
    with pytest.raises(ValueError, match=r"\[1\]"):
        ops.instance_labels(dev)
    lib = _lib.load()
    labels = torch.zeros(3, 32, 32, dtype=torch.uint8, device="cuda")
    colors = torch.zeros(3, 256, dtype=torch.int32, device="cuda")
    num = torch.zeros(3, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.cn_instance_labels_workspace_bytes(3)), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.cn_instance_labels(p(dev), 3, 32, 32, p(labels), p(colors), p(num), p(ws), ws.numel(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    want = labels_from_rgb(frames[[0, 2]])
    assert num.cpu().tolist() == [int(want[2][0]), 256, int(want[2][1])]
    assert np.array_equal(labels.cpu().numpy()[[0, 2]], want[0])
    assert np.array_equal(colors.cpu().numpy()[[0, 2]].astype(np.int64), want[1])


def test_overflow_that_no_single_workgroup_sees():
    """Colours laid out in stripes of 1024 pixels with a period of 8 stripes, 40 (frame 0) or 31 (frame 1) colours per stripe
    class: wherever the kernel cuts a frame into workgroups, the 320 colours of frame 0 are found only once the workgroups'
    sets are merged, and the 248 of frame 1 must all be there."""
    import torch

    from cropnerf_amd import ops

    H_, W_ = 128, 512
    rng = np.random.default_rng(9)
    stripe = (np.arange(H_ * W_) // 1024) % 8
    frames = np.zeros((2, H_, W_, 3), np.uint8)
    for f, per in enumerate((40, 31)):
        c = 1 + stripe * per + rng.integers(0, per, size=H_ * W_)  # 1 .. 8 * per
        frames[f] = np.stack([c % 256, c // 256 + 1, (c * 7) % 256], 1).reshape(H_, W_, 3)
    assert [len(np.unique(fr.reshape(-1, 3), axis=0)) for fr in frames] == [320, 248]
    with pytest.raises(ValueError, match=r"\[0\]"):
        ops.instance_labels(torch.from_numpy(frames).cuda())
    _, _, n = _check(frames[1:])
    assert n.tolist() == [248]


# ---- end to end: the tree of tests/test_contours.py::test_merger_counts_from_a_projection_tree without label frames

H, W, N_CAMS, K = 64, 96, 12, 2


def _disc(cam, c, r2):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - 32) ** 2 + (xx - (30 + 3 * cam + 14 * c)) ** 2 <= r2


def _recording(base, one_colour_per_fruit=True):
    """artifacts/R/projection (two super-clusters, no label_frame*.png), artifacts/R/pcd/all_super_cluster_info.npy and
    training_data/R/SegmentationObject with the colour masks."""
    from PIL import Image

    rng = np.random.default_rng(3)
    masks = base / "training_data" / "R" / "SegmentationObject"
    masks.mkdir(parents=True)
    mask = {cam: np.zeros((H, W, 3), np.uint8) for cam in range(N_CAMS)}
    for sc in range(2):
        for cam in range(N_CAMS):
            d = base / "artifacts" / "R" / "projection" / f"super_cluster_{sc}" / f"cam_{cam}"
            d.mkdir(parents=True)
            for c in range(K):  # the two halves of one fruit, side by side
                blob = _disc(cam, c, 81) & (rng.uniform(size=(H, W)) > 0.05)
                img = np.repeat((blob * 255).astype(np.uint8)[..., None], 3, -1)
                Image.fromarray(img).save(d / f"wo_occ_cluster_{c}.png")
                Image.fromarray(img).save(d / f"visible_cluster_{c}.png")
            Image.fromarray(rng.integers(0, 255, size=(H, W, 3)).astype(np.uint8)).save(d / f"frame_{cam + 1:05d}.png")
    # both super-clusters project to the same pixels in this tree, so one mask per camera serves both
    for cam in range(N_CAMS):
        for c in range(K):
            mask[cam][_disc(cam, c, 144)] = (200, 30, 40) if one_colour_per_fruit else ((200, 30, 40), (20, 250, 60))[c]
        Image.fromarray(mask[cam]).save(masks / f"frame_{cam + 1:05d}.png")
    pcd = base / "artifacts" / "R" / "pcd"
    pcd.mkdir(parents=True)
    np.save(pcd / "all_super_cluster_info.npy", np.array([{"aabb": np.zeros((K, 6))} for _ in range(2)], dtype=object),
            allow_pickle=True)
    return ["--base_dir", str(base), "--recording_name", "R", "--frame_sampling_interval", "3"]


def _drop_written_labels(base):
    for p in (base / "artifacts" / "R" / "projection").glob("super_cluster_*/cam_*/label_*.png"):
        p.unlink()


def test_merger_main_finds_the_masks(tmp_path, capsys):
    from cropnerf_amd.segmentation import merger

    argv = _recording(tmp_path)
    assert merger.main(argv) == 2
    cap = capsys.readouterr()
    assert "0_th super cluster has: 1." in cap.out and "1_th super cluster has: 1." in cap.out and cap.err == ""
    assert len(list((tmp_path / "artifacts" / "R" / "projection").glob("super_cluster_*/cam_*/label_frame_*.png"))) == 2 * N_CAMS
    # without the recording's masks every sub-cluster is a fruit of its own -- what the merger printed before it looked there
    shutil.rmtree(tmp_path / "training_data")
    _drop_written_labels(tmp_path)
    assert merger.main(argv) == 4
    assert capsys.readouterr().err.count("cannot be merged") == 2


def test_merger_main_keeps_two_colours_apart(tmp_path):
    from cropnerf_amd.segmentation import merger

    assert merger.main(_recording(tmp_path, one_colour_per_fruit=False)) == 4


def test_convert_command_then_merger_with_label_frames_only(tmp_path, capsys):
    from cropnerf_amd.fruit_nerf.utils import convert_segmentation_img_to_label as cmd
    from cropnerf_amd.segmentation import merger

    argv = _recording(tmp_path)
    assert cmd.main(["R", "--base-dir", str(tmp_path), "--batch-frames", "5"]) == N_CAMS
    shutil.rmtree(tmp_path / "training_data" / "R" / "SegmentationObject")
    assert sorted(p.name for p in (tmp_path / "training_data" / "R" / "SegmentationLabel").iterdir()) == \
        [f"label_frame_{cam + 1:05d}.png" for cam in range(N_CAMS)]
    assert merger.main(argv) == 2
    assert capsys.readouterr().err == ""
