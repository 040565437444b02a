"""Colour instance masks -> 8-bit label frames -- mirror of ``fruit_nerf/utils/convert_segmentation_img_to_label.py``,
step 1 of the reference's workflow.

    python -m cropnerf_amd.fruit_nerf.utils.convert_segmentation_img_to_label plant_1 [--base-dir /opt/data]
        [--input-dir D] [--output-dir D] [--batch-frames 32]

Every mask ``<base>/training_data/<R>/SegmentationObject/<frame>`` becomes
``<base>/training_data/<R>/SegmentationLabel/label_<stem>.png``, the file the merger's image stage reads.  The labels are
those of ``cn_instance_labels`` (``csrc/labels.hip``): 0 for black, else 1 + the number of smaller distinct colours of the
frame, colours compared as ``B << 16 | G << 8 | R``.  The reference numbers the colours in the iteration order of a
Python ``set`` and looks every pixel up in a ``dict``; its consumers compare labels for equality within a frame and against
0 only, so any numbering gives the same fruit count.

Differences from the reference: the output is ALWAYS an 8-bit gray PNG (the reference writes ``label_<frame>`` with the
frame's own extension, so a ``.jpg`` mask would get JPEG-compressed labels); a frame without a black pixel is valid; a
frame with more than 255 colours is an error that names the file instead of a label that wraps.  Frames are read with PIL
as RGB, which is what ``cv2.imread``'s default mode makes of gray, palette and RGBA files."""

from __future__ import annotations

import argparse
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Tuple

import numpy as np

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def read_rgb(path) -> np.ndarray:
    from PIL import Image

    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def device_convert(device="cuda") -> Callable[[np.ndarray], np.ndarray]:
    """[F,H,W,3] uint8 array -> [F,H,W] uint8 labels through ``ops.instance_labels``."""

    def convert(frames: np.ndarray) -> np.ndarray:
        import torch

        from ... import ops

        out = ops.instance_labels(torch.from_numpy(np.ascontiguousarray(frames)).to(device))
        return out["labels"].cpu().numpy()

    return convert


def convert_img_to_label(input_dir, output_dir, batch_frames: int = 32, device="cuda", convert=None) -> List[str]:
    """Every image of ``input_dir`` -> ``output_dir/label_<stem>.png`` (8-bit gray).  Files are decoded on a thread pool,
    grouped by image size and sent to ``convert`` (default: the device path) in batches of at most ``batch_frames`` frames.
    A frame with more than 255 colours raises ``ValueError`` naming it; the batches before it stay written.  Returns the
    paths written, in the order of the sorted directory listing within each size."""
    from PIL import Image

    from ..projection import _worker_count

    if batch_frames < 1:
        raise ValueError(f"batch_frames = {batch_frames}")
    convert = convert or device_convert(device)
    names = sorted(n for n in os.listdir(str(input_dir)) if n.lower().endswith(IMAGE_EXTENSIONS))
    os.makedirs(str(output_dir), exist_ok=True)
    written: List[str] = []
    pending: Dict[Tuple[int, int], List[Tuple[str, np.ndarray]]] = {}

    def flush(group: List[Tuple[str, np.ndarray]], pool) -> None:
        try:
            labels = np.asarray(convert(np.stack([a for _, a in group])))
        except ValueError as e:  # a frame with too many colours: name its file, keep the frames before it
            if len(group) == 1:
                raise ValueError(f"{os.path.join(str(input_dir), group[0][0])}: more than 255 non-black colours "
                                 f"(not an instance mask?)") from e
            for item in group:
                flush([item], pool)
            raise
        paths = [os.path.join(str(output_dir), f"label_{os.path.splitext(n)[0]}.png") for n, _ in group]
        list(pool.map(lambda pl: Image.fromarray(np.ascontiguousarray(pl[1], dtype=np.uint8)).save(pl[0]),
                      zip(paths, labels)))
        written.extend(paths)

    with ThreadPoolExecutor(max_workers=_worker_count()) as pool:
        # decoded a batch's worth at a time, so that host memory stays bounded as well
        for at in range(0, len(names), batch_frames):
            chunk = names[at:at + batch_frames]
            for name, arr in zip(chunk, pool.map(lambda n: read_rgb(os.path.join(str(input_dir), n)), chunk)):
                group = pending.setdefault(arr.shape[:2], [])
                group.append((name, arr))
                if len(group) == batch_frames:
                    flush(group, pool)
                    group.clear()
        for group in pending.values():
            if group:
                flush(group, pool)
    return written


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="colour instance masks (SegmentationObject) -> label frames (SegmentationLabel)")
    ap.add_argument("recording", type=str, help="recording name, e.g. plant_1")
    ap.add_argument("--base-dir", type=str, default="/opt/data")
    ap.add_argument("--input-dir", type=str, default=None, help="default: <base-dir>/training_data/<recording>/SegmentationObject")
    ap.add_argument("--output-dir", type=str, default=None, help="default: <base-dir>/training_data/<recording>/SegmentationLabel")
    ap.add_argument("--batch-frames", type=int, default=32, help="frames per device call")
    a = ap.parse_args(argv)
    root = os.path.join(a.base_dir, "training_data", a.recording)
    written = convert_img_to_label(a.input_dir or os.path.join(root, "SegmentationObject"),
                                   a.output_dir or os.path.join(root, "SegmentationLabel"), a.batch_frames)
    print(f"{len(written)} label frames written")
    return len(written)


if __name__ == "__main__":
    main()
