"""Time the instance-label conversion (csrc/labels.hip) on a recording-sized input: 147 synthetic frames of 1440 x 1920 (the
capture fixture's count and size) with a few dozen coloured blobs each.

    python tools/label_probe.py [--frames 147] [--batch-frames 32] [--numpy-frames 4]

Prints: the device conversion end to end (host arrays in, label arrays out, batches of --batch-frames) and per launch (events
around ``cn_instance_labels`` on frames already in device memory); the numpy restatement (``np.unique`` with
``return_inverse``) per frame on this machine; and what decoding / encoding one such frame as PNG costs, which is what a user
of the command waits for.  No test depends on these numbers."""

from __future__ import annotations

import argparse
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 1440, 1920


def synthetic_frame(rng, blobs: int = 36) -> np.ndarray:
    frame = np.zeros((H, W, 3), np.uint8)
    for _ in range(blobs):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(20, 120))
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        frame[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, 256, size=3)
    return frame


def numpy_labels(frame: np.ndarray) -> np.ndarray:
    f = frame.astype(np.uint32)
    keys = (f[..., 2] << 16) | (f[..., 1] << 8) | f[..., 0]
    uniq, inv = np.unique(keys.reshape(-1), return_inverse=True)
    if uniq[0] != 0:
        inv = inv + 1
    return inv.reshape(keys.shape).astype(np.uint8)


def main(argv=None) -> None:
    import torch
    from PIL import Image

    from cropnerf_amd import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=147)
    ap.add_argument("--batch-frames", type=int, default=32)
    ap.add_argument("--numpy-frames", type=int, default=4)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(0)
    frames = np.stack([synthetic_frame(rng) for _ in range(a.frames)])
    print(f"{a.frames} frames of {H} x {W}, {frames.nbytes / 1e9:.2f} GB of RGB", flush=True)

    def convert_all():
        out = []
        for at in range(0, a.frames, a.batch_frames):
            out.append(ops.instance_labels(torch.from_numpy(frames[at:at + a.batch_frames]).cuda())["labels"].cpu().numpy())
        return np.concatenate(out)

    convert_all()  # warm-up: library load, allocator
    torch.cuda.synchronize()
    t = time.perf_counter()
    labels = convert_all()
    end_to_end = time.perf_counter() - t
    print(f"device, end to end (host in, host out, batches of {a.batch_frames}): {end_to_end * 1e3:.1f} ms "
          f"= {end_to_end / a.frames * 1e3:.2f} ms per frame", flush=True)

    dev = torch.from_numpy(frames[:a.batch_frames]).cuda()
    n = dev.shape[0]
    times = []
    for _ in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.instance_labels(dev)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times = sorted(times[2:])
    med = times[len(times) // 2]
    moved = n * H * W * 7 / 1e9  # 3 B in twice, 1 B out
    print(f"device, one call on {n} resident frames: median {med:.3f} ms, min {times[0]:.3f} ms "
          f"= {med / n:.4f} ms per frame, {moved / (med * 1e-3):.0f} GB/s of the 7 B per pixel the passes move; "
          f"{a.frames} frames: {med / n * a.frames:.2f} ms", flush=True)

    k = min(a.numpy_frames, a.frames)
    t = time.perf_counter()
    ref = [numpy_labels(frames[i]) for i in range(k)]
    per_frame = (time.perf_counter() - t) / k
    assert all(np.array_equal(r, labels[i]) for i, r in enumerate(ref)), "device labels differ from the numpy restatement"
    print(f"numpy restatement (np.unique, return_inverse): {per_frame * 1e3:.1f} ms per frame over {k} frames "
          f"= {per_frame * a.frames:.1f} s for {a.frames} frames (labels equal to the device's)", flush=True)

    buf = io.BytesIO()
    t = time.perf_counter()
    Image.fromarray(frames[0]).save(buf, format="PNG")
    enc_rgb = time.perf_counter() - t
    t = time.perf_counter()
    np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    dec = time.perf_counter() - t
    out = io.BytesIO()
    t = time.perf_counter()
    Image.fromarray(labels[0]).save(out, format="PNG")
    enc = time.perf_counter() - t
    print(f"PNG, one frame on one thread: decode mask {dec * 1e3:.1f} ms, encode label frame {enc * 1e3:.1f} ms "
          f"(mask file {len(buf.getvalue()) / 1e3:.0f} kB, written in {enc_rgb * 1e3:.0f} ms) "
          f"= {(dec + enc) * a.frames:.1f} thread-seconds for {a.frames} frames", flush=True)


if __name__ == "__main__":
    main()
