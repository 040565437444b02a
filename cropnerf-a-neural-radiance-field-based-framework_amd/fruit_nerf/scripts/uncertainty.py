#!/usr/bin/env python
"""BayesRays for a trained run (``crop_nerf/fruit_nerf/bayesrays``; argparse instead of tyro).

``uncertainty.py compute`` -- the Hessian grid (``bayesrays/uncertainty.py``, the same field names):

    python uncertainty.py compute --load-config RUN/config.json [--output-path unc.npy] [--lod 8] [--iters 1000]

Writes ``(2^lod + 1)^3`` float32 values with ``np.save`` and prints N (batches x rays per batch: what ``render --N`` takes)
and the elapsed time.

``uncertainty.py render`` -- uncertainty and filtered views from such a grid (``output_uncertainty.py`` as
``run_viewer_u.py:357-382`` sets it up; an image per eval camera instead of the viewer):

    python uncertainty.py render --load-config RUN/config.json --unc-path unc.npy --output-dir OUT \
        [--filter-out] [--filter-thresh 0.5] [--white-bg | --black-bg] [--num-rays 32768] [--N 4096000]

Writes ``OUT/<stem>_uncertainty.png`` and ``OUT/<stem>_rgb.png`` per eval camera (the training cameras when the run holds no
eval split).
"""

from __future__ import annotations

import argparse
import os
import sys
import time
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch


@dataclass
class ComputeUncertainty:
    """Fields as ``bayesrays/uncertainty.py:33-42``."""

    load_config: Path
    output_path: Path = Path("unc.npy")
    lod: int = 8
    iters: int = 1000

    def main(self) -> None:
        from cropnerf_amd.fruit_nerf import bayesrays as B
        from cropnerf_amd.fruit_nerf.checkpoint import eval_setup

        if not 1 <= self.lod <= 10:
            raise SystemExit("--lod must lie in [1, 10]")
        _, pipeline, _, _ = eval_setup(self.load_config, test_mode="test")
        self.output_path.parent.mkdir(parents=True, exist_ok=True)
        start = time.time()
        hessian, n = B.compute_hessian(pipeline.model, pipeline.datamanager, self.lod, self.iters)
        elapsed = time.time() - start
        with open(str(self.output_path), "wb") as f:
            np.save(f, hessian)
        print(f"Saved {hessian.size} Hessian values (lod {self.lod}) to {self.output_path}")
        print(f"N = {n} rays")
        print(f"Execution time: {elapsed:.6f} seconds")


@dataclass
class RenderUncertainty:
    """Fields as ``run_viewer_u.py:343-355`` plus what the viewer's slider and ``output_uncertainty.py:44`` hold."""

    load_config: Path
    unc_path: Path = Path("unc.npy")
    output_dir: Path = Path("uncertainty")
    filter_out: bool = False
    filter_thresh: float = 0.5
    white_bg: bool = False
    black_bg: bool = False
    num_rays: int = 1 << 15
    N: float = 1000 * 4096

    def main(self) -> None:
        from cropnerf_amd.fruit_nerf import bayesrays as B

        hessian, lod = B.load_hessian(self.unc_path)  # before anything is loaded: a missing file fails here
        from cropnerf_amd.fruit_nerf.checkpoint import eval_setup
        from cropnerf_amd.fruit_nerf.fruit_nerf import save_image

        _, pipeline, _, _ = eval_setup(self.load_config, test_mode="test")
        model = pipeline.model.eval()
        state = B.UncertaintyState(hessian, self.N, lod, self.filter_out, self.filter_thresh, self.white_bg, self.black_bg)
        dataset = getattr(pipeline.datamanager, "eval_dataset", None)
        if dataset is None or len(dataset) == 0:
            print("The run holds no eval cameras: rendering the training cameras.")
            dataset = pipeline.datamanager.train_dataset
        self.output_dir.mkdir(parents=True, exist_ok=True)
        cameras = dataset.cameras.to(model.device)
        print(f"lod {lod}, N {self.N:g}, filter_out {self.filter_out} (threshold {self.filter_thresh}), {len(cameras)} cameras")
        for idx in range(len(cameras)):
            rays = cameras.generate_rays(camera_indices=idx, keep_shape=True)
            height, width = rays.origins.shape[:2]
            flat = rays.flatten()
            parts = {"rgb": [], "uncertainty": []}
            for i in range(0, len(flat), self.num_rays):
                out = B.get_outputs_with_uncertainty(model, flat[i:i + self.num_rays], state)
                for k in parts:
                    parts[k].append(out[k])
            stem = Path(str(dataset.image_filenames[idx])).stem
            save_image(torch.cat(parts["rgb"]).view(height, width, 3), os.path.join(self.output_dir, f"{stem}_rgb.png"))
            save_image(torch.cat(parts["uncertainty"]).view(height, width, 1).expand(height, width, 3),
                       os.path.join(self.output_dir, f"{stem}_uncertainty.png"))
        print(f"Saved {2 * len(cameras)} images to {self.output_dir}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compute")
    c.add_argument("--load-config", type=Path, required=True)
    c.add_argument("--output-path", type=Path, default=Path("unc.npy"))
    c.add_argument("--lod", type=int, default=8)
    c.add_argument("--iters", type=int, default=1000)
    r = sub.add_parser("render")
    r.add_argument("--load-config", type=Path, required=True)
    r.add_argument("--unc-path", type=Path, required=True)
    r.add_argument("--output-dir", type=Path, required=True)
    r.add_argument("--filter-out", action="store_true")
    r.add_argument("--filter-thresh", type=float, default=0.5)
    bg = r.add_mutually_exclusive_group()
    bg.add_argument("--white-bg", action="store_true")
    bg.add_argument("--black-bg", action="store_true")
    r.add_argument("--num-rays", type=int, default=1 << 15)
    r.add_argument("--N", type=float, default=1000 * 4096, help="rays seen by the Hessian stage: iterations x rays per batch")
    return ap


def entrypoint(argv=None):
    a = build_parser().parse_args(argv)
    if a.cmd == "compute":
        ComputeUncertainty(a.load_config, a.output_path, a.lod, a.iters).main()
        return
    if a.num_rays <= 0:
        raise SystemExit("--num-rays must be positive")
    RenderUncertainty(a.load_config, a.unc_path, a.output_dir, a.filter_out, a.filter_thresh, a.white_bg, a.black_bg,
                      a.num_rays, a.N).main()


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[3]))
    entrypoint()
