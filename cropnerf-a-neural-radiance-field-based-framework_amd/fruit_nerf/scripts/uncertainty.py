#!/usr/bin/env python
"""``uncertainty.py render`` -- BayesRays uncertainty and filtered views of a trained run from a Hessian grid (the consumer side
of ``crop_nerf/fruit_nerf/bayesrays``: ``output_uncertainty.py`` as ``run_viewer_u.py:357-382`` sets it up; argparse instead of
tyro, an image per eval camera instead of the viewer).

    python uncertainty.py render --load-config RUN/config.json --unc-path unc.npy --output-dir OUT \
        [--filter-out] [--filter-thresh 0.5] [--white-bg | --black-bg] [--num-rays 32768] [--N 4096000]

Writes ``OUT/<stem>_uncertainty.png`` and ``OUT/<stem>_rgb.png`` per eval camera (the training cameras when the run holds no
eval split).  ``unc.npy`` is what the reference's ``bayesrays/uncertainty.py`` saves: ``(2^lod + 1)^3`` Hessian values.
"""

from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass
from pathlib import Path

import torch


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
    if a.num_rays <= 0:
        raise SystemExit("--num-rays must be positive")
    RenderUncertainty(a.load_config, a.unc_path, a.output_dir, a.filter_out, a.filter_thresh, a.white_bg, a.black_bg,
                      a.num_rays, a.N).main()


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[3]))
    entrypoint()
