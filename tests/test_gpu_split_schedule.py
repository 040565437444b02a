"""The image-width hint under the four-ray team kernel (render_split_kernel in the split-bf16 and fp16 matrix modes).

With `cn_render_opts.image_width / pixel_start` the team kernel enumerates only the pixels of the batch, cuts them into
equal per-XCD ranges and walks column stripes in 2 x 2 blocks (render_split.hpp: QuadSched).  The hint is a pure
scheduling choice: every ray must be rendered exactly once and bit-identically to the run without the hint, at any
width, offset, partial first / last row and batch size -- including batches that fill fewer pairs than the device has.
"""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from _helpers import dev_params, make_scene, product_specs, rays_with_box, to_dev

pytestmark = pytest.mark.gpu

S = 64
OUTS = ("rgb", "accumulation", "depth", "semantics", "semantics_colormap", "weights")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from cropnerf_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def setup(ops):
    scene = make_scene(seed=0)
    fspec, _ = product_specs(scene)
    fh = ops.FieldHandle(dev_params(scene), fspec)
    rb = rays_with_box(scene, 3)
    return scene, fh, rb


def _render_poisoned(ops, fh, sc, opts, o, d, n, f):
    """cn_render_rays into output buffers pre-filled with NaN (the launch only writes them: a ray the schedule skipped keeps
    its poison)."""
    from cropnerf_amd import _lib as L

    R = o.shape[0]
    out = {k: torch.full((R, w), float("nan"), device="cuda")
           for k, w in (("rgb", 3), ("accumulation", 1), ("depth", 1), ("semantics", 1), ("semantics_colormap", 3), ("weights", S))}
    ws = fh.workspace()
    L.check(L.load().cn_render_rays(C.byref(fh.struct), C.byref(sc), C.byref(opts), o.data_ptr(), d.data_ptr(), n.data_ptr(),
                                    f.data_ptr(), None, None, R, *(out[k].data_ptr() for k in OUTS), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


# (image width, first pixel, rays): the bench's batches (one starting a row, one in mid-row); mid-row starts; batches ending
# on the last pixel of an 800 x 800 and a 1920 x 1440 image; batches shorter than a row (at row 0 and in mid-row); sizes
# that are no multiple of 2 048; odd widths (a last column outside the 2 x 2 blocks), down to a one-pixel-wide image.
# Every batch below 2 048 rays fills fewer pairs than the device has (a grid of fewer than 256 workgroups).
SHAPES = [
    (800, 0, 65536), (800, 65536, 65536), (800, 777, 3000), (800, 800 * 800 - 5001, 5001), (800, 160, 1600),
    (1920, 0, 1000), (1920, 7 * 1920 + 13, 100), (1920, 1920 * 1440 - 70001, 70001), (1920, 1919, 3842),
    (801, 3, 4097), (801, 5 * 801 - 1, 2), (37, 5, 700), (3, 1, 50), (1, 0, 9), (2, 1, 7),
]


@pytest.mark.parametrize("mode", ["split_bf16", "f16"])
@pytest.mark.parametrize("width,start,R", SHAPES)
def test_team_schedule_hint_renders_every_ray_once_bit_identically(ops, setup, monkeypatch, mode, width, start, R):
    from cropnerf_amd import _lib as L

    monkeypatch.setenv("CN_FUSED_SPLIT", "2")  # the producer/consumer kernel at every batch size
    mp = {"split_bf16": L.MATRIX_SPLIT_BF16, "f16": L.MATRIX_F16}[mode]
    scene, fh, rb = setup
    g = torch.Generator().manual_seed(width * 7919 + start + R)
    idx = torch.randint(0, len(rb), (R,), generator=g)
    o, d, n, f = (to_dev(t[idx]) for t in (rb.origins, rb.directions, rb.nears, rb.fars))
    sc = ops.scene_struct(scene.aabb, True)
    base = _render_poisoned(ops, fh, sc, ops.render_opts(S, matrix_precision=mp), o, d, n, f)
    hinted = _render_poisoned(ops, fh, sc, ops.render_opts(S, matrix_precision=mp, image_width=width, pixel_start=start),
                              o, d, n, f)
    for k in OUTS:
        assert not torch.isnan(base[k]).any(), f"{k}: rays never written without the hint"
        assert not torch.isnan(hinted[k]).any(), f"{k}: rays never written under the striped schedule"
        assert torch.equal(base[k], hinted[k]), k
