"""The pair gathers with ONE parity bit per cell and the floor-free cell (csrc/cn_common.hpp: hash_level_xpair_*,
hash_level_pk_*, hash_cell), the pair-wise bf16 split (csrc/render_split.hpp: split_bf16) and the host-computed step of the
uniform sampler, through the kernels that use them: the four-ray team gather of render_split_kernel in split-bf16 mode on a
torch-layout fp32 table, a tcnn-layout fp32 table and a tcnn-layout fp16 table (dense AND hashed levels in one grid), and
the fp16 matrix mode on the tcnn fp16 table (the packed fp16 blend).

70 rays (no multiple of the 8 pairs or of a 4-ray team), S = 40 (one chunk whose second half-step is partly empty) and 100
(a partial last chunk), uniform spacing, with and without the image hint.  Bars, restated from the project's own tests:
5e-5 absolute against the exact-fp32 products of the same call, rtol 2e-4 / atol 2e-5 (semantics 5e-5, weights 1e-6) against
the oracle (tests/test_gpu_bf16_kpack.py, tests/test_gpu_parity.py); for the fp16 mode the bars of tests/test_gpu_f16.py.

Before anything is rendered the samples' cells are computed on the host from the oracle's positions: on every level both
parities of the x index and both values of row ff's parity bit occur in at least 10 % of the samples, so that neither side
of a select goes untested.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np
import pytest
import torch

from _helpers import assert_close, dev_params, make_scene, make_tcnn_scene, product_specs, rays_with_box, to_dev
from oracle import field as OF
from oracle import render as ORD
from oracle import samplers as OSM

RTOL, ATOL, ATOL_SEM, ATOL_W = 2e-4, 2e-5, 5e-5, 1e-6  # test_split_bf16_matrix_option_meets_the_parity_bar
VS_FP32 = 5e-5  # split-bf16 against exact-fp32 products, absolute
R = 70
WIDTH, START = 40, 13  # the image hint: a partial first row, one full row, a partial last row
CONTRACTION = True
MIN_SHARE = 0.10
CN_P1, CN_P2 = 2654435761, 805459861


def _pick_rays(scene, seed):
    """R rays drawn from all cameras' images, each with its camera's appearance row."""
    g = torch.Generator().manual_seed(seed)
    ncam = scene.c2w.shape[0]
    cams = torch.randint(0, ncam, (R,), generator=g)
    per_cam = [rays_with_box(scene, c) for c in range(ncam)]
    pix = torch.randint(0, len(per_cam[0]), (R,), generator=g)
    pick = lambda name: torch.stack([getattr(per_cam[int(c)], name)[int(p)] for c, p in zip(cams, pix)])
    return {"origins": pick("origins"), "directions": pick("directions"), "nears": pick("nears"), "fars": pick("fars"),
            "cams": cams}


def _edges(rays, S):
    u = torch.linspace(0.0, 1.0, S + 1)[None, :]
    return (rays["nears"] + (rays["fars"] - rays["nears"]) * u).contiguous()


def _positions(rays, S):
    e = _edges(rays, S)
    starts, ends = e[:, :-1, None], e[:, 1:, None]
    return rays["origins"][:, None, :] + rays["directions"][:, None, :] * (starts + ends) / 2, starts, ends


def _level_records(fspec):
    """(scale, pos_offset, m1, m2) per level, as make_grid_dev fills them."""
    g = fspec.grid
    if g.layout == "tcnn":
        plan = g.plan()
        bits = [int(plan.level_bits[l]) for l in range(g.num_levels)]
        assert any(b > 0 for b in bits) and any(b == 0 for b in bits), "dense and hashed levels in one grid"
        return [(s, 0.5, (1 << b) if b else CN_P1, (1 << (2 * b)) if b else CN_P2) for s, b in zip(g.scalings(), bits)]
    return [(s, 0.0, CN_P1, CN_P2) for s in g.scalings()]


def parity_shares(scene, fspec, rays, S):
    """Per level: the share of the samples with an odd x index, and with row ff's parity bit set."""
    pos, _, _ = _positions(rays, S)
    p, _ = OF.normalized_positions(pos, scene.aabb, CONTRACTION)
    p = p.reshape(-1, 3).numpy().astype(np.float64)
    out = []
    for scale, off, m1, m2 in _level_records(fspec):
        x = (p * np.float64(np.float32(scale)) + off).astype(np.float32)  # fmaf(p, scale, pos_offset)
        i = np.floor(x).astype(np.uint64)
        row0 = (i[:, 0] ^ ((i[:, 1] * (m1 & 0xFFFFFF)) & 0xFFFFFFFF) ^ ((i[:, 2] * (m2 & 0xFFFFFF)) & 0xFFFFFFFF)) & 1
        out.append((float((i[:, 0] & 1).mean()), float(row0.mean())))
    return out


def _assert_both_branches_are_exercised(scene, fspec, rays, S, what):
    for l, (odd, second) in enumerate(parity_shares(scene, fspec, rays, S)):
        for name, share in (("odd x index", odd), ("row ff parity bit", second)):
            assert MIN_SHARE <= share <= 1.0 - MIN_SHARE, f"{what}, S = {S}, level {l}: {name} in {share:.1%} of the samples"


def _fp16_values(scene):
    """The scene with every tcnn parameter vector rounded to fp16 values: what the oracle's tcnn modules compute with, so
    that a FLOAT table packed from them holds the oracle's numbers."""
    params = {k: (v.to(torch.float16).to(torch.float32) if k.endswith("tcnn_encoding.params") else v)
              for k, v in scene.params.items()}
    return dataclasses.replace(scene, params=params)


def _make(kind):
    if kind == "torch_f32":
        scene, dtype = make_scene(seed=2, log2_T=15, prop_log2_T=12), None
    else:
        scene = _fp16_values(make_tcnn_scene(seed=3, log2_T=15, prop_log2_T=12))
        dtype = torch.float32 if kind == "tcnn_f32" else torch.float16
    return scene, dtype


KINDS = ["torch_f32", "tcnn_f32", "tcnn_f16"]
SAMPLES = [40, 100]


@pytest.mark.parametrize("kind", KINDS)
def test_chosen_rays_exercise_both_sides_of_every_select(kind):
    """The coverage condition itself needs no GPU: it is checked here for all cases, and again in front of each render."""
    scene, _ = _make(kind)
    fspec, _ = product_specs(scene)
    rays = _pick_rays(scene, 21)
    for S in SAMPLES:
        _assert_both_branches_are_exercised(scene, fspec, rays, S, kind)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from cropnerf_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def setups(ops):
    cache = {}

    def get(kind):
        if kind not in cache:
            scene, dtype = _make(kind)
            fspec, _ = product_specs(scene)
            dp = dev_params(scene, table_dtype=dtype) if dtype is not None else dev_params(scene)
            table = dp["field.mlp_base_grid.hash_table"]
            assert table.dtype == (torch.float16 if kind == "tcnn_f16" else torch.float32)
            cache[kind] = (scene, fspec, ops.FieldHandle(dp, fspec), _pick_rays(scene, 21), {})
        return cache[kind]

    return get


def _oracle(setup, S, half_activations=False, per_camera=True):
    """Rendered reference on the uniform bin edges, computed once per (scene, S, arithmetic) and shared."""
    scene, _, _, rays, refs = setup
    key = (S, half_activations, per_camera)
    if key not in refs:
        pos, starts, ends = _positions(rays, S)
        spec = dataclasses.replace(scene.fspec, tcnn_half_activations=True) if half_activations else scene.fspec
        if per_camera:
            fo = OF.field_forward(pos, rays["directions"], rays["cams"][:, None], scene.params, spec, scene.aabb, CONTRACTION,
                                  "test", training=True)
        else:
            fo = OF.field_forward(pos, rays["directions"], None, scene.params, spec, scene.aabb, CONTRACTION, "inference")
        w = OSM.get_weights(ends - starts, fo["density"])
        refs[key] = {"weights": w[..., 0], "accumulation": ORD.render_accumulation(w),
                     "rgb": ORD.render_rgb(fo["rgb"], w, "last_sample"), "semantics": ORD.render_semantics(fo["semantics"], w),
                     "depth": ORD.render_depth_median(w, starts, ends)}
    return refs[key]


def _render(ops, setup, S, mp, hint, monkeypatch, per_camera=True):
    from cropnerf_amd import _lib as L

    monkeypatch.setenv("CN_FUSED_SPLIT", "2")  # the producer/consumer kernel for this small batch
    scene, _, fh, rays, _ = setup
    kw = {"image_width": WIDTH, "pixel_start": START} if hint else {}
    if per_camera:
        kw["app_mode"] = L.APP_PER_CAMERA
    out = ops.render_rays(fh, ops.scene_struct(scene.aabb, CONTRACTION), ops.render_opts(S, matrix_precision=mp, **kw),
                          to_dev(rays["origins"]), to_dev(rays["directions"]), to_dev(rays["nears"]), to_dev(rays["fars"]),
                          camera_indices=to_dev(rays["cams"]) if per_camera else None, want_weights=True)
    torch.cuda.synchronize()
    return out


def _depth_ok(depth, ref_depth):
    ok = (depth.cpu() - ref_depth).abs() <= 1e-5 + 1e-5 * ref_depth.abs()
    return ok.float().mean().item() >= 0.995


@pytest.mark.gpu
@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("kind", KINDS)
def test_split_bf16_team_gather_meets_the_fp32_and_oracle_bars(ops, setups, monkeypatch, kind, S):
    from cropnerf_amd import _lib as L

    setup = setups(kind)
    scene, fspec, _, rays, _ = setup
    _assert_both_branches_are_exercised(scene, fspec, rays, S, kind)
    fast = _render(ops, setup, S, L.MATRIX_SPLIT_BF16, False, monkeypatch)
    hinted = _render(ops, setup, S, L.MATRIX_SPLIT_BF16, True, monkeypatch)
    exact = _render(ops, setup, S, L.MATRIX_FP32, False, monkeypatch)
    for k, v in fast.items():
        assert torch.isfinite(v).all(), f"{k} not finite"
        assert torch.equal(v, hinted[k]), f"{k}: the image hint changed a bit"
    for k in ("rgb", "accumulation", "semantics"):
        print(f"{kind} S={S} split-bf16 vs fp32 {k}: max abs {float((fast[k] - exact[k]).abs().max()):.3e}")
    for k in ("rgb", "accumulation", "semantics"):
        assert_close(fast[k], exact[k], 0.0, VS_FP32, f"split-bf16 vs fp32 {k}")
    assert not torch.equal(fast["rgb"], exact["rgb"]), "the split-bf16 products were not used"
    ref = _oracle(setup, S)
    for k, atol in (("weights", ATOL_W), ("accumulation", ATOL), ("rgb", ATOL), ("semantics", ATOL_SEM)):
        print(f"{kind} S={S} split-bf16 vs oracle {k}: max abs {float((fast[k].cpu() - ref[k]).abs().max()):.3e}")
    for k, atol in (("weights", ATOL_W), ("accumulation", ATOL), ("rgb", ATOL), ("semantics", ATOL_SEM)):
        assert_close(fast[k], ref[k], RTOL, atol, f"split-bf16 vs oracle {k}")
    assert _depth_ok(fast["depth"], ref["depth"])


@pytest.mark.gpu
@pytest.mark.parametrize("S", SAMPLES)
def test_fp16_mode_on_the_tcnn_half_table_meets_its_bars(ops, setups, monkeypatch, S):
    """The packed fp16 blend (hash_level_pk_*) under the bars of tests/test_gpu_f16.py, mean appearance as there."""
    from cropnerf_amd import _lib as L

    setup = setups("tcnn_f16")
    scene, fspec, _, rays, _ = setup
    _assert_both_branches_are_exercised(scene, fspec, rays, S, "tcnn_f16")
    out = _render(ops, setup, S, L.MATRIX_F16, False, monkeypatch, per_camera=False)
    hinted = _render(ops, setup, S, L.MATRIX_F16, True, monkeypatch, per_camera=False)
    exact = _render(ops, setup, S, L.MATRIX_FP32, False, monkeypatch, per_camera=False)
    for k, v in out.items():
        assert torch.isfinite(v).all(), f"{k} not finite"
        assert torch.equal(v, hinted[k]), f"{k}: the image hint changed a bit"
    ref16 = _oracle(setup, S, half_activations=True, per_camera=False)
    ref32 = _oracle(setup, S, half_activations=False, per_camera=False)
    for k in ("rgb", "accumulation", "weights", "semantics"):
        print(f"fp16 mode S={S} vs the half-activation oracle {k}: max abs {float((out[k].cpu() - ref16[k]).abs().max()):.3e}")
    assert_close(out["rgb"], ref16["rgb"], 0.0, 2.5e-4, "rgb vs the half-activation oracle")
    assert_close(out["rgb"], ref32["rgb"], 0.0, 5e-5, "rgb vs the fp32-arithmetic oracle")
    assert_close(out["accumulation"], ref16["accumulation"], 2e-4, 2e-5, "accumulation")
    assert_close(out["weights"], ref16["weights"], 2e-4, 2e-5, "weights")
    assert_close(out["semantics"], ref16["semantics"], 0.0, 5e-5, "semantics")
    assert _depth_ok(out["depth"], ref16["depth"])
    mse = float(((out["rgb"].cpu().float() - exact["rgb"].cpu().float()) ** 2).mean())
    assert -10.0 * math.log10(max(mse, 1e-30)) >= 90.0
    assert not torch.equal(out["rgb"], exact["rgb"])
