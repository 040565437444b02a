"""Split-bf16 matrix mode of render_split_kernel: the 16-wide layers as one K block of 32 that carries hi AND lo.

Semantics layer 0 and colour layer 0 read the 16 base outputs.  Their B operand holds, per lane, hi of the lane's four
values in slots 0-3 and lo in slots 4-7 (render_split.hpp: split_bf16_k16); the weight-image blocks 6...13 repeat a lane's four
weights in slots 4-7 (render_fused.hip: bf16_image_word).  Two products, hi image x operand and lo image x operand, then give
all four hi / lo terms.

The CPU test restates the packing on the host and checks its two properties: the mirrored slots, and the algebra of the two
products.  The GPU tests hold the device's image to that restatement bit for bit, and the render to the bars the project
states for this mode: 5e-5 absolute against the exact-fp32 products of the same kernel and, against
the oracle, the bar of test_gpu_parity.py::test_split_bf16_matrix_option_meets_the_parity_bar (restated below).  Shapes:
70 rays (no multiple of the 8 pairs or of a 4-ray team), 100 samples (partial last chunk), 192, 40 (one chunk whose second
half-step is partly empty), uniform spacing and explicit bins, six cameras' appearance rows, with and without the image hint.
"""

from __future__ import annotations

import pytest
import torch

from _helpers import assert_close, dev_params, make_scene, make_tcnn_scene, product_specs, rays_with_box, to_dev
from oracle import field as OF
from oracle import render as ORD
from oracle import samplers as OSM

# the bars of test_split_bf16_matrix_option_meets_the_parity_bar (tests/test_gpu_parity.py)
RTOL, ATOL, ATOL_SEM, ATOL_W = 2e-4, 2e-5, 5e-5, 1e-6
VS_FP32 = 5e-5  # split-bf16 against exact-fp32 products, absolute

R = 70
WIDTH, START = 40, 13  # the image hint: a partial first row, one full row, a partial last row
BLOCK_BF16 = 2 * 64 * 8  # a weight-image block: [hi | lo][lane 64][8 bf16]


# ---------------------------------------------------------------------------------------------- host restatement
def pack_k16_blocks(ws0: torch.Tensor, wc0: torch.Tensor) -> torch.Tensor:
    """Image blocks 6...13 as prep_kernel writes them: [8 blocks][hi | lo][lane 64][8 slots], bfloat16.  Blocks 0-3 are the
    four row tiles of semantics layer 0 (ws0 [64, 15]), blocks 4-7 those of colour layer 0's geometry columns (wc0 [64, 63],
    columns 16...30).  Lane (g, j) holds row 16 mt + j; slot e < 4 holds base output neuron m = 4 g + e (neuron 0 is the density
    logit: weight 0, neuron m > 0 is geometry feature m - 1), slots 4-7 repeat slots 0-3."""
    out = torch.zeros(8, 2, 64, 8, dtype=torch.bfloat16)
    for b in range(8):
        w = ws0 if b < 4 else wc0[:, 16:31]
        mt = b & 3
        for lane in range(64):
            g, j = lane >> 4, lane & 15
            x = torch.zeros(4, dtype=torch.float32)
            for e in range(4):
                m = 4 * g + e
                if m > 0:
                    x[e] = w[16 * mt + j, m - 1]
            hi = x.to(torch.bfloat16)  # round to nearest even, as the device's conversion
            lo = (x - hi.float()).to(torch.bfloat16)
            out[b, 0, lane] = torch.cat([hi, hi])
            out[b, 1, lane] = torch.cat([lo, lo])
    return out


def pack_k16_operand(o16: torch.Tensor) -> torch.Tensor:
    """The B operand of one column: [lane group 4][8 slots] bfloat16 from the 16 base outputs -- hi of outputs 4 g ... 4 g + 3
    in slots 0-3, lo (bf16 of x - hi) in slots 4-7."""
    x = o16.reshape(4, 4).float()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=1)


def _random_weights(seed):
    g = torch.Generator().manual_seed(seed)
    # magnitudes spread over several binades so that hi and lo parts both matter
    ws0 = torch.randn(64, 15, generator=g) * torch.exp2(torch.randint(-6, 3, (64, 15), generator=g).float())
    wc0 = torch.randn(64, 63, generator=g) * torch.exp2(torch.randint(-6, 3, (64, 63), generator=g).float())
    return ws0, wc0


def test_host_packing_mirrors_the_upper_slots_and_two_products_give_all_four_terms():
    ws0, wc0 = _random_weights(5)
    img = pack_k16_blocks(ws0, wc0)
    assert torch.equal(img[:, 0, :, 4:], img[:, 0, :, :4]), "hi fragment: slots 4-7 mirror slots 0-3"
    assert torch.equal(img[:, 1, :, 4:], img[:, 1, :, :4]), "lo fragment: slots 4-7 mirror slots 0-3"
    assert img[:, :, :16, 0].abs().max() == 0, "base output 0 (the density logit) feeds neither layer"
    g = torch.Generator().manual_seed(6)
    o16 = torch.randn(16, generator=g) * torch.exp2(torch.randint(-4, 4, (16,), generator=g).float())
    b = pack_k16_operand(o16).double()  # [g][slot]
    bh, bl = b[:, :4], b[:, 4:]
    a = img.double().reshape(8, 2, 4, 16, 8)  # [block][hi | lo][g][j][slot]
    ah, al = a[:, 0, :, :, :4], a[:, 1, :, :, :4]
    # what the matrix pipe sums: element j of A times element j of B over the eight slots of the four lane groups
    two = torch.einsum("bgjs,gs->bj", a[:, 0], b) + torch.einsum("bgjs,gs->bj", a[:, 1], b)
    full = torch.einsum("bgjs,gs->bj", ah + al, bh + bl)
    # bf16 x bf16 products are exact in float64; sums of 32 or 64 such terms round at 2^-53 relative each
    scale = torch.einsum("bgjs,gs->bj", (ah.abs() + al.abs()), (bh.abs() + bl.abs()))
    assert ((two - full).abs() <= 64 * 2.0 ** -53 * scale).all()
    # and hi + lo carries the weight / the activation to 2^-16 relative or better (two roundings to 8 significant bits)
    w = torch.cat([torch.cat([torch.zeros(64, 1), ws0], 1), torch.cat([torch.zeros(64, 1), wc0[:, 16:31]], 1)]).double()
    w = w.reshape(8, 16, 4, 4).permute(0, 2, 1, 3)  # [block][g][j][e]
    assert ((ah + al - w).abs() <= 2.0 ** -16 * w.abs()).all()
    assert ((bh + bl - o16.double().reshape(4, 4)).abs() <= 2.0 ** -16 * o16.double().abs().reshape(4, 4)).all()


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from cropnerf_amd import ops as _ops

    return _ops


def _pick_rays(scene, seed):
    """R rays drawn from all cameras' images, each with its camera's appearance row."""
    g = torch.Generator().manual_seed(seed)
    ncam = scene.c2w.shape[0]
    cams = torch.randint(0, ncam, (R,), generator=g)
    assert cams.unique().numel() >= 3
    per_cam = [rays_with_box(scene, c) for c in range(ncam)]
    pix = torch.randint(0, len(per_cam[0]), (R,), generator=g)
    pick = lambda name: torch.stack([getattr(per_cam[int(c)], name)[int(p)] for c, p in zip(cams, pix)])
    return {"origins": pick("origins"), "directions": pick("directions"), "nears": pick("nears"), "fars": pick("fars"),
            "cams": cams}


def _edges(rays, S, bins):
    """[R, S + 1] euclidean bin edges: the uniform sampler's, or explicit ones (a warped, per-ray different spacing)."""
    u = torch.linspace(0.0, 1.0, S + 1)[None, :]
    if bins:
        p = 1.0 + torch.linspace(0.0, 1.0, R)[:, None]  # exponent 1 ... 2
        u = u ** p
    return (rays["nears"] + (rays["fars"] - rays["nears"]) * u).contiguous()


@pytest.fixture(scope="module")
def float_setup(ops):
    scene = make_scene(seed=2, log2_T=15, prop_log2_T=12)
    fspec, _ = product_specs(scene)
    return scene, ops.FieldHandle(dev_params(scene), fspec), _pick_rays(scene, 21)


@pytest.fixture(scope="module")
def half_setup(ops):
    scene = make_tcnn_scene(seed=3, log2_T=15, prop_log2_T=12)
    fspec, _ = product_specs(scene)
    return scene, ops.FieldHandle(dev_params(scene), fspec), _pick_rays(scene, 22)  # tcnn layout, fp16 table


def _render(ops, setup, S, bins, mp, hint, monkeypatch):
    from cropnerf_amd import _lib as L

    monkeypatch.setenv("CN_FUSED_SPLIT", "2")  # the producer/consumer kernel for this small batch
    scene, fh, rays = setup
    kw = {"image_width": WIDTH, "pixel_start": START} if hint else {}
    opts = ops.render_opts(S, app_mode=L.APP_PER_CAMERA, matrix_precision=mp, **kw)
    out = ops.render_rays(fh, ops.scene_struct(scene.aabb, True), opts, to_dev(rays["origins"]), to_dev(rays["directions"]),
                          to_dev(rays["nears"]), to_dev(rays["fars"]), camera_indices=to_dev(rays["cams"]),
                          bins=to_dev(_edges(rays, S, True)) if bins else None, want_weights=True)
    torch.cuda.synchronize()
    return out


def _check_against_fp32(fast, exact, hinted):
    for k, v in fast.items():
        assert torch.isfinite(v).all(), f"{k} not finite"
        assert torch.equal(v, hinted[k]), f"{k}: the image hint changed a bit"
    for k in ("rgb", "accumulation", "semantics"):
        err = float((fast[k] - exact[k]).abs().max())
        print(f"split-bf16 vs fp32 {k}: max abs {err:.3e} (scale {float(exact[k].abs().max()):.3g})")
    for k in ("rgb", "accumulation", "semantics"):
        assert_close(fast[k], exact[k], 0.0, VS_FP32, f"split-bf16 vs fp32 {k}")
    assert not torch.equal(fast["rgb"], exact["rgb"]), "the split-bf16 products were not used"


CASES = [(100, False), (192, False), (40, False), (100, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("S,bins", CASES)
def test_float_table_render_meets_the_fp32_and_oracle_bars(ops, float_setup, monkeypatch, S, bins):
    from cropnerf_amd import _lib as L

    scene, fh, rays = float_setup
    fast = _render(ops, float_setup, S, bins, L.MATRIX_SPLIT_BF16, False, monkeypatch)
    hinted = _render(ops, float_setup, S, bins, L.MATRIX_SPLIT_BF16, True, monkeypatch)
    exact = _render(ops, float_setup, S, bins, L.MATRIX_FP32, False, monkeypatch)
    _check_against_fp32(fast, exact, hinted)
    # the oracle on the same bin edges, per-camera appearance rows (test_render_rays_per_camera_appearance's set-up)
    e = _edges(rays, S, bins)
    starts, ends = e[:, :-1, None], e[:, 1:, None]
    pos = rays["origins"][:, None, :] + rays["directions"][:, None, :] * (starts + ends) / 2
    fo = OF.field_forward(pos, rays["directions"], rays["cams"][:, None], scene.params, scene.fspec, scene.aabb, True,
                          "test", training=True)
    w = OSM.get_weights(ends - starts, fo["density"])
    for k, ref, atol in (("weights", w[..., 0], ATOL_W), ("accumulation", ORD.render_accumulation(w), ATOL),
                         ("rgb", ORD.render_rgb(fo["rgb"], w, "last_sample"), ATOL),
                         ("semantics", ORD.render_semantics(fo["semantics"], w), ATOL_SEM)):
        print(f"split-bf16 vs oracle {k}: max abs {float((fast[k].cpu() - ref).abs().max()):.3e}")
        assert_close(fast[k], ref, RTOL, atol, f"split-bf16 vs oracle {k}")
    ref_depth = ORD.render_depth_median(w, starts, ends)
    ok = (fast["depth"].cpu() - ref_depth).abs() <= 1e-5 + 1e-5 * ref_depth.abs()
    assert ok.float().mean().item() >= 0.995


@pytest.mark.gpu
@pytest.mark.parametrize("S,bins", [(100, False), (40, True)])
def test_half_table_render_meets_the_fp32_bar(ops, half_setup, monkeypatch, S, bins):
    from cropnerf_amd import _lib as L

    fast = _render(ops, half_setup, S, bins, L.MATRIX_SPLIT_BF16, False, monkeypatch)
    hinted = _render(ops, half_setup, S, bins, L.MATRIX_SPLIT_BF16, True, monkeypatch)
    exact = _render(ops, half_setup, S, bins, L.MATRIX_FP32, False, monkeypatch)
    _check_against_fp32(fast, exact, hinted)


@pytest.mark.gpu
def test_per_sample_outputs_meet_the_fp32_bars(ops, float_setup, monkeypatch):
    """cn_render_samples (the exporters' forward) in split-bf16 against its exact-fp32 form: the bars of
    test_split_kernel_per_sample_outputs_match_fused (densities are exp(logit): a relative bar)."""
    from cropnerf_amd import _lib as L

    monkeypatch.setenv("CN_FUSED_SPLIT", "2")
    scene, fh, rays = float_setup
    S = 100
    args = [to_dev(rays[k]) for k in ("origins", "directions", "nears", "fars")]
    sc = ops.scene_struct(scene.aabb, True)
    run = lambda mp: ops.render_samples(fh, sc, ops.render_opts(S, app_mode=L.APP_PER_CAMERA, matrix_precision=mp), *args,
                                        camera_indices=to_dev(rays["cams"]))
    fast, exact = run(L.MATRIX_SPLIT_BF16), run(L.MATRIX_FP32)
    torch.cuda.synchronize()
    for k, v in fast.items():
        assert torch.isfinite(v.float()).all(), f"{k} not finite"
    assert torch.equal(fast["positions"], exact["positions"])
    assert_close(fast["density"], exact["density"], 2e-4, 1e-6, "per-sample density")
    assert_close(fast["rgb"], exact["rgb"], 0.0, VS_FP32, "per-sample rgb")
    assert_close(fast["semantics"], exact["semantics"], 2e-4, 5e-5, "per-sample semantics")
    assert not torch.equal(fast["rgb"], exact["rgb"])


@pytest.mark.gpu
def test_device_image_blocks_match_the_host_packing(ops, float_setup, monkeypatch):
    """Blocks 6...13 of the weight image a split-bf16 cn_render_rays call leaves in its workspace, bit for bit."""
    from cropnerf_amd import _lib as L

    scene, fh, rays = float_setup
    _render(ops, float_setup, 40, False, L.MATRIX_SPLIT_BF16, False, monkeypatch)
    blob = fh.workspace()[: 14 * BLOCK_BF16 * 2].cpu().view(torch.bfloat16).reshape(14, 2, 64, 8)
    want = pack_k16_blocks(scene.params["field.mlp_semantics.layers.0.weight"], scene.params["field.mlp_head.layers.0.weight"])
    assert torch.equal(blob[6:].view(torch.int16), want.view(torch.int16))
    assert torch.equal(blob[6:, :, :, 4:].view(torch.int16), blob[6:, :, :, :4].view(torch.int16))
    assert blob[6:, 1].abs().max() > 0, "the lo fragments carry the weights' low bits"
