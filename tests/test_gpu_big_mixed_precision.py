"""The reference's mixed-precision training class on the ``fruit_nerf_method_big`` / ``_huge`` field shape (geo 30, 3 x 128
semantic layers; ``fruit_nerf_config.py:66-172``, ``mixed_precision=True`` in all three specifications): the fp16 forward
``cn_field_eval_f16``, the mixed-precision general backward ``cn_field_backward_general_mp(..., CN_MATRIX_F16)``, and the
trainer's generic path under ``matrix_precision="f16"``.

Oracle: ``oracle/tcnn.py`` with ``tcnn_half_activations=True`` -- fp16 parameters, every encoding accumulation and layer input
rounded to fp16, the rounding a straight-through step under autograd.  Bars are those of the default shape's mixed-precision
test (``test_gpu_tcnn.py``): relative L2 2e-2 per field tensor, losses 2e-3.
"""

import dataclasses

import pytest
import torch

from _helpers import Scene, to_dev
from oracle import field as OF
from oracle import losses as OL
from oracle import rays as ORY
from oracle import samplers as OSM
from oracle import tcnn as TC

pytestmark = pytest.mark.gpu

N_IMG = 5
DIMS = {"field.mlp_base_mlp": (32, 31, 64, 1), "field.mlp_semantics": (30, 64, 128, 2), "field.mlp_head": (16 + 30 + 32, 3, 64, 2)}


def _half_values(state):
    # masters that are fp16 values already (as a checkpoint of the reference holds them): the oracle's fp16 parameter copy is the
    # master itself, and what is compared is the arithmetic, not a second rounding of the parameters
    return {k: (v.to(torch.float16).to(torch.float32) if k.endswith("tcnn_encoding.params") else v) for k, v in state.items()}


def _field_setup(max_res, R=41, S=13):
    """The field of test_gpu_tcnn.py::test_big_shapes_in_the_tcnn_layout_forward_and_backward, with fp16-valued masters."""
    from cropnerf_amd import config as PC
    from cropnerf_amd import ops as O
    from cropnerf_amd.fruit_nerf import tcnn_params as TP
    from _helpers import make_scene

    ospec = OF.FieldSpec(grid=OF.GridSpec(16, 16, max_res, 12, 2), geo_feat_dim=30, num_layers_semantic=3,
                         hidden_dim_semantics=128, num_images=N_IMG, implementation="tcnn")
    state = {k: v for k, v in TC.random_params(ospec, [], seed=22, grid_scale=0.1).items() if k.startswith("field.")}
    state["field.mlp_head.tcnn_encoding.params"] = state["field.mlp_head.tcnn_encoding.params"] * 4.0
    state = _half_values(state)
    pspec = PC.FieldSpec(grid=PC.GridSpec(16, 16, max_res, 12, 2, "tcnn"), geo_feat_dim=30, num_layers_semantic=3,
                         hidden_dim_semantics=128, num_images=N_IMG)
    sc = make_scene(seed=2, log2_T=12, num_images=N_IMG, height=12, width=12, focal=16.0, prop_log2_T=10)
    rb = ORY.with_aabb_near_far(ORY.image_rays(sc.c2w, sc.intr, 1, 12, 12), sc.aabb.reshape(-1)).slice(0, R)
    g = torch.Generator().manual_seed(4)
    cam = torch.randint(0, N_IMG, (R, 1), generator=g)
    rs = OSM.spaced_sampler(rb, S, "uniform")
    up = (torch.randn(R, S, generator=g), torch.randn(R, S, 3, generator=g), torch.randn(R, S, generator=g))
    full = dict(state)
    full["camera_optimizer.pose_adjustment"] = torch.zeros(N_IMG, 6)
    dp = TP.from_tcnn_state_dict(full, pspec, [], "cuda", torch.float32)
    fh = O.FieldHandle(dp, pspec)
    return dict(ospec=ospec, state=state, pspec=pspec, sc=sc, rb=rb, cam=cam, rs=rs, up=up, dp=dp, fh=fh,
                scene=O.scene_struct(sc.aabb, True))


def _dev_args(f):
    return (to_dev(f["rb"].origins), to_dev(f["rb"].directions), to_dev(f["cam"][:, 0]), to_dev(f["rs"].starts[..., 0]),
            to_dev(f["rs"].ends[..., 0]))


def _tcnn_grads(f, grads):
    """The product's gradient dict as gradients of tcnn's own parameter vectors (alias entries folded, frozen biases dropped)."""
    from cropnerf_amd import ops as O
    from cropnerf_amd.fruit_nerf import tcnn_params as TP

    O.tcnn_grid_tie_gradients(f["pspec"].grid, grads["field.mlp_base_grid.hash_table"])
    for name in TP.frozen_parameter_names(f["pspec"], []):
        grads[name].zero_()
    return {k: v.detach().cpu() for k, v in TP.to_tcnn_state_dict(grads, f["pspec"], []).items()}


def _rel(a, b, k):
    """Relative L2 of what is a free parameter on both sides (the padded input columns of tcnn's first matrix apart)."""
    if k[: -len(".tcnn_encoding.params")] in DIMS:
        n_in, n_out, width, n_hidden = DIMS[k[: -len(".tcnn_encoding.params")]]
        ma, mb = TC.mlp_matrices(a, n_in, n_out, width, n_hidden), TC.mlp_matrices(b, n_in, n_out, width, n_hidden)
        ma[0], mb[0] = ma[0][:, : n_in + 1], mb[0][:, : n_in + 1]
        a, b = torch.cat([m.reshape(-1) for m in ma]), torch.cat([m.reshape(-1) for m in mb])
    return float((a - b).norm() / (b.norm() + 1e-12))


def _backward(f, up, matrix_precision):
    from cropnerf_amd import _lib as L
    from cropnerf_amd import ops as O

    grads = {k: torch.zeros_like(v) for k, v in f["dp"].items()}
    O.field_backward_general(f["fh"], O.FieldHandle(grads, f["pspec"]), f["scene"], *_dev_args(f), *(to_dev(u) for u in up),
                             app_mode=L.APP_PER_CAMERA, matrix_precision=matrix_precision)
    torch.cuda.synchronize()
    return _tcnn_grads(f, grads)


@pytest.mark.parametrize("max_res", [4096, 8192])
def test_fp16_forward_and_mixed_backward_against_the_half_activation_oracle(max_res):
    """``cn_field_eval_f16`` against the half-activation oracle's forward, and ``cn_field_backward_general_mp(F16)`` against its
    autograd gradients (measured forward: density 3e-6, rgb 2e-4, semantics 1.7e-3).  The fp32 kernel differentiates the
    unrounded forward: where the two functions' gates differ, the mixed table gradient must follow the rounded one."""
    from cropnerf_amd import _lib as L
    from cropnerf_amd import ops as O

    f = _field_setup(max_res)
    ospec_h = dataclasses.replace(f["ospec"], tcnn_half_activations=True)
    rb, cam, rs, sc, state = f["rb"], f["cam"], f["rs"], f["sc"], f["state"]
    R, S = rs.starts.shape[:2]
    pos = rs.positions()
    # ---- forward -----------------------------------------------------------------------------------------------------------
    with torch.no_grad():
        fo = OF.field_forward(pos, rb.directions, cam, state, ospec_h, sc.aabb, True, "val", training=True)
        geo = OF.field_density(pos, state, ospec_h, sc.aabb, True)[1]
        sem = OF.semantics_from_geo(geo.reshape(-1, 30), state, ospec_h).view(R, S)
    out = O.field_eval_f16(f["fh"], f["scene"], *_dev_args(f), app_mode=L.APP_PER_CAMERA)
    torch.cuda.synchronize()
    fwd = {"density": (out["density"], fo["density"][..., 0]), "rgb": (out["rgb"], fo["rgb"]),
           "semantics": (out["semantics"], sem)}
    errs = {k: float((a.cpu() - b).norm() / b.norm()) for k, (a, b) in fwd.items()}
    print(f"max_res {max_res}: fp16 forward vs half-activation oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < 2e-2 for v in errs.values()), errs
    # the fp16 forward is not the split-bf16 / fp32 one: it rounds where the oracle rounds
    ex = O.field_eval(f["fh"], f["scene"], *_dev_args(f), app_mode=L.APP_PER_CAMERA)
    assert not torch.equal(ex["rgb"], out["rgb"])
    # ---- backward ----------------------------------------------------------------------------------------------------------
    # Every hidden pre-activation of the half-activation forward (base, semantic and colour MLPs)
    pre, relu = [], torch.relu
    TC.torch.relu = lambda t: (pre.append(t.detach()), relu(t))[1]
    try:
        with torch.no_grad():
            OF.field_forward(pos, rb.directions, cam, state, ospec_h, sc.aabb, True, "val", training=True)
    finally:
        TC.torch.relu = relu
    assert len(pre) == 5 and all(t.shape[0] == R * S for t in pre)  # base 1, semantics 2, colour 2 hidden layers
    margin = [t.abs().min(dim=1).values / t.abs().max() for t in pre]

    def compare(keep, what):
        kept = float(keep.float().mean())
        gd, grgb, gsem = f["up"]
        up = (gd * keep, grgb * keep[..., None], gsem * keep)
        p = {k: v.clone().requires_grad_(True) for k, v in state.items()}
        fo = OF.field_forward(pos, rb.directions, cam, p, ospec_h, sc.aabb, True, "val", training=True)
        geo = OF.field_density(pos, p, ospec_h, sc.aabb, True)[1].detach()
        sem = OF.semantics_from_geo(geo.reshape(-1, 30), p, ospec_h).view(R, S)
        ((fo["density"][..., 0] * up[0]).sum() + (fo["rgb"] * up[1]).sum() + (sem * up[2]).sum()).backward()
        assert all(v.grad.abs().sum() > 0 for v in p.values())
        g16, g32 = _backward(f, up, L.MATRIX_F16), _backward(f, up, L.MATRIX_FP32)
        mixed = {k: _rel(g16[k], v.grad, k) for k, v in p.items()}
        exact = {k: _rel(g32[k], v.grad, k) for k, v in p.items()}
        print(f"max_res {max_res}, {what} ({100 * kept:.1f} % of the samples):")
        print("  mixed backward vs half-activation oracle:", {k: f"{v:.2e}" for k, v in mixed.items()})
        print("  fp32 backward vs half-activation oracle: ", {k: f"{v:.2e}" for k, v in exact.items()})
        return kept, mixed, exact

    # Parity.  A sample with any hidden pre-activation within a few fp16 ulps of zero has a ReLU gate that the order of the
    # sums decides (one flipped gate moves a gradient tensor by up to 1e-2 of its norm): those get no upstream gradient.
    # Measured: at most 1.1e-2 (the table at 4096, the semantic MLP at 8192) with ~80 % of the samples kept.
    kept, mixed, _ = compare((torch.stack(margin).min(dim=0).values > 2e-4).view(R, S), "every near-zero gate masked")
    assert 0.7 < kept < 1.0, kept
    assert len(mixed) >= 7
    bad = {k: v for k, v in mixed.items() if v > 2e-2}
    assert not bad, f"mixed-precision gradients vs the half-activation oracle: {bad}"
    # Not noise on fp32.  Masking only the base MLP's gates (those the position arithmetic decides at these resolutions, as the
    # fp32 test of this shape does) leaves the semantic and colour gates that fp16 rounding decides: the mixed kernel rounds
    # where the oracle rounds and follows them, the fp32 kernel does not.  At max_res 8192 that puts the mixed table gradient
    # four times closer to the oracle (measured 3.7e-3 against 1.5e-2); at 4096 the gates this seed leaves near zero barely
    # reach the table (fp32: 8e-4) and the bf16 products' own 4e-3 dominate, so there it is reported, not asserted.
    _, mixed, exact = compare((margin[0] > 5e-4).view(R, S), "base-MLP gates masked")
    grid = "field.mlp_base_grid.tcnn_encoding.params"
    if max_res == 8192:
        assert mixed[grid] < 0.5 * exact[grid], "the mixed table gradient is no closer to the rounded function's than fp32's"


def test_fp32_through_the_mp_entry_is_the_ex_entry_bit_for_bit(monkeypatch):
    """``cn_field_backward_general_mp(..., CN_MATRIX_FP32)`` and ``(CN_MATRIX_SPLIT_BF16)`` run today's kernel: under
    ``CN_DETERMINISTIC_SCATTER=1`` (order-free accumulation) they equal ``cn_field_backward_general_ex`` bit for bit."""
    import ctypes as C

    from cropnerf_amd import _lib as L
    from cropnerf_amd import ops as O

    monkeypatch.setenv("CN_DETERMINISTIC_SCATTER", "1")
    lib = L.load()
    assert lib.cn_deterministic_build() == 1
    f = _field_setup(4096)
    args = _dev_args(f)
    up = tuple(to_dev(u) for u in f["up"])
    R, S = f["rs"].starts.shape[:2]
    ws = torch.empty(lib.cn_field_backward_general_workspace_bytes(C.byref(f["fh"].struct)), dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def run(call):
        # one flat buffer behind every gradient tensor: one registered range
        flat = torch.zeros(sum(v.numel() for v in f["dp"].values()), device="cuda")
        grads, off = {}, 0
        for k, v in f["dp"].items():
            grads[k] = flat[off:off + v.numel()].view_as(v)
            off += v.numel()
        O.deterministic_register([flat], owner=flat)
        gh = O.FieldHandle(grads, f["pspec"])
        head = (C.byref(f["fh"].struct), C.byref(gh.struct), C.byref(f["scene"]), L.APP_PER_CAMERA, 1, None,
                *(ptr(a) for a in args), *(ptr(u) for u in up), R, S, None, None, 0)
        L.check(call(head))
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in grads.items()}

    ref = run(lambda h: lib.cn_field_backward_general_ex(*h, ptr(ws), ws.numel(), None))
    for mode in (L.MATRIX_FP32, L.MATRIX_SPLIT_BF16):
        got = run(lambda h: lib.cn_field_backward_general_mp(*h, mode, ptr(ws), ws.numel(), None))
        for k in ref:
            assert torch.equal(got[k], ref[k]), (mode, k)
    assert float(ref["field.mlp_base_grid.hash_table"].abs().sum()) > 0


def test_unknown_matrix_precision_and_unsupported_shapes_are_refused():
    from cropnerf_amd import _lib as L
    from cropnerf_amd import config as PC
    from cropnerf_amd import ops as O
    from cropnerf_amd import synthetic

    f = _field_setup(4096, R=4, S=3)
    up = f["up"]
    for bad in (3, -1):
        with pytest.raises(L.CropNerfHipError) as e:
            _backward(f, up, bad)
        assert e.value.code == L.CN_ERR_INVALID
    # a generic shape the backward takes but the fp16 forward is not built for
    spec = PC.FieldSpec(grid=PC.GridSpec(16, 16, 2048, 12, 2), geo_feat_dim=20, num_layers_semantic=3, hidden_dim_semantics=96,
                        num_images=N_IMG)
    assert not O.field_eval_f16_supported(spec) and O.field_eval_f16_supported(f["pspec"])
    fh = O.FieldHandle(synthetic.p_rand(spec, [], seed=1, device="cuda"), spec)
    with pytest.raises(L.CropNerfHipError) as e:
        O.field_eval_f16(fh, f["scene"], *_dev_args(f), app_mode=L.APP_PER_CAMERA)
    assert e.value.code == L.CN_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the trainer
S_PROP, S_FINAL = (64, 32), 16


def _big_tcnn_scene(seed, max_res=2048, log2_T=12):
    from cropnerf_amd import synthetic

    fspec = OF.FieldSpec(grid=OF.GridSpec(16, 16, max_res, log2_T, 2), geo_feat_dim=30, num_layers_semantic=3,
                         hidden_dim_semantics=128, num_images=4, implementation="tcnn")
    pspecs = [OF.ProposalSpec(OF.GridSpec(5, 16, 128, 10), implementation="tcnn"),
              OF.ProposalSpec(OF.GridSpec(5, 16, 256, 10), implementation="tcnn")]
    params = TC.random_params(fspec, pspecs, seed=seed, grid_scale=0.1)
    params["field.mlp_head.tcnn_encoding.params"] = params["field.mlp_head.tcnn_encoding.params"] * 4.0
    params = _half_values(params)
    g = torch.Generator().manual_seed(seed + 99)
    params["camera_optimizer.pose_adjustment"] = (torch.rand(4, 6, generator=g) - 0.5) * 0.02
    c2w, intr = synthetic.orbit_cameras(4, height=20, width=20, focal=28.0)
    return Scene(params, fspec, pspecs, torch.tensor(synthetic.SCENE_AABB, dtype=torch.float32), c2w, intr, 20, 20)


def _batch(seed, R=128):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randint(0, 4, (R,), generator=g), torch.randint(0, 20, (R,), generator=g),
                       torch.randint(0, 20, (R,), generator=g)], -1)
    jitter = [torch.rand(R, 1, generator=g) for _ in range(3)]
    return idx, jitter, torch.rand(R, 3, generator=g), (torch.rand(R, 1, generator=g) > 0.5).float()


def _big_model(sc, mode):
    from cropnerf_amd.config import FruitNerfModelConfig
    from cropnerf_amd.fruit_nerf import tcnn_params
    from cropnerf_amd.fruit_nerf.fruit_nerf import FruitModel, Semantics
    from cropnerf_amd.rays import SceneBox
    from _helpers import product_specs

    pl = [{"hidden_dim": 16, "log2_hashmap_size": p.grid.log2_hashmap_size, "num_levels": 5, "max_res": p.grid.max_res}
          for p in sc.pspecs]
    g = sc.fspec.grid
    cfg = FruitNerfModelConfig(geo_feat_dim=30, num_layers_semantic=3, hidden_dim_semantics=128, max_res=g.max_res,
                               log2_hashmap_size=g.log2_hashmap_size, proposal_net_args_list=pl,
                               num_proposal_samples_per_ray=S_PROP, num_nerf_samples_per_ray=S_FINAL, implementation="tcnn",
                               matrix_precision=mode)
    fspec, pspecs = product_specs(sc)
    params = tcnn_params.from_tcnn_state_dict(sc.params, fspec, pspecs, "cuda", torch.float32)
    model = FruitModel(cfg, SceneBox(sc.aabb), num_train_data=sc.c2w.shape[0], metadata={"semantics": Semantics()},
                       device="cuda", test_mode="val", params=params)
    model.training = True
    return model


def _rays(sc, idx):
    from cropnerf_amd.rays import Cameras

    cams = Cameras(sc.c2w, sc.intr[:, 0], sc.intr[:, 1], sc.intr[:, 2], sc.intr[:, 3], sc.height, sc.width).to("cuda")
    return cams.generate_rays(idx.cuda())


def test_trainer_runs_the_big_shape_in_the_mixed_precision_class():
    """A _big-shaped tcnn model with ``matrix_precision="f16"``: the trainer takes the generic path in the mixed class, its losses
    are the half-activation oracle's within 2e-3 and its field gradients within 2e-2; the table gradient is closer to the
    oracle's than the fp32 iteration's is."""
    from cropnerf_amd import _lib as L
    from cropnerf_amd import ops as O
    from cropnerf_amd.fruit_nerf import tcnn_params as TP
    from cropnerf_amd.fruit_nerf.trainer import FruitTrainer

    sc = _big_tcnn_scene(seed=7)
    idx, jitter, image, mask = _batch(7)
    half_f = dataclasses.replace(sc.fspec, tcnn_half_activations=True)
    params = {k: v.clone().requires_grad_(True) for k, v in sc.params.items()}
    rb = ORY.pinhole_rays(sc.c2w, sc.intr, idx[:, 0], idx[:, 1], idx[:, 2])
    out_ref = OL.train_forward(rb, params, half_f, sc.pspecs, sc.aabb, S_PROP, S_FINAL, jitter)
    ld = OL.loss_dict(out_ref, image, mask)
    ld["camera_opt_regularizer"] = OL.camera_opt_regularizer(params["camera_optimizer.pose_adjustment"])
    sum(ld.values()).backward()

    def run(mode):
        model = _big_model(sc, mode)
        tr = FruitTrainer(model)
        assert tr.general
        assert model.train_matrix_precision() == (L.MATRIX_F16 if mode == "f16" else L.MATRIX_FP32)
        out = tr.forward_backward(_rays(sc, idx), {"image": image, "fruit_mask": mask}, jitter=jitter)
        for spec, key in tr._tcnn_tables:
            O.tcnn_grid_tie_gradients(spec, tr.grads[key])
        for name in tr._frozen:
            tr.grads[name].zero_()
        got = TP.to_tcnn_state_dict({k: v for k, v in tr.grads.items()}, model.field_spec, model.proposal_specs)
        return out, {k: v.detach().cpu() for k, v in got.items()}

    out16, g16 = run("f16")
    out32, g32 = run("fp32")
    for k, v in ld.items():
        ref = float(v.detach())
        assert abs(float(out16["loss_dict"][k]) - ref) <= 2e-3 * abs(ref) + 1e-7, (k, float(out16["loss_dict"][k]), ref)
    vs_oracle = {k: _rel(g16[k], p.grad, k) for k, p in params.items() if p.grad is not None}
    fp32_vs_oracle = {k: _rel(g32[k], p.grad, k) for k, p in params.items() if p.grad is not None}
    print("trainer, mixed vs half-activation oracle:", {k: f"{v:.2e}" for k, v in vs_oracle.items()})
    print("trainer, fp32 vs half-activation oracle: ", {k: f"{v:.2e}" for k, v in fp32_vs_oracle.items()})
    field = [k for k in vs_oracle if k.startswith("field.")]
    assert len(field) >= 5
    bad = {k: v for k, v in vs_oracle.items() if v > (2e-2 if k.startswith("field.") else 3e-2)}
    assert not bad, f"mixed-precision gradients vs the half-activation oracle: {bad}"



def test_big_shape_mixed_training_reduces_the_loss_like_fp32():
    """Twelve Adam steps on one batch in both modes: the mixed run's loss falls and stays within 3 % of the fp32 run's."""
    from cropnerf_amd.fruit_nerf.trainer import FruitTrainer

    sc = _big_tcnn_scene(seed=3)
    idx, jitter, image, mask = _batch(3)
    rays = _rays(sc, idx)
    losses = {}
    for mode in ("fp32", "f16"):
        tr = FruitTrainer(_big_model(sc, mode))
        hist = []
        for _ in range(12):
            out = tr.forward_backward(rays, {"image": image, "fruit_mask": mask}, jitter=jitter)
            hist.append(sum(float(v) for v in out["loss_dict"].values()))
            tr.optimizer_step()
        losses[mode] = hist
    print("losses:", losses)
    assert losses["f16"][-1] < 0.9 * losses["f16"][0], losses
    for a, b in zip(losses["f16"], losses["fp32"]):
        assert abs(a - b) <= 0.03 * abs(b) + 1e-4, losses


def test_huge_configured_mixed_iteration_is_finite():
    """One iteration of a model built from the fruit_nerf_method_huge specification (2^21-entry levels, max_res 8192, a 7-level
    second proposal network) with ``matrix_precision="f16"``: the generic mixed path runs and every loss and gradient is finite."""
    from cropnerf_amd import _lib as L
    from cropnerf_amd import synthetic
    from cropnerf_amd.fruit_nerf import fruit_nerf_config as FC
    from cropnerf_amd.fruit_nerf.fruit_nerf import FruitModel, Semantics
    from cropnerf_amd.fruit_nerf.trainer import FruitTrainer
    from cropnerf_amd.rays import Cameras, SceneBox

    cfg = dataclasses.replace(FC.native_method("fruit_nerf_huge").config.pipeline.model, matrix_precision="f16")
    c2w, intr = synthetic.orbit_cameras(4, height=64, width=64)
    aabb = SceneBox(torch.tensor(synthetic.SCENE_AABB))
    model = FruitModel(cfg, aabb, 4, {"semantics": Semantics()}, device="cuda", test_mode="val")
    for k, v in model.params.items():
        if k.endswith("hash_table"):
            v.mul_(100.0)  # the 1e-3 init is an empty volume
    model.training = True
    tr = FruitTrainer(model)
    assert tr.general and model.train_matrix_precision() == L.MATRIX_F16
    g = torch.Generator().manual_seed(1)
    R = 512
    idx = torch.stack([torch.randint(0, 4, (R,), generator=g), torch.randint(0, 64, (R,), generator=g),
                       torch.randint(0, 64, (R,), generator=g)], -1)
    rays = Cameras(c2w, intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 64, 64).to("cuda").generate_rays(idx.cuda())
    batch = {"image": torch.rand(R, 3, generator=g), "fruit_mask": (torch.rand(R, 1, generator=g) > 0.5).float()}
    out = tr.forward_backward(rays, batch)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in out["loss_dict"].values())
    assert bool(torch.isfinite(tr.flat_grads).all()) and float(tr.flat_grads.abs().sum()) > 0
