"""GPU tests of the BayesRays Hessian stage: ``cn_semantics_density_gradient``, ``cn_field_density_position_gradient``,
``cn_hessian_accumulate`` and ``fruit_nerf/bayesrays.py``'s ``hessian_for_samples`` / ``hessian_for_rays`` / ``compute_hessian``.

References: ``tests/golden/bayesrays_hessian.npz`` (outputs of the reference's own ``find_uncertainty``, made by
``tests/golden/make_golden_bayesrays_hessian.py``), float64 torch autograd over the oracle's weights and field
(``tests/_bayesrays_hessian_ref.py``), and the training backward ``cn_field_backward_ex`` / ``_general`` for the position gradient.

Bars: the float bar 2e-4 / 2e-5 on kernel 1; twice that on the Hessian of given gradients (H is quadratic in
the summed gradient); relative L2 1e-4 between the two device routes to the position gradient (same gather, same cell), 1e-2
against autograd (the bar of ``test_gradients_match_autograd`` for position-derived gradients: a sample within an ulp of a
hash-cell face may land in the neighbouring cell), and twice that, 2e-2, on the end-to-end Hessian.  Every test prints its worst
figure; DESIGN.md section 4.23 records them.
"""

import dataclasses
import os

import numpy as np
import pytest
import torch

import _bayesrays_hessian_ref as REF
from _helpers import dev_params, make_scene, make_tcnn_scene, oracle_model, product_specs, to_dev
from oracle import field as OF
from oracle import rays as ORY
from oracle import samplers as OSM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(lod, c, si) for lod in (3, 4) for c in (0, 1) for si in (0, 1)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "bayesrays_hessian.npz"))


@pytest.fixture(scope="module")
def ops():
    from cropnerf_amd import ops as _ops

    return _ops


def _rel_l2(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


# ------------------------------------------------------------------------------------------------ kernel 3
@pytest.mark.parametrize("lod,c,si", CASES)
def test_hessian_accumulate_meets_the_reference(gold, ops, lod, c, si):
    """The fixture's rays and per-sample gradients in, the reference's Hessian out: every vertex, no sample excluded (a
    coefficient is zero on the far face of a cell, so H is continuous in the positions).  A second call doubles the buffer."""
    dev = lambda k: torch.from_numpy(gold[f"s{si}/{k}"]).cuda().contiguous()
    bins = dev("bins")
    starts, ends = bins[:, :-1].contiguous(), bins[:, 1:].contiguous()
    scene = ops.scene_struct(torch.from_numpy(gold["aabb"]), bool(c))
    ref = torch.from_numpy(gold[f"lod{lod}/c{c}/s{si}/hessian"])
    h = torch.zeros(ref.numel(), device="cuda")
    out = ops.hessian_accumulate(dev("origins"), dev("directions"), starts, ends, dev("gradients"), scene, lod, h)
    assert out is h
    got = h.cpu()
    bar = 4e-4 * ref + 4e-5 * ref.max()
    err = (got - ref).abs()
    print(f"hessian lod {lod} contraction {c} shape {tuple(starts.shape)}: worst error {float((err / bar).max()):.3g} of the bar")
    assert bool((err <= bar).all()), f"{int((err > bar).sum())} of {ref.numel()} vertices outside the bar"
    assert torch.equal(got != 0, ref != 0)
    ops.hessian_accumulate(dev("origins"), dev("directions"), starts, ends, dev("gradients"), scene, lod, h)
    twice = h.cpu()
    assert bool(((twice - 2 * got).abs() <= 1e-5 * got + 1e-6 * got.max()).all())  # float atomics: the order may differ


def test_hessian_accumulate_with_256_samples_per_ray(ops):
    """The largest supported ray (a wave's table then holds 4096 slots, one wave per workgroup) against the torch restatement."""
    g = torch.Generator().manual_seed(5)
    R, S, lod = 9, 256, 5
    o = torch.rand(R, 3, generator=g) * 0.4 - 0.2
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    bins = torch.linspace(0.0, 3.0, S + 1).expand(R, S + 1).contiguous()
    grads = torch.randn(R, S, 3, generator=g)
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    starts, ends = bins[:, :-1].contiguous(), bins[:, 1:].contiguous()
    points = o[:, None, :] + d[:, None, :] * ((starts + ends) / 2)[..., None]
    for c in (False, True):
        ref = REF.hessian_reduction(points.double(), grads.double(), aabb, c, lod).float()
        h = torch.zeros(ref.numel(), device="cuda")
        ops.hessian_accumulate(to_dev(o), to_dev(d), to_dev(starts), to_dev(ends), to_dev(grads), ops.scene_struct(aabb, c), lod, h)
        assert bool(((h.cpu() - ref).abs() <= 4e-4 * ref + 4e-5 * ref.max()).all())


# ------------------------------------------------------------------------------------------------ kernel 1
@pytest.mark.parametrize("S", [5, 48, 96])
def test_semantics_density_gradient_matches_autograd(ops, S):
    """70 rays, S below, inside and beyond one wave's 64 lanes; ray 3 has zero density, ray 5 is saturated."""
    g = torch.Generator().manual_seed(S)
    R = 70
    width = torch.rand(R, S, generator=g) * 0.1 + 0.01
    bins = torch.cat([torch.zeros(R, 1), torch.cumsum(width, -1)], -1) + 0.05
    starts, ends = bins[:, :-1].contiguous(), bins[:, 1:].contiguous()
    density = torch.rand(R, S, generator=g) ** 3 * 30.0
    density[3] = 0.0
    density[5] = 1e4
    sem = torch.randn(R, S, generator=g) * 3.0
    r_total, r_w, r_dd = REF.semantics_density_gradient_autograd(starts, ends, density, sem)
    out = ops.semantics_density_gradient(to_dev(starts), to_dev(ends), to_dev(density), to_dev(sem), want_weights=True)
    total, w, dd = out["semantics"].cpu().double(), out["weights"].cpu().double(), out["d_density"].cpu().double()
    bar = 2e-4 * r_dd.abs() + 2e-5 * r_dd.abs().max()
    print(f"density gradient S {S}: worst error {float(((dd - r_dd).abs() / bar).max()):.3g} of the bar, rendered value "
          f"{float(((total - r_total).abs() / (2e-4 * r_total.abs() + 2e-5)).max()):.3g}")
    assert total.shape == (R, 1) and dd.shape == (R, S)
    assert bool(((total - r_total).abs() <= 2e-4 * r_total.abs() + 2e-5).all())
    assert bool(((w - r_w).abs() <= 2e-4 * r_w.abs() + 2e-5).all())
    assert bool(((dd - r_dd).abs() <= bar).all())
    assert float(total[3]) == 0.0 and float(dd[3].abs().max()) > 0
    plain = ops.semantics_density_gradient(to_dev(starts), to_dev(ends), to_dev(density), to_dev(sem))
    assert "weights" not in plain and plain["d_density"].equal(out["d_density"])


# ------------------------------------------------------------------------------------------------ kernel 2
def _field_case(shape, R=70, S=13):
    """A field of the given shape over make_scene(log2_T=15)'s cameras and box; rays that start outside the box."""
    from cropnerf_amd import config as PC

    kw = {"default": dict(geo_feat_dim=15, num_layers_semantic=2, hidden_dim_semantics=64, max_res=2048),
          "big": dict(geo_feat_dim=30, num_layers_semantic=3, hidden_dim_semantics=128, max_res=4096)}[shape]
    sc = make_scene(seed=2, log2_T=15, num_images=5, height=12, width=12, focal=16.0, prop_log2_T=10)
    ospec = OF.FieldSpec(grid=OF.GridSpec(16, 16, kw["max_res"], 15, 2), geo_feat_dim=kw["geo_feat_dim"],
                         num_layers_semantic=kw["num_layers_semantic"], hidden_dim_semantics=kw["hidden_dim_semantics"],
                         num_images=5)
    params = {k: v for k, v in OF.random_params(ospec, [], seed=21, grid_scale=0.1).items() if k.startswith("field.")}
    pspec = PC.FieldSpec(grid=PC.GridSpec(16, 16, kw["max_res"], 15, 2), geo_feat_dim=kw["geo_feat_dim"],
                         num_layers_semantic=kw["num_layers_semantic"], hidden_dim_semantics=kw["hidden_dim_semantics"],
                         num_images=5)
    rb = ORY.image_rays(sc.c2w, sc.intr, 1, 12, 12).slice(0, R)
    rb = dataclasses.replace(rb, nears=torch.full((R, 1), 0.05), fars=torch.full((R, 1), 6.0))
    rs = OSM.spaced_sampler(rb, S, "uniform")
    g = torch.Generator().manual_seed(4)
    return sc, ospec, pspec, params, rb, rs.starts[..., 0].contiguous(), rs.ends[..., 0].contiguous(), torch.randn(R, S, generator=g)


def _backward_route(ops, fh, pspec, dp, scene, rb, starts, ends, gd, general):
    """The parent commit's only route to the same gradient: the training backward with zero colour / semantic gradients."""
    R, S = starts.shape
    grads = {k: torch.zeros_like(v) for k, v in dp.items()}
    gh = ops.FieldHandle(grads, pspec)
    d_pos = torch.zeros(R, S, 3, device="cuda")
    cam = torch.zeros(R, dtype=torch.int64, device="cuda")
    args = (fh, gh, scene, to_dev(rb.origins), to_dev(rb.directions), cam, to_dev(starts), to_dev(ends), to_dev(gd),
            torch.zeros(R, S, 3, device="cuda"), torch.zeros(R, S, device="cuda"))
    (ops.field_backward_general if general else ops.field_backward)(*args, d_positions=d_pos, flags=0)
    return d_pos


@pytest.mark.parametrize("shape", ["default", "big", "tcnn_f16"])
def test_position_gradient_matches_the_training_backward(ops, shape):
    """Same d_density, zero d_rgb / d_semantics, flags 0: the two device routes share the gather and the cell decision."""
    if shape == "tcnn_f16":
        sc = make_tcnn_scene(seed=3, log2_T=15, num_images=5, height=12, width=12, focal=16.0, prop_log2_T=10)
        pspec, _ = product_specs(sc)
        dp16 = dev_params(sc)  # half table, tcnn layout
        assert dp16["field.mlp_base_grid.hash_table"].dtype == torch.float16
        dp = dict(dp16)  # the backward needs an fp32 table: the same values widened
        dp["field.mlp_base_grid.hash_table"] = dp16["field.mlp_base_grid.hash_table"].float()
        R, S = 70, 13
        rb = ORY.image_rays(sc.c2w, sc.intr, 1, 12, 12).slice(0, R)
        rb = dataclasses.replace(rb, nears=torch.full((R, 1), 0.05), fars=torch.full((R, 1), 6.0))
        rs = OSM.spaced_sampler(rb, S, "uniform")
        starts, ends = rs.starts[..., 0].contiguous(), rs.ends[..., 0].contiguous()
        gd = torch.randn(R, S, generator=torch.Generator().manual_seed(4))
        fh_new = ops.FieldHandle(dp16, pspec)
    else:
        sc, _, pspec, params, rb, starts, ends, gd = _field_case(shape)
        dp = {k: to_dev(v) for k, v in params.items()}
        fh_new = ops.FieldHandle(dp, pspec)
    worst = 0.0
    for contraction in (True, False):
        scene = ops.scene_struct(sc.aabb, contraction)
        got = ops.field_density_position_gradient(fh_new, scene, to_dev(rb.origins), to_dev(rb.directions), to_dev(starts),
                                                  to_dev(ends), to_dev(gd), want_density=True)
        ref = _backward_route(ops, ops.FieldHandle(dp, pspec), pspec, dp, scene, rb, starts, ends, gd, general=shape != "default")
        assert float(ref.abs().max()) > 0
        worst = max(worst, _rel_l2(got["d_positions"], ref))
        fo = ops.field_eval(ops.FieldHandle(dp, pspec), scene, to_dev(rb.origins), to_dev(rb.directions), None, to_dev(starts),
                            to_dev(ends))
        assert _rel_l2(got["density"], fo["density"]) <= 1e-5
        assert torch.equal(got["density"] == 0, fo["density"] == 0)
    print(f"position gradient, {shape}: relative L2 error {worst:.3e} against the training backward")
    assert worst <= 1e-4


@pytest.mark.parametrize("contraction", [True, False])
def test_position_gradient_matches_autograd(ops, contraction):
    """Against float64 autograd through ``oracle.field.field_density`` with a requires_grad offset added to the positions;
    torch layout.  Rays run from 0.05 to 6: without contraction most samples lie outside the box and give exact zeros."""
    sc, ospec, pspec, params, rb, starts, ends, gd = _field_case("default")
    p64 = {k: v.double() for k, v in params.items()}
    points = (rb.origins[:, None, :] + rb.directions[:, None, :] * ((starts + ends) / 2)[..., None]).double()
    offsets = torch.zeros_like(points, requires_grad=True)
    density, _ = OF.field_density(points + offsets, p64, ospec, sc.aabb.double(), contraction)
    (density[..., 0] * gd.double()).sum().backward()
    dp = {k: to_dev(v) for k, v in params.items()}
    got = ops.field_density_position_gradient(ops.FieldHandle(dp, pspec), ops.scene_struct(sc.aabb, contraction),
                                              to_dev(rb.origins), to_dev(rb.directions), to_dev(starts), to_dev(ends),
                                              to_dev(gd))["d_positions"].cpu()
    err = _rel_l2(got, offsets.grad)
    print(f"position gradient, contraction {contraction}: relative L2 error {err:.3e} against autograd")
    assert err <= 1e-2
    _, sel = REF.normalized(points.float(), sc.aabb, contraction)
    if not contraction:
        assert 0 < int((~sel).sum()) < sel.numel()
    assert bool((got[~sel] == 0).all()) and float(got[sel].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ model level
LOD = 4


def _model_setup(num_images=5, rays_per_batch=70, **cfg):
    from cropnerf_amd.config import FruitNerfModelConfig
    from cropnerf_amd.fruit_nerf.fruit_nerf import FruitModel, Semantics
    from cropnerf_amd.rays import SceneBox

    sc = make_scene(seed=4, log2_T=15, num_images=num_images, height=24, width=24, focal=33.0, prop_log2_T=13)
    params = dict(sc.params)
    params["camera_optimizer.pose_adjustment"] = torch.zeros_like(params["camera_optimizer.pose_adjustment"])
    params["field.mlp_base_mlp.layers.1.bias"] = params["field.mlp_base_mlp.layers.1.bias"].clone()
    params["field.mlp_base_mlp.layers.1.bias"][0] += 2.0  # denser matter: weights that vary along a ray
    sc = dataclasses.replace(sc, params=params)
    pl = [{"hidden_dim": 16, "log2_hashmap_size": p.grid.log2_hashmap_size, "num_levels": 5, "max_res": p.grid.max_res}
          for p in sc.pspecs]
    config = FruitNerfModelConfig(log2_hashmap_size=sc.fspec.grid.log2_hashmap_size, proposal_net_args_list=pl, **cfg)
    model = FruitModel(config, SceneBox(sc.aabb), num_train_data=num_images, metadata={"semantics": Semantics()},
                       device="cuda", test_mode="test", params=sc.params)
    return sc, config, model


@pytest.fixture(scope="module")
def setup():
    return _model_setup()


def test_hessian_for_samples_matches_the_float64_restatement(setup):
    """2 batches of 70 rays x 48 samples (the oracle proposal sampler's final samples, made on the CPU), lod 4: field_eval ->
    kernels 1, 2, 3 against oracle-field autograd in float64 + the reference's reduction in torch."""
    from cropnerf_amd.fruit_nerf.bayesrays import hessian_for_samples

    sc, _, model = setup
    model.eval()
    om = oracle_model(sc, "test")
    ref = torch.zeros((2 ** LOD + 1) ** 3, dtype=torch.float64)
    got = None
    for b in range(2):
        rb = ORY.image_rays(sc.c2w, sc.intr, 1 + b, sc.height, sc.width).slice(200, 270)
        out = om.forward(rb)
        starts, ends = out["_starts"][..., 0].contiguous(), out["_ends"][..., 0].contiguous()
        assert tuple(starts.shape) == (70, 48)
        points, grads = REF.sample_gradients(sc.params, sc.fspec, sc.aabb, True, rb.origins, rb.directions, starts, ends)
        ref += REF.hessian_reduction(points, grads, sc.aabb.double(), True, LOD)
        got = hessian_for_samples(model, to_dev(rb.origins), to_dev(rb.directions), None, to_dev(starts), to_dev(ends), LOD, got)
    got = got.cpu().double()
    err = _rel_l2(got, ref)
    floor = 1e-6 * float(ref.max())
    print(f"end to end: relative L2 error of H {err:.3e}; {int((ref > floor).sum())} non-zero vertices, max H {float(ref.max()):.4g}")
    assert float(ref.max()) > 0 and err <= 2e-2
    differ = ((got != 0) != (ref != 0)) & (torch.maximum(got, ref) >= floor)  # entries below the floor on both sides do not count
    assert not bool(differ.any()), f"{int(differ.sum())} vertices are non-zero on one side only"


def test_round_trip_through_the_cli(setup, tmp_path):
    """compute_hessian over a 3-batch datamanager; the ``compute`` CLI writes a file ``load_hessian`` accepts; rendering a training
    camera with it gives a finite uncertainty whose mean lies strictly below the zero-Hessian one's."""
    from cropnerf_amd.fruit_nerf import bayesrays as B
    from cropnerf_amd.fruit_nerf.checkpoint import eval_setup, save_run
    from cropnerf_amd.fruit_nerf.scripts import uncertainty as U
    from cropnerf_amd.rays import Cameras, SceneBox

    sc, config, _ = _model_setup(num_images=3)
    cams = Cameras(sc.c2w, sc.intr[:, 0], sc.intr[:, 1], sc.intr[:, 2], sc.intr[:, 3], sc.height, sc.width)
    cfg_path = save_run(tmp_path / "outputs" / "plant" / "fruit_nerf" / "run0", config, cams, SceneBox(sc.aabb), sc.params, step=3)
    _, pipe, _, _ = eval_setup(cfg_path, test_mode="test")
    pipe.model.training = True
    h, n = B.compute_hessian(pipe.model, pipe.datamanager, lod=LOD, iters=1)
    assert pipe.model.training is True  # restored
    assert n == 3 * pipe.datamanager.config.train_num_rays_per_batch and pipe.datamanager.train_count == 3
    assert h.dtype == np.float32 and h.shape == ((2 ** LOD + 1) ** 3,) and np.isfinite(h).all() and h.max() > 0 and h.min() >= 0
    out_path = tmp_path / "unc" / "unc.npy"
    U.entrypoint(["compute", "--load-config", str(cfg_path), "--output-path", str(out_path), "--lod", str(LOD), "--iters", "2"])
    loaded, lod = B.load_hessian(out_path)
    assert lod == LOD and loaded.dtype == np.float32 and loaded.max() > 0
    model = pipe.model.eval()
    rays = pipe.datamanager.train_dataset.cameras.to(model.device).generate_rays(camera_indices=0, keep_shape=True).flatten()
    with_h = B.get_outputs_with_uncertainty(model, rays, B.UncertaintyState(loaded, N=float(n)))["uncertainty"]
    zero_h = B.get_outputs_with_uncertainty(model, rays, B.UncertaintyState(np.zeros_like(loaded), N=float(n)))["uncertainty"]
    assert bool(torch.isfinite(with_h).all())
    print(f"round trip: mean uncertainty {float(with_h.mean()):.4f} with the computed Hessian, {float(zero_h.mean()):.4f} with zeros")
    assert float(with_h.mean()) < float(zero_h.mean())


# ------------------------------------------------------------------------------------------------ error paths
def test_error_paths(ops, setup):
    from cropnerf_amd import config as PC
    from cropnerf_amd._lib import CropNerfHipError
    from cropnerf_amd.fruit_nerf import bayesrays as B

    sc, _, model = setup
    scene = ops.scene_struct(sc.aabb, True)
    R = 4
    o, d = torch.zeros(R, 3, device="cuda"), torch.ones(R, 3, device="cuda")
    z = lambda *s: torch.zeros(*s, device="cuda")
    for lod in (0, 11):
        with pytest.raises(CropNerfHipError):
            ops.hessian_accumulate(o, d, z(R, 5), z(R, 5), z(R, 5, 3), scene, lod, z(17 ** 3))
        with pytest.raises(ValueError):
            B.hessian_for_samples(model, o, d, None, z(R, 5), z(R, 5), lod)
    with pytest.raises(CropNerfHipError, match="257"):
        ops.hessian_accumulate(o, d, z(R, 257), z(R, 257), z(R, 257, 3), scene, 4, z(17 ** 3))
    with pytest.raises(ValueError):  # a buffer of another lod's length
        ops.hessian_accumulate(o, d, z(R, 5), z(R, 5), z(R, 5, 3), scene, 4, z(9 ** 3))
    with pytest.raises(ValueError):
        B.hessian_for_samples(model, o, d, None, z(R, 5), z(R, 5), 4, out=z(9 ** 3))
    # base width 256
    ospec = OF.FieldSpec(grid=OF.GridSpec(16, 16, 2048, 12, 2), hidden_dim=256, num_images=3)
    params = {k: to_dev(v) for k, v in OF.random_params(ospec, [], seed=1).items() if k.startswith("field.")}
    wide = ops.FieldHandle(params, PC.FieldSpec(grid=PC.GridSpec(16, 16, 2048, 12, 2), hidden_dim=256, num_images=3))
    with pytest.raises(CropNerfHipError, match="256"):
        ops.field_density_position_gradient(wide, scene, o, d, z(R, 5), z(R, 5), z(R, 5))
    _, _, passing = _model_setup(pass_semantic_gradients=True)
    with pytest.raises(NotImplementedError, match="pass_semantic_gradients"):
        B.hessian_for_samples(passing, o, d, None, z(R, 5), z(R, 5), 4)
