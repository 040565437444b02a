"""Host-side tests of the BayesRays Hessian stage (no GPU): the specification the kernels implement is the reference's -- a torch
restatement of ``cn_hessian_accumulate`` meets ``tests/golden/bayesrays_hessian.npz`` (outputs of the reference's own
``find_uncertainty``) and the closed form of ``cn_semantics_density_gradient`` meets float64 autograd, both at the bars the GPU
tests hold the kernels to -- the ``compute`` sub-command parses the reference's field names, and the fixture regenerates equal.
"""

import os
import sys

import numpy as np
import pytest
import torch

import _bayesrays_hessian_ref as REF

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(lod, c, si) for lod in (3, 4) for c in (0, 1) for si in (0, 1)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "bayesrays_hessian.npz"))


def _generator():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_golden_bayesrays_hessian as M
    finally:
        sys.path.pop(0)
    return M


def _case(gold, si):
    t = {k: torch.from_numpy(gold[f"s{si}/{k}"]) for k in ("origins", "directions", "bins", "gradients")}
    starts, ends = t["bins"][:, :-1], t["bins"][:, 1:]
    points = t["origins"][:, None, :] + t["directions"][:, None, :] * ((starts + ends) / 2)[..., None]
    return points, t["gradients"]


@pytest.mark.parametrize("lod,c,si", CASES)
def test_reduction_restatement_meets_the_fixture(gold, lod, c, si):
    """float32, as the kernel: |dH| <= 4e-4 H_ref + 4e-5 max H_ref on every vertex."""
    points, grads = _case(gold, si)
    ref = torch.from_numpy(gold[f"lod{lod}/c{c}/s{si}/hessian"])
    got = REF.hessian_reduction(points, grads, torch.from_numpy(gold["aabb"]), bool(c), lod)
    assert got.dtype == torch.float32 and got.shape == ref.shape == ((2 ** lod + 1) ** 3,)
    err = (got - ref).abs()
    assert bool((err <= 4e-4 * ref + 4e-5 * ref.max()).all()), f"worst {float((err / (4e-4 * ref + 4e-5 * ref.max())).max()):.3g} of the bar"
    assert torch.equal(got != 0, ref != 0)


def test_fixture_holds_the_stated_cases(gold):
    assert gold["lods"].tolist() == [3, 4] and gold["shapes"].tolist() == [[70, 48], [5, 5]]
    aabb = torch.from_numpy(gold["aabb"])
    for si in (0, 1):
        points, grads = _case(gold, si)
        assert tuple(grads.shape) == tuple(gold["shapes"][si]) + (3,) and bool((grads.abs().sum(-1) > 0).all())
        _, sel_box = REF.normalized(points, aabb, False)
        _, sel_con = REF.normalized(points, aabb, True)
        assert 0 < int((~sel_box).sum()) < sel_box.numel()  # deselected samples without contraction
        assert bool(sel_con.all())
    assert os.path.getsize(os.path.join(HERE, "golden", "bayesrays_hessian.npz")) < 200 * 1024


@pytest.mark.parametrize("S", [5, 48, 96])
def test_density_gradient_formula_meets_autograd(S):
    """The closed form in float32 against float64 autograd over ``oracle.samplers.get_weights``: 2e-4 / 2e-5 on the rendered value
    and (relative to the largest entry) on d_density; one ray of zero density, one saturated."""
    g = torch.Generator().manual_seed(S)
    R = 70
    width = torch.rand(R, S, generator=g) * 0.1 + 0.01
    bins = torch.cat([torch.zeros(R, 1), torch.cumsum(width, -1)], -1) + 0.05
    starts, ends = bins[:, :-1].contiguous(), bins[:, 1:].contiguous()
    density = torch.rand(R, S, generator=g) ** 3 * 30.0
    density[3] = 0.0
    density[5] = 1e4
    sem = torch.randn(R, S, generator=g) * 3.0
    total, w, dd = REF.semantics_density_gradient_formula(starts, ends, density, sem)
    r_total, r_w, r_dd = REF.semantics_density_gradient_autograd(starts, ends, density, sem)
    assert bool(((total - r_total).abs() <= 2e-4 * r_total.abs() + 2e-5).all())
    assert bool(((w - r_w).abs() <= 2e-4 * r_w.abs() + 2e-5).all())
    assert bool(((dd - r_dd).abs() <= 2e-4 * r_dd.abs() + 2e-5 * r_dd.abs().max()).all())
    assert float(dd[3].abs().max()) > 0 and float(total[3]) == 0.0


def test_cli_parses_the_references_field_names():
    from cropnerf_amd.fruit_nerf.scripts import uncertainty as U

    ap = U.build_parser()
    a = ap.parse_args(["compute", "--load-config", "run/config.json"])
    assert (a.cmd, str(a.load_config), str(a.output_path), a.lod, a.iters) == ("compute", "run/config.json", "unc.npy", 8, 1000)
    a = ap.parse_args(["compute", "--load-config", "c.yml", "--output-path", "o/u.npy", "--lod", "4", "--iters", "3"])
    assert (str(a.output_path), a.lod, a.iters) == ("o/u.npy", 4, 3)
    with pytest.raises(SystemExit):
        ap.parse_args(["compute"])
    with pytest.raises(SystemExit):  # refused before any run directory is read
        U.entrypoint(["compute", "--load-config", "nowhere/config.json", "--lod", "11"])
    # render is untouched
    a = ap.parse_args(["render", "--load-config", "run/config.json", "--unc-path", "unc.npy", "--output-dir", "out"])
    assert a.cmd == "render" and a.filter_thresh == 0.5


def test_semantic_gradients_are_refused():
    from cropnerf_amd.fruit_nerf import bayesrays as B

    class Model:
        class config:
            pass_semantic_gradients = True

    for call in (lambda: B.hessian_for_samples(Model(), None, None, None, None, None, 4),
                 lambda: B.hessian_for_rays(Model(), None, 4), lambda: B.compute_hessian(Model(), None, 4, 1)):
        with pytest.raises(NotImplementedError, match="pass_semantic_gradients"):
            call()


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from cropnerf_amd import ops

    scene = ops.scene_struct(torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]), True)
    z = torch.zeros(4, 5)
    with pytest.raises(ValueError):
        ops.semantics_density_gradient(z, z, z, torch.zeros(4, 6))
    with pytest.raises(ValueError):
        ops.hessian_accumulate(torch.zeros(4, 3), torch.zeros(4, 3), z, z, torch.zeros(4, 5, 2), scene, 4, torch.zeros(17 ** 3))
    with pytest.raises((RuntimeError, TypeError)):
        ops.semantics_density_gradient(z, z, z, z)
    with pytest.raises((RuntimeError, TypeError)):
        ops.hessian_accumulate(torch.zeros(4, 3), torch.zeros(4, 3), z, z, torch.zeros(4, 5, 3), scene, 4, torch.zeros(17 ** 3))


def test_entry_points_validate_on_the_host():
    """Null pointers, lod 0 and 11 and 257 samples are refused before any HIP call."""
    import ctypes as C

    from cropnerf_amd import _lib as L

    lib = L.load()
    null, one = C.c_void_p(0), C.c_void_p(64)
    scene = L.Scene()
    assert lib.cn_semantics_density_gradient(null, one, one, one, 1, 1, one, null, one, null) == -1
    assert lib.cn_hessian_accumulate(one, one, one, one, one, 1, 1, C.byref(scene), 4, 3.0, null, null) == -1
    assert lib.cn_hessian_accumulate(one, one, one, one, one, 1, 1, C.byref(scene), 0, 3.0, one, null) == -2
    assert lib.cn_hessian_accumulate(one, one, one, one, one, 1, 1, C.byref(scene), 11, 3.0, one, null) == -2
    assert lib.cn_hessian_accumulate(one, one, one, one, one, 1, 257, C.byref(scene), 4, 3.0, one, null) == -2
    assert b"257" in lib.cn_last_error()
    assert lib.cn_field_density_position_gradient(None, C.byref(scene), one, one, one, one, one, 1, 1, one, null, null) == -1


def test_fixture_regenerates_equal(gold):
    """Executes the reference's functions again (``tests/golden/make_golden_bayesrays_hessian.py``) and compares every array."""
    M = _generator()
    if not M.available():
        pytest.skip("the reference tree is not on this machine")
    fresh = M.build()
    assert sorted(fresh) == sorted(gold.files)
    for k in gold.files:
        np.testing.assert_array_equal(fresh[k], gold[k], err_msg=k)
