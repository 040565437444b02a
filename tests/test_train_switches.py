"""CPU checks of the two training switches of ``FruitNerfModelConfig``: ``pass_semantic_gradients`` and nerfacto's
``use_gradient_scaling`` -- the config surface, the C-ABI surface, and the oracle restatement the GPU tests
(``test_gpu_train_switches.py``) hold the kernels to."""

import re
from pathlib import Path

import pytest
import torch

from _helpers import make_scene
from oracle import losses as OL
from oracle import rays as ORY
import _train_switches_oracle as TS

ROOT = Path(__file__).resolve().parent.parent
S_PROP, S_FINAL = (64, 32), 16
GPU_GRAD_BAR = 3e-3  # the relative-L2 bar of the end-to-end GPU test (test_gpu_train.py: test_gradients_match_autograd)


def test_use_gradient_scaling_defaults_to_nerfacto():
    from cropnerf_amd.config import FruitNerfModelConfig

    cfg = FruitNerfModelConfig()
    assert cfg.use_gradient_scaling is False
    assert cfg.pass_semantic_gradients is False


def test_config_tree_carries_both_switches():
    """nerfstudio writes every config field to config.yml: both keys reach the model config instead of being dropped."""
    from cropnerf_amd.fruit_nerf import nerfstudio_io as NIO

    tree = {"pipeline": {"model": {"use_gradient_scaling": True, "pass_semantic_gradients": True,
                                   "semantic_loss_weight": 1.0, "predict_normals": False}}}
    mc = NIO.model_config_from_tree(tree)
    assert mc.use_gradient_scaling is True
    assert mc.pass_semantic_gradients is True
    assert NIO.model_config_from_tree({"pipeline": {"model": {}}}).use_gradient_scaling is False


def test_header_declares_the_switch_entry_points_and_constants():
    from cropnerf_amd import _lib as L

    text = (ROOT / "include" / "cropnerf_hip.h").read_text()
    consts = dict(re.findall(r"#define\s+(CN_TRAIN_[A-Z_]+)\s+(\d+)u?\b", text))
    assert consts == {"CN_TRAIN_PASS_SEMANTIC_GRADIENTS": "1", "CN_TRAIN_GRADIENT_SCALING": "2"}
    assert L.TRAIN_PASS_SEMANTIC_GRADIENTS == int(consts["CN_TRAIN_PASS_SEMANTIC_GRADIENTS"])
    assert L.TRAIN_GRADIENT_SCALING == int(consts["CN_TRAIN_GRADIENT_SCALING"])
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("cn_train_render_backward_ex", 21), ("cn_field_backward_ex", 21),
                        ("cn_field_backward_general_ex", 22)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        assert "uint32_t flags" in args, name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name


def _setup(seed=5, R=96):
    # (the scene of test_gpu_train.py's _setup)
    sc = make_scene(seed=seed, log2_T=12, num_images=4, height=20, width=20, focal=28.0, prop_log2_T=10)
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randint(0, 4, (R,), generator=g), torch.randint(0, 20, (R,), generator=g),
                       torch.randint(0, 20, (R,), generator=g)], -1)
    jitter = [torch.rand(R, 1, generator=g) for _ in range(3)]
    image = torch.rand(R, 3, generator=g)
    mask = (torch.rand(R, 1, generator=g) > 0.5).float()
    return sc, idx, jitter, image, mask


def _run(fn, **kw):
    sc, idx, jitter, image, mask = _setup()
    p = {k: v.clone().requires_grad_(True) for k, v in sc.params.items()}
    rb = ORY.pinhole_rays(sc.c2w, sc.intr, idx[:, 0], idx[:, 1], idx[:, 2])
    out = fn(rb, p, sc.fspec, sc.pspecs, sc.aabb, S_PROP, S_FINAL, jitter, **kw)
    ld = OL.loss_dict(out, image, mask)
    ld["camera_opt_regularizer"] = OL.camera_opt_regularizer(p["camera_optimizer.pose_adjustment"])
    sum(ld.values()).backward()
    return ({k: v.detach().clone() for k, v in ld.items()}, {k: v.grad for k, v in p.items() if v.grad is not None}, out)


@pytest.fixture
def one_thread():
    # (the CPU hash-table gradient is an index_add whose multi-threaded summation order varies from run to run)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_restated_oracle_with_both_switches_off_is_train_forward(one_thread):
    l0, g0, _ = _run(OL.train_forward)
    l1, g1, _ = _run(TS.train_forward)
    assert set(l0) == set(l1) and all(torch.equal(l0[k], l1[k]) for k in l0)
    assert set(g0) == set(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("switch", ["pass_semantic_gradients", "use_gradient_scaling"])
def test_each_switch_moves_the_base_gradients_well_past_the_gpu_bar(one_thread, switch):
    """Forward values do not move; the gradients of the base MLP and the hash table move by at least 10x the GPU test's bar,
    so a kernel that ignored the switch fails there."""
    l0, g0, o0 = _run(TS.train_forward)
    l1, g1, o1 = _run(TS.train_forward, **{switch: True})
    assert all(torch.equal(l0[k], l1[k]) for k in l0)
    assert torch.equal(o0["rgb"], o1["rgb"]) and torch.equal(o0["semantics"], o1["semantics"])
    keys = [k for k in g0 if k.startswith("field.mlp_base")]
    assert "field.mlp_base_grid.hash_table" in keys and len(keys) >= 5
    for k in keys:
        rel = (g1[k] - g0[k]).norm().item() / (g0[k].norm().item() + 1e-12)
        assert rel >= 10 * GPU_GRAD_BAR, (k, rel)
    if switch == "pass_semantic_gradients":
        # the semantic MLP's own gradients are the same either way (only its input and weights stop being detached)
        for k in g0:
            if "semantics" in k:
                assert torch.equal(g0[k], g1[k]), k
    else:
        # the scaling is really exercised: a substantial share of the final samples lie closer than unit distance
        rs = o1["ray_samples_list"][-1]
        f = TS.scale_factor(rs.starts, rs.ends)
        assert float((f < 1).float().mean()) >= 0.2


def test_gradient_scaler_is_identity_forward_and_clamped_square_backward():
    x = torch.tensor([[1.0], [2.0], [3.0]], requires_grad=True)
    d = torch.tensor([[0.5], [1.5], [-0.25]])
    y = TS.GradientScaler.apply(x, d)
    assert torch.equal(y, x)
    (y * torch.tensor([[2.0], [3.0], [4.0]])).sum().backward()
    assert torch.allclose(x.grad, torch.tensor([[0.5], [3.0], [0.25]]))
