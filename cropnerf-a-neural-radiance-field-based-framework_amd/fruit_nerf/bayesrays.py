"""BayesRays -- mirror of ``crop_nerf/fruit_nerf/bayesrays``: the Hessian stage (``uncertainty.py``) and the renders made from
its grid (``output_uncertainty.py``: ``get_uncertainty :19-30``, ``get_output_nerfacto_new :32-111``,
``get_output_nerfacto_all :279-314``, with the attributes ``run_viewer_u.py`` sets on the model, ``:373-382``; its
``get_output_nerfacto_new :80-170`` adds the semantic outputs).

Producer: ``compute_hessian`` walks training batches with the model in eval (no jitter, eval near plane, eval appearance
embedding, no camera-optimizer step), takes the proposal sampler's final samples and accumulates, per ray and literal grid vertex,
``3 |sum coef * d semantics / d x|^2`` (``uncertainty.py:44-90, 292-339``): ``cn_field_eval`` -> ``cn_semantics_density_gradient``
-> ``cn_field_density_position_gradient`` -> ``cn_hessian_accumulate``.  The rendered semantics reach the sample positions through
the density only -- the logits come from detached geo features (``fruit_field.py:264-266``) -- so ``pass_semantic_gradients=True``
is refused rather than computed in the detached form.  The field runs in fp32 here whatever the model's ``matrix_precision``.

Consumer: from a Hessian grid -- the ``unc.npy`` of the producer or of the reference's script -- to an
``uncertainty`` image and, with ``filter_out``, renders from which uncertain matter is removed: the mask
``un_points <= filter_thresh * 6`` multiplies every density, in the proposal networks and in the field, before its weights.

The reference patches these functions over ``model.get_outputs``; here they are functions of (model, ray_bundle, state) and
``FruitModel.get_outputs`` is untouched.  Every number comes from a HIP kernel.  The proposal loop runs through the unfused
entry points (``cn_sample_spaced`` / ``cn_proposal_density`` / ``cn_composite`` / ``cn_sample_pdf``), because the mask sits
between a level's density and its weights; the field is evaluated per sample by ``cn_field_eval`` (any field shape).
Like the reference's function -- and unlike ``FruitModel.get_outputs`` -- there is no camera-optimizer tweak of the rays.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from .. import ops
from ..rays import RayBundle

__all__ = ["MAX_UNCERTAINTY", "MIN_UNCERTAINTY", "DEFAULT_N", "load_hessian", "UncertaintyState",
           "get_outputs_with_uncertainty", "get_outputs_for_filter_levels", "hessian_for_samples", "hessian_for_rays",
           "compute_hessian"]

MAX_UNCERTAINTY, MIN_UNCERTAINTY = 6, -3  # output_uncertainty.py:41-42 (cn_uncertainty_composite holds the same two)
DEFAULT_N = 1000 * 4096  # run_viewer_u.py:376: query iterations x rays per batch of the Hessian stage


def load_hessian(path, lod: Optional[int] = None):
    """``unc.npy`` -> (float32 array [(2^lod + 1)^3], lod).  ``lod`` is inferred from the length (``run_viewer_u.py:377``);
    ``ValueError`` when the length is not ``(2^k + 1)^3`` (or not the given ``lod``'s)."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: no Hessian file (the unc.npy that `uncertainty.py compute` writes)")
    h = np.ascontiguousarray(np.load(str(path)), dtype=np.float32).reshape(-1)
    inferred = ops.uncertainty_lod(h.size)
    if lod is not None and int(lod) != inferred:
        raise ValueError(f"{path}: {h.size} values are a lod-{inferred} grid, not lod {lod}")
    return h, inferred


@dataclass
class UncertaintyState:
    """What ``run_viewer_u.py:373-380`` hangs on the model: ``hessian``, ``N``, ``lod``, ``filter_thresh``, the two
    background switches, and ``filter_out`` of ``output_uncertainty.py:44``."""

    hessian: object  # numpy array or tensor, (2^lod + 1)^3 values
    N: float = DEFAULT_N
    lod: Optional[int] = None
    filter_out: bool = False
    filter_thresh: float = 1.0
    white_bg: bool = False
    black_bg: bool = False
    _un: Optional[Tensor] = field(default=None, repr=False)

    def __post_init__(self):
        n = int(self.hessian.numel() if isinstance(self.hessian, Tensor) else np.asarray(self.hessian).size)
        inferred = ops.uncertainty_lod(n)
        if self.lod is not None and int(self.lod) != inferred:
            raise ValueError(f"hessian has {n} values: a lod-{inferred} grid, not lod {self.lod}")
        self.lod = inferred

    def table(self, device) -> Tensor:
        """``un = 1 / (H / N + lambda)`` on ``device`` (``cn_uncertainty_table``; computed once, kept)."""
        if self._un is None or self._un.device != torch.device(device):
            h = self.hessian if isinstance(self.hessian, Tensor) else torch.from_numpy(np.asarray(self.hessian))
            h = h.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
            self._un = ops.uncertainty_table(h, self.N, self.lod)
        return self._un

    def background(self, model):
        if self.white_bg:
            return L.BG_COLOR, (1.0, 1.0, 1.0)
        if self.black_bg:
            return L.BG_COLOR, (0.0, 0.0, 0.0)
        return model._background()


def _render(model, ray_bundle: RayBundle, state: UncertaintyState, filter_out: bool, filter_thresh: float,
            full: bool) -> Dict[str, Tensor]:
    cfg = model.config
    rb = model._prepared(ray_bundle)
    o, d, n, f = rb.origins, rb.directions, rb.nears, rb.fars
    cam = model._cam_idx(rb)
    if model._app_mode() == L.APP_PER_CAMERA and cam is None:
        raise AttributeError("Camera indices are not provided.")
    un, lod = state.table(o.device), state.lod
    limit = float(filter_thresh) * MAX_UNCERTAINTY
    prop_scene = model._scene(model._prop_contraction)
    field_scene = model._scene(model._field_contraction)  # get_uncertainty reads the FIELD's distortion at every level

    def masked(density, starts, ends):
        return ops.uncertainty_lookup(o, d, starts, ends, field_scene, un, lod, density if filter_out else None, limit)

    out: Dict[str, Tensor] = {}
    n_lvl = len(model.proposal_networks)
    sm = ops.sample_spaced(n, f, cfg.num_proposal_samples_per_ray[0], L.SPACING_PIECEWISE)
    bins = torch.cat([sm["spacing_starts"], sm["spacing_ends"][:, -1:]], -1).contiguous()
    starts, ends = sm["starts"], sm["ends"]
    for lvl in range(n_lvl):
        den = ops.proposal_density(model.proposal_networks[lvl], prop_scene, o, d, starts, ends)
        if filter_out:
            masked(den, starts, ends)
        comp = ops.composite(starts, ends, den, want_weights=True)
        out[f"prop_depth_{lvl}"] = comp["depth"]
        s_next = cfg.num_proposal_samples_per_ray[lvl + 1] if lvl + 1 < n_lvl else cfg.num_nerf_samples_per_ray
        bins, eu = ops.sample_pdf(bins, comp["weights"], n, f, s_next, anneal=model._anneal)
        starts, ends = eu[:, :-1].contiguous(), eu[:, 1:].contiguous()
    fo = ops.field_eval(model.field, field_scene, o, d, cam, starts, ends, app_mode=model._app_mode(),
                        sh_unit_dir=cfg.sh_input == "unit", matrix_precision=model._matrix_precision())
    density = fo["density"]
    if full:  # run_viewer_u.py:59-78,120-130: the semantic weights come from the UNFILTERED density, kept where the sample
        # is labelled fruit and dense, set to the batch's smallest density elsewhere
        fruit = (torch.sigmoid(fo["semantics"]) - 0.9 > 0) & (density >= 70)
        sem_density = torch.where(fruit, density, density.min())
    un_points = masked(density, starts, ends)  # masks fo["density"] in place when filtering
    bg_mode, bg = state.background(model)
    comp = ops.composite(starts, ends, density, fo["rgb"], None, bg_mode, bg, eval_clamp=not model.training,
                         want_weights=full)
    res = {"rgb": comp["rgb"], "accumulation": comp["accumulation"], "depth": comp["depth"]}
    if not full:
        return res
    res["uncertainty"] = ops.uncertainty_composite(comp["weights"], un_points)
    res.update(out)
    sem = ops.composite(starts, ends, sem_density, None, fo["semantics"], eval_clamp=not model.training)
    res["semantics"], res["semantics_colormap"] = sem["semantics"], sem["semantics_colormap"]
    return res


@torch.no_grad()
def get_outputs_with_uncertainty(model, ray_bundle: RayBundle, state: UncertaintyState) -> Dict[str, Tensor]:
    """``get_output_nerfacto_new`` (``output_uncertainty.py:32-111``) in eval: collider, proposal sampling (no jitter, the
    model's current anneal) with every proposal density masked when ``state.filter_out``, field, mask, renderers.  Outputs
    ``rgb``, ``accumulation``, ``depth``, ``uncertainty`` ([R,1] in [0, 1]), ``prop_depth_i`` and, as
    ``run_viewer_u.py:80-170`` has them, ``semantics`` / ``semantics_colormap``."""
    return _render(model, ray_bundle, state, state.filter_out, state.filter_thresh, full=True)


@torch.no_grad()
def get_outputs_for_filter_levels(model, ray_bundle: RayBundle, state: UncertaintyState,
                                  thresh_range: Sequence[float]) -> Dict[str, Tensor]:
    """``get_output_nerfacto_all`` (``output_uncertainty.py:279-314``): one filtered render per threshold, keys
    ``rgb-0.50``, ``accumulation-0.50``, ``depth-0.50``."""
    outputs: Dict[str, Tensor] = {}
    for thresh in thresh_range:
        thresh = float(thresh.item() if isinstance(thresh, Tensor) else thresh)
        res = _render(model, ray_bundle, state, True, thresh, full=False)
        for k in ("rgb", "accumulation", "depth"):
            outputs[f"{k}-{thresh:.2f}"] = res[k]
    return outputs


# ------------------------------------------------------------------------------------------------ the Hessian stage
def _refuse_semantic_gradients(model) -> None:
    if getattr(model.config, "pass_semantic_gradients", False):
        raise NotImplementedError(
            "pass_semantic_gradients=True: the semantic logits then depend on the sample positions as well, and the Hessian "
            "stage differentiates the density path only (the reference's default, detached geo features)")


def _new_hessian(lod: int, device) -> Tensor:
    if not 1 <= int(lod) <= 10:
        raise ValueError(f"lod {lod} outside [1, 10]")
    return torch.zeros(((1 << int(lod)) + 1) ** 3, dtype=torch.float32, device=device)


@torch.no_grad()
def hessian_for_samples(model, origins: Tensor, directions: Tensor, camera_indices: Optional[Tensor], starts: Tensor,
                        ends: Tensor, lod: int, out: Optional[Tensor] = None) -> Tensor:
    """One batch of ``find_uncertainty`` (``uncertainty.py:44-90``) on given samples: adds to ``out`` (a new zero grid of
    ``(2^lod + 1)^3`` floats when None) and returns it."""
    _refuse_semantic_gradients(model)
    if out is None:
        out = _new_hessian(lod, starts.device)
    scene = model._scene(model._field_contraction)
    fo = ops.field_eval(model.field, scene, origins, directions, camera_indices, starts, ends, app_mode=model._app_mode(),
                        sh_unit_dir=model.config.sh_input == "unit", matrix_precision=L.MATRIX_FP32)
    dd = ops.semantics_density_gradient(starts, ends, fo["density"], fo["semantics"])["d_density"]
    dp = ops.field_density_position_gradient(model.field, scene, origins, directions, starts, ends, dd)["d_positions"]
    return ops.hessian_accumulate(origins, directions, starts, ends, dp, scene, lod, out)  # 3: semantics.repeat(1, 3), :326


@torch.no_grad()
def hessian_for_rays(model, ray_bundle: RayBundle, lod: int, out: Optional[Tensor] = None) -> Tensor:
    """``get_unc_nerfacto`` + ``find_uncertainty`` for one ray bundle: collider, the model's proposal sampler as it runs in the
    model's current mode (``compute_hessian`` puts it in eval), then ``hessian_for_samples`` on its final samples."""
    _refuse_semantic_gradients(model)
    cfg = model.config
    rb = model._prepared(ray_bundle)
    cam = model._cam_idx(rb)
    if model._app_mode() == L.APP_PER_CAMERA and cam is None:
        raise AttributeError("Camera indices are not provided.")
    ps = ops.proposal_sample(model.proposal_networks, model._scene(model._prop_contraction), rb.origins, rb.directions,
                             rb.nears, rb.fars, cfg.num_proposal_samples_per_ray, cfg.num_nerf_samples_per_ray,
                             anneal=model._anneal, matrix_precision=L.MATRIX_FP32)
    bins = ps["euclidean_bins"]
    return hessian_for_samples(model, rb.origins, rb.directions, cam, bins[:, :-1].contiguous(), bins[:, 1:].contiguous(),
                               lod, out)


def compute_hessian(model, datamanager, lod: int = 8, iters: int = 1000) -> Tuple[np.ndarray, int]:
    """``ComputeUncertainty.main`` (``uncertainty.py:292-339``): ``max(len(train_dataset), iters)`` batches of
    ``datamanager.next_train`` through the model in eval.  Returns the float32 grid [(2^lod + 1)^3] -- what ``np.save`` writes
    as ``unc.npy`` -- and N = batches x rays per batch, the count ``UncertaintyState`` divides by."""
    _refuse_semantic_gradients(model)
    hessian = _new_hessian(lod, model.device)
    steps = max(len(datamanager.train_dataset), int(iters))
    was_training = model.training
    model.eval()
    rays = 0
    try:
        for step in range(steps):
            ray_bundle, _ = datamanager.next_train(step)
            rays += int(ray_bundle.origins.reshape(-1, 3).shape[0])
            hessian_for_rays(model, ray_bundle, lod, hessian)
    finally:
        model.training = was_training
    return hessian.cpu().numpy(), rays
