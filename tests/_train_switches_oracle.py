"""Oracle restatement of the training forward with the two gradient switches of ``FruitNerfModelConfig``.

``oracle.losses.train_forward`` (``FruitModel.get_outputs`` in training) with:

- ``pass_semantic_gradients`` (``fruit_nerf.py:65``): no ``.detach()`` on the semantic MLP's geo input
  (``fruit_field.py:265-266``) nor on the weights the semantic renderer gets (``fruit_nerf.py:587-590``);
- ``use_gradient_scaling`` (nerfacto's field, ``fruit_nerf.py:553-554``): nerfstudio's ``scale_gradients_by_distance_squared``
  on the field outputs -- the identity forward, and in the backward the gradient of every output of sample i (density, rgb,
  semantics) times ``clamp(((start_i + end_i) / 2) ** 2, 0, 1)``.  That function lives upstream in nerfstudio 1.1.3, not in
  the reference; it is restated here from its documented arithmetic, so its parity is unpinned, like the other upstream
  arithmetic the oracle restates.

With both switches off the operations are those of ``oracle.losses.train_forward``, in the same order.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

from oracle import field as F
from oracle import rays as RY
from oracle import render as RD
from oracle import samplers as SM


class GradientScaler(torch.autograd.Function):
    """Identity forward; backward multiplies the incoming gradient by ``clamp(ray_dist ** 2, 0, 1)`` (constant: the bins
    are detached)."""

    @staticmethod
    def forward(ctx, value: Tensor, ray_dist: Tensor) -> Tensor:
        ctx.save_for_backward(ray_dist)
        return value.view_as(value)

    @staticmethod
    def backward(ctx, grad: Tensor):
        (ray_dist,) = ctx.saved_tensors
        return grad * torch.square(ray_dist).clamp(0, 1), None


def scale_factor(starts: Tensor, ends: Tensor) -> Tensor:
    """The per-sample factor of ``GradientScaler`` ([..., 1])."""
    return torch.square((starts + ends) / 2).clamp(0, 1)


def train_forward(rb: RY.RayBundle, params: Dict[str, Tensor], fspec: F.FieldSpec, pspecs, aabb: Tensor,
                  num_proposal_samples: Sequence[int], num_nerf_samples: int, jitter: Sequence[Optional[Tensor]],
                  pass_semantic_gradients: bool = False, use_gradient_scaling: bool = False, anneal: float = 1.0,
                  near_plane: float = 0.05, far_plane: float = 1000.0, apply_pose: bool = True,
                  update_proposals: bool = True) -> Dict[str, Tensor]:
    rb = RY.near_far_collider(rb, training=True, near_plane=near_plane, far_plane=far_plane)
    if apply_pose:
        rb = RY.apply_pose_adjustment(rb, params["camera_optimizer.pose_adjustment"])

    def _fn(i, ps):
        def fn(pos):
            den = F.proposal_density(pos, params, i, ps, aabb, True)
            return den if update_proposals else den.detach()
        return fn

    fns = [_fn(i, ps) for i, ps in enumerate(pspecs)]
    rs, weights_list, samples_list = SM.proposal_sampler(rb, fns, num_proposal_samples, num_nerf_samples,
                                                         anneal=anneal, jitter=jitter)
    fo = F.field_forward(rs.positions(), rs.directions, rs.camera_indices, params, fspec, aabb, True, "val",
                         training=True)
    density, rgb_s = fo["density"], fo["rgb"]
    if use_gradient_scaling:
        ray_dist = (rs.starts + rs.ends) / 2
        density = GradientScaler.apply(density, ray_dist)
        rgb_s = GradientScaler.apply(rgb_s, ray_dist)
    weights = SM.get_weights(rs.deltas, density)
    weights_list = list(weights_list) + [weights]
    samples_list = list(samples_list) + [rs]
    rgb = RD.render_rgb(rgb_s, weights, "last_sample", training=True)
    geo = F.field_density(rs.positions(), params, fspec, aabb, True)[1]
    if not pass_semantic_gradients:
        geo = geo.detach()
    sem_s = F.semantics_from_geo(geo.reshape(-1, fspec.geo_feat_dim), params, fspec).view(*weights.shape[:2], 1)
    if use_gradient_scaling:
        sem_s = GradientScaler.apply(sem_s, ray_dist)
    sem = RD.render_semantics(sem_s, weights if pass_semantic_gradients else weights.detach())
    return {"rgb": rgb, "semantics": sem, "accumulation": RD.render_accumulation(weights),
            "weights_list": weights_list, "ray_samples_list": samples_list, "_field": fo}
