"""Torch restatements of the BayesRays Hessian stage (``bayesrays/uncertainty.py:44-90, 93-153``) shared by
``test_bayesrays_hessian_host.py`` and ``test_gpu_bayesrays_hessian.py``: CPU only, float64 where the caller passes doubles."""

from __future__ import annotations

import torch

from oracle import field as OF
from oracle import samplers as OSM


def normalized(points, aabb, contraction):
    """``normalize_point_coords`` (``bayesrays/utils.py:6-15``): positions in [0, 1)^3, zeroed when deselected, and the selector."""
    if contraction:
        mag = points.abs().amax(-1, keepdim=True)
        pos = (torch.where(mag < 1, points, (2 - 1 / mag) * (points / mag)) + 2.0) / 4.0
    else:
        pos = (points - aabb[0].to(points)) / (aabb[1] - aabb[0]).to(points)
    sel = ((pos > 0.0) & (pos < 1.0)).all(-1)
    return pos * sel[..., None], sel


def hessian_reduction(points, grads, aabb, contraction, lod, channel_scale=3.0):
    """What ``cn_hessian_accumulate`` adds for one batch: literal (aliasing) indices, coefficients zeroed for deselected samples,
    sums per (ray, index) BEFORE the square, ``channel_scale * |a|^2`` added per vertex.  points, grads [R,S,3]."""
    R, S = points.shape[:2]
    Lr = 2 ** lod
    n = (Lr + 1) ** 3
    pos, sel = normalized(points, aabb, contraction)
    x = pos * Lr
    f = x.floor()
    ray = torch.arange(R)[:, None].expand(R, S)
    keys, vals = [], []
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                idx = ((f[..., 0] + cx) * Lr * Lr + (f[..., 1] + cy) * Lr + (f[..., 2] + cz)).long()
                coef = ((x[..., 0] - (f[..., 0] + 1 - cx)).abs() * (x[..., 1] - (f[..., 1] + 1 - cy)).abs()
                        * (x[..., 2] - (f[..., 2] + 1 - cz)).abs()) * sel
                keys.append((ray * n + idx).reshape(-1))
                vals.append((coef[..., None] * grads).reshape(-1, 3))
    keys, vals = torch.cat(keys), torch.cat(vals)
    uniq, inv = torch.unique(keys, return_inverse=True)
    a = torch.zeros(uniq.numel(), 3, dtype=vals.dtype).index_add_(0, inv, vals)
    return torch.zeros(n, dtype=vals.dtype).index_add_(0, uniq % n, channel_scale * (a * a).sum(-1))


def semantics_density_gradient_formula(starts, ends, density, sem):
    """The closed form ``cn_semantics_density_gradient`` evaluates, in the dtype of its inputs ([R,S] each)."""
    delta = ends - starts
    dd = delta * density
    excl = torch.cumsum(dd, -1) - dd
    trans = torch.exp(-excl)
    w = torch.nan_to_num((1 - torch.exp(-dd)) * trans)
    wl = w * sem
    total = wl.sum(-1, keepdim=True)
    suffix = total - torch.cumsum(wl, -1)
    return total, w, delta * (torch.exp(-(excl + dd)) * sem - suffix)


def semantics_density_gradient_autograd(starts, ends, density, sem):
    """float64 autograd over the oracle's ``get_weights``: rendered semantics [R,1] and d / d density [R,S]."""
    den = density.double().clone().requires_grad_(True)
    w = OSM.get_weights((ends - starts).double()[..., None], den[..., None])[..., 0]
    out = (w * sem.double()).sum(-1, keepdim=True)
    out.sum().backward()
    return out.detach(), w.detach(), den.grad


def sample_gradients(params, spec, aabb, contraction, origins, directions, starts, ends, dtype=torch.float64):
    """``get_unc_nerfacto`` + the backward of ``find_uncertainty`` on the oracle field: d (sum_s w_s logit_s) / d offset_s with
    a zero offset added to every sample position, logits from detached geo features.  Returns (points, gradients) [R,S,3]."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
    o, d, starts, ends = (t.to(dtype) for t in (origins, directions, starts, ends))
    points = o[:, None, :] + d[:, None, :] * ((starts + ends) / 2)[..., None]
    offsets = torch.zeros_like(points, requires_grad=True)
    density, geo = OF.field_density(points + offsets, p, spec, aabb.to(dtype), contraction)
    logits = OF.semantics_from_geo(geo.detach().reshape(-1, spec.geo_feat_dim), p, spec).view(*starts.shape)
    w = OSM.get_weights((ends - starts)[..., None], density)[..., 0]
    (w * logits).sum().backward()
    return points.detach(), offsets.grad
