#!/usr/bin/env python
"""Golden vectors of the BayesRays producer, made by EXECUTING the reference's own code (build container only).

    python tests/golden/make_golden_bayesrays_hessian.py      ->  tests/golden/bayesrays_hessian.npz

Same method as ``make_golden_bayesrays.py`` (whose helpers this file imports): the reference's files are read with ``ast`` and
the definitions are executed unchanged on seeded tensors in a namespace that holds only what they name:

    fruit_nerf/bayesrays/uncertainty.py   ComputeUncertainty.find_uncertainty :44-90 (the whole method, bound to an object that
                                          holds the three attributes it reads: aabb, lod, device)
    fruit_nerf/bayesrays/utils.py         find_grid_indices :18-41, normalize_point_coords :6-15 (whole functions)

Inputs, all seeded: rays (origins, directions, bin edges), ``points = o + d (start + end) / 2`` [R,S,3], a leaf ``offsets``
[R,S,3] of zeros (the deformation field is initialised to zero) and ``rgb = s.repeat(1, 3)`` with ``s`` [R,1] a closed-form
function of the offsets, ``s_r = sum_s tanh(<A_rs, offset_rs> + b_rs) + (sum_s <B_rs, offset_rs>)^2 / 2`` -- its gradient at
zero, ``A_rs (1 - tanh(b_rs)^2)``, is dense, of both signs and different for every sample.  Stored: the rays, that per-sample
gradient (what ``find_uncertainty`` reads from ``offsets.grad``) and the Hessian it returns.  Arrays only.

Cases: lod 3 and 4, contraction on and off, (R, S) = (70, 48) and (5, 5).  With contraction off rays run past the box, so the
fixture holds deselected samples.  The generator ASSERTS, per case, that some (ray, index) pair is fed by two different
geometric vertices (the reference's stride-L indexing aliases) and that some pair is fed by more than one sample.
"""

import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
try:
    import make_golden_bayesrays as G
finally:
    sys.path.pop(0)

SHAPES = ((70, 48), (5, 5))
LODS = (3, 4)
AABB = G.AABB
SEED = 3


def available() -> bool:
    return G.available() and os.path.exists(f"{G.BAYES}/uncertainty.py")


def extract_method(path, cls, name, namespace):
    """exec the FunctionDef `name` of class `cls` of the module at `path` (and nothing else of it) inside `namespace`."""
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == name:
                    exec(compile(ast.Module(body=[sub], type_ignores=[]), path, "exec"), namespace)
                    return namespace[name]
    raise RuntimeError(f"{path}: {cls}.{name} not found")


def rays(R, S, g):
    """Origins on a shell around the box looking inwards with some scatter, and bin edges [R, S + 1] from 0.05 to 2.5-5: the
    rays cross the box and leave it again (deselected samples without contraction).  Rays 0 and 1 are placed by hand."""
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    o = -d * (1.2 + 0.8 * torch.rand(R, 1, generator=g)) + (torch.rand(R, 3, generator=g) - 0.5) * 0.6
    o[:, 1] += 0.5  # the box's centre
    d = torch.nn.functional.normalize(d + 0.15 * torch.randn(R, 3, generator=g), dim=-1)
    width = torch.rand(R, S, generator=g) + 0.3
    bins = torch.cat([torch.zeros(R, 1), torch.cumsum(width, -1)], -1)
    bins = 0.05 + bins / bins[:, -1:] * (torch.rand(R, 1, generator=g) * 2.5 + 2.5)
    # ray 0 runs up the z axis through one (x, y) column of cells from far below the box to far above it: the top vertex
    # (a, b, L) of the column and the bottom vertex (a, b + 1, 0) of its neighbour have the same literal index, with and
    # without contraction, at both lods.  Sample midpoints at z = -5, -1.875, 0.375, 1.875, 4.625 when S = 5.
    o[0], d[0] = torch.tensor((0.1, 0.6, -6.0)), torch.tensor((0.0, 0.0, 1.0))
    bins[0] = torch.tensor((0.0, 2.0, 6.25, 6.5, 9.25, 12.0)) if S == 5 else torch.linspace(0.0, 12.0, S + 1)
    # ray 1 starts inside the box and steps by 0.1: neighbouring samples share cells at either lod
    o[1], bins[1] = torch.tensor((0.2, 0.4, -0.3)), torch.linspace(0.0, 0.1 * S, S + 1)
    return o, d, bins


def check_case(ns, points, aabb, distortion, lod, key):
    """The two properties every case must exercise (counted on the reference's own indices and coefficients)."""
    inds, coefs = ns["find_grid_indices"](points, aabb, distortion, lod, "cpu")
    R, S = points.shape[:2]
    L = 2 ** lod
    pos, _ = ns["normalize_point_coords"](points, aabb, distortion)
    cell = torch.floor(pos.view(-1, 3) * L).long()
    ray = torch.arange(R)[:, None].repeat(1, S).flatten()
    live = coefs > 0
    feeds = {}   # (ray, index) -> set of geometric vertices / set of samples
    for c in range(8):
        cx, cy, cz = (c >> 2) & 1, (c >> 1) & 1, c & 1
        vert = torch.stack([cell[:, 0] + cx, cell[:, 1] + cy, cell[:, 2] + cz], -1)
        for n in torch.nonzero(live[c]).flatten().tolist():
            v, s = feeds.setdefault((int(ray[n]), int(inds[c, n])), (set(), set()))
            v.add(tuple(vert[n].tolist()))
            s.add(n)
    aliased = sum(1 for v, _ in feeds.values() if len(v) > 1)
    shared = sum(1 for _, s in feeds.values() if len(s) > 1)
    if aliased == 0:
        raise AssertionError(f"{key}: no (ray, index) pair is fed by two geometric vertices: pick another seed")
    if shared == 0:
        raise AssertionError(f"{key}: no (ray, index) pair is fed by more than one sample: pick another seed")
    return aliased, shared, int((~live.any(0)).sum())


def build(seed=SEED, stats=None):
    ns = {"torch": torch, "SceneBox": G.SceneBox}
    G.extract(f"{G.BAYES}/utils.py", {"normalize_point_coords", "find_grid_indices"}, ns)
    find_uncertainty = extract_method(f"{G.BAYES}/uncertainty.py", "ComputeUncertainty", "find_uncertainty", ns)

    g = torch.Generator().manual_seed(4100 + seed)
    aabb = torch.tensor(AABB)
    out = {"aabb": np.array(AABB, dtype=np.float32), "lods": np.array(LODS, dtype=np.int64),
           "shapes": np.array(SHAPES, dtype=np.int64)}
    for si, (R, S) in enumerate(SHAPES):
        o, d, bins = rays(R, S, g)
        A = torch.randn(R, S, 3, generator=g)
        b = torch.randn(R, S, generator=g)
        B = torch.randn(R, S, 3, generator=g)
        out[f"s{si}/origins"], out[f"s{si}/directions"], out[f"s{si}/bins"] = o.numpy(), d.numpy(), bins.numpy()
        starts, ends = bins[:, :-1, None], bins[:, 1:, None]
        points = o[:, None, :] + d[:, None, :] * (starts + ends) / 2  # Frustums.get_positions
        first = True
        for lod in LODS:
            for contraction in (0, 1):
                distortion = G.linf_contraction if contraction else None
                offsets = torch.zeros(R, S, 3, requires_grad=True)
                s = (torch.tanh((A * offsets).sum(-1) + b).sum(-1) + 0.5 * (B * offsets).sum((-1, -2)) ** 2)[:, None]
                me = G.Record(aabb=aabb, lod=lod, device="cpu")
                grad = torch.autograd.grad(s.sum(), offsets, retain_graph=True)[0]
                hessian = find_uncertainty(me, points, offsets, s.repeat(1, 3), distortion)
                closed = A * (1 - torch.tanh(b) ** 2)[..., None]
                assert torch.allclose(grad, closed, rtol=1e-6, atol=1e-7)
                if first:
                    out[f"s{si}/gradients"] = grad.numpy()
                    first = False
                key = f"lod{lod}/c{contraction}/s{si}"
                out[f"{key}/hessian"] = hessian.detach().numpy()
                got = check_case(ns, points, aabb, distortion, lod, key)
                if stats is not None:
                    stats[key] = got + (int((hessian != 0).sum()),)
    return out


def main():
    stats = {}
    out = build(stats=stats)
    path = os.path.join(HERE, "bayesrays_hessian.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(out), "arrays")
    for k, (aliased, shared, dead, nz) in stats.items():
        print(k, "pairs fed by two vertices", aliased, "by several samples", shared, "deselected samples", dead,
              "non-zero vertices", nz, "max H", float(out[f"{k}/hessian"].max()))


if __name__ == "__main__":
    main()
