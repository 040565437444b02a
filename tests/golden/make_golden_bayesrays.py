#!/usr/bin/env python
"""Golden vectors of the BayesRays consumer, produced by EXECUTING the reference's own code (build container only).

    python tests/golden/make_golden_bayesrays.py      ->  tests/golden/bayesrays_functions.npz

Same method as ``make_golden_reference.py``: the reference's files are read with ``ast``, definitions and statement blocks are
taken out of modules that cannot be imported here (they import nerfstudio / nerfacc at the top) and executed unchanged on
seeded tensors in a namespace that holds only what they name:

    fruit_nerf/bayesrays/utils.py                normalize_point_coords :6-15, find_grid_indices :18-41 (whole functions)
    fruit_nerf/bayesrays/output_uncertainty.py   get_uncertainty :19-30 (whole function, on an object holding the attributes it
                                                 reads); statement blocks of get_output_nerfacto_new: :36-42 (the table
                                                 un = 1 / (H / N + lambda) and the two bounds), :60 (the density mask),
                                                 :65-70 (the composited, clipped and normalised uncertainty)

Stand-ins for the two upstream names those functions call: ``SceneBox.get_normalized_positions`` is nerfstudio's
``(p - aabb[0]) / (aabb[1] - aabb[0])`` and the ``distortion`` callable is nerfstudio's ``SceneContraction(order=inf)``.

The fixture holds arrays only (inputs and outputs); nothing of the reference's text is stored.  ``build()`` returns the
arrays; ``tests/test_bayesrays_host.py`` regenerates them when the reference tree is present.

Cases: lod 3 and 4; 67 rays x 48 samples and 5 rays x 70 samples (neither a multiple of 64); box normalisation and L-inf
contraction; rays 0-3 of every shape walk the axes and a diagonal on a 1/16 lattice, so their samples fall exactly on cell
faces and vertices, on normalised 0 and 1 of the box, and outside it; the other rays are random and reach beyond radius 1.
The Hessian is log-uniform over eleven decades with exact zeros and values >= 1000 N.  Two filter thresholds.  The generator
ASSERTS that no stored un_point lies within 1e-4 of a threshold * 6, so the masks can be compared exactly.
"""

import ast
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CROPNERF_REFERENCE", "/root/reference/crop_nerf")  # as make_golden_reference.py
BAYES = f"{REF}/fruit_nerf/bayesrays"

N_RAYS_DATASET = 1000 * 4096  # run_viewer_u.py:376
SHAPES = ((67, 48), (5, 70))
LODS = (3, 4)
THRESHOLDS = (0.5, 0.2)
AABB = ((-1.0, -0.5, -2.0), (1.0, 1.5, 2.0))  # power-of-two extents: the box normalisation of lattice points is exact
MARGIN = 1e-4
SEED = 8  # seeds 0-7 each put an un_point within MARGIN of 0.5 * 6


def available() -> bool:
    return os.path.exists(f"{BAYES}/output_uncertainty.py") and os.path.exists(f"{BAYES}/utils.py")


def extract(path, names, namespace):
    """exec the FunctionDef nodes `names` of the module at `path` (and nothing else of it) inside `namespace`."""
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    found = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
            found.append(node.name)
    missing = set(names) - set(found)
    if missing:
        raise RuntimeError(f"{path}: functions not found: {sorted(missing)}")
    return namespace


def statement_block(path, first, last):
    """A code object of the statements of the module at `path` between source lines `first` and `last` (inclusive), taken from
    the innermost statement list that holds them -- the reference's own AST nodes, nothing edited."""
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)

    def pick(body):
        sel = [n for n in body if first <= n.lineno and n.end_lineno <= last]
        if sel:
            return sel
        for n in body:
            if n.lineno <= first and last <= n.end_lineno:
                for field in ("body", "orelse", "finalbody"):
                    sub = getattr(n, field, None)
                    if isinstance(sub, list) and sub and isinstance(sub[0], ast.stmt):
                        got = pick(sub)
                        if got:
                            return got
        return []

    sel = pick(tree.body)
    if not sel:
        raise RuntimeError(f"{path}: no statements between lines {first} and {last}")
    return compile(ast.Module(body=sel, type_ignores=[]), path, "exec")


class Record:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class SceneBox:
    """nerfstudio ``SceneBox.get_normalized_positions``."""

    @staticmethod
    def get_normalized_positions(positions, aabb):
        aabb_lengths = aabb[1] - aabb[0]
        return (positions - aabb[0]) / aabb_lengths


def linf_contraction(x):
    """nerfstudio ``SceneContraction(order=float("inf")).forward``."""
    mag = torch.linalg.norm(x, ord=float("inf"), dim=-1)[..., None]
    return torch.where(mag < 1, x, (2 - (1 / mag)) * (x / mag))


def rays(R, S, g):
    """Origins, directions, bin edges [R, S + 1] and weights [R, S] of one shape."""
    o = torch.rand(R, 3, generator=g) * 3.0 - 1.5
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    width = torch.rand(R, S, generator=g) + 0.05
    bins = torch.cat([torch.zeros(R, 1), torch.cumsum(width, -1)], -1)
    bins = bins / bins[:, -1:] * (torch.rand(R, 1, generator=g) * 4.0 + 1.0)
    # lattice rays: sample midpoints at j / 16 from the origin, along x, y, z and the diagonal
    lattice = (torch.arange(S + 1, dtype=torch.float32) - 0.5) / 16.0
    for r, (org, dr) in enumerate((((-1.25, 0.25, 0.5), (1.0, 0.0, 0.0)), ((0.3, -0.75, 0.1), (0.0, 1.0, 0.0)),
                                   ((-0.5, 0.5, -2.25), (0.0, 0.0, 2.0)), ((-1.25, -0.75, -2.25), (1.0, 1.0, 1.0)))):
        o[r], d[r], bins[r] = torch.tensor(org), torch.tensor(dr), lattice
    # weights as a compositor gives them (sum <= 1); ray 4 sees nothing at all
    sigma = torch.rand(R, S, generator=g) ** 3 * 6.0
    delta = bins[:, 1:] - bins[:, :-1]
    alpha = 1 - torch.exp(-sigma * delta)
    trans = torch.cumprod(torch.cat([torch.ones(R, 1), 1 - alpha[:, :-1]], -1), -1)
    w = alpha * trans
    w[4] = 0.0
    return o, d, bins, w


def hessian(lod, g):
    n = (2 ** lod + 1) ** 3
    h = 10.0 ** (torch.rand(n, generator=g) * 11.0 - 8.0) * N_RAYS_DATASET  # H / N in [1e-8, 1e3]
    kind = torch.rand(n, generator=g)
    h[kind < 0.08] = 0.0
    h[kind > 0.92] = 1000.0 * N_RAYS_DATASET * (1.0 + 9.0 * torch.rand(n, generator=g))[kind > 0.92]
    h[0] = 0.0  # what every deselected sample reads
    return h


def build(seed=SEED):
    ns = {"torch": torch, "SceneBox": SceneBox}
    extract(f"{BAYES}/utils.py", {"normalize_point_coords", "find_grid_indices"}, ns)
    extract(f"{BAYES}/output_uncertainty.py", {"get_uncertainty"}, ns)
    get_uncertainty = ns["get_uncertainty"]
    table_block = statement_block(f"{BAYES}/output_uncertainty.py", 36, 42)
    mask_block = statement_block(f"{BAYES}/output_uncertainty.py", 60, 60)
    comp_block = statement_block(f"{BAYES}/output_uncertainty.py", 65, 70)

    g = torch.Generator().manual_seed(2300 + seed)
    out = {"N": np.array(N_RAYS_DATASET, dtype=np.int64), "aabb": np.array(AABB, dtype=np.float32),
           "lods": np.array(LODS, dtype=np.int64), "thresholds": np.array(THRESHOLDS, dtype=np.float64),
           "shapes": np.array(SHAPES, dtype=np.int64)}
    aabb = torch.tensor(AABB)
    shapes = {}
    for si, (R, S) in enumerate(SHAPES):
        o, d, bins, w = rays(R, S, g)
        shapes[si] = (o, d, bins, w)
        out[f"s{si}/origins"], out[f"s{si}/directions"] = o.numpy(), d.numpy()
        out[f"s{si}/bins"], out[f"s{si}/weights"] = bins.numpy(), w.numpy()
        # the compositor alone, on values the lookup cannot produce: both clip ends
        cu = torch.rand(R, S, generator=g) * 13.0 - 5.0
        cw = w.clone()
        cw[0], cu[0] = 0.0, 7.0                 # sees nothing: -3 -> 0
        cw[1], cu[1] = 1.0 / S, 7.5             # weights sum to 1 on 7.5: clipped to 6 -> 1
        cw[2], cu[2] = 1.0 / S, -5.0            # clipped to -3 -> 0
        cns = {"torch": torch, "weights": cw[..., None], "un_points": cu[..., None], "min_uncertainty": -3, "max_uncertainty": 6}
        exec(comp_block, cns)
        out[f"s{si}/comp_weights"], out[f"s{si}/comp_un"] = cw.numpy(), cu.numpy()
        out[f"s{si}/comp_uncertainty"] = cns["uncertainty"].numpy()
    for lod in LODS:
        h = hessian(lod, g)
        model = Record(N=N_RAYS_DATASET, lod=lod, hessian=h)
        exec(table_block, {"self": model})
        out[f"lod{lod}/hessian"], out[f"lod{lod}/un"] = h.numpy(), model.un.numpy()
        for contraction in (0, 1):
            model.scene_box = Record(aabb=aabb)
            model.field = Record(spatial_distortion=linf_contraction if contraction else None)
            for si, (o, d, bins, w) in shapes.items():
                starts, ends = bins[:, :-1, None], bins[:, 1:, None]
                points = o[:, None, :] + d[:, None, :] * (starts + ends) / 2  # Frustums.get_positions
                un_points = get_uncertainty(model, points)
                k = f"lod{lod}/c{contraction}/s{si}"
                out[f"{k}/un_points"] = un_points[..., 0].numpy()
                density_in = w[..., None] + 1.0
                for ti, thresh in enumerate(THRESHOLDS):
                    near = (un_points - thresh * 6).abs().min().item()
                    if near < MARGIN:
                        raise AssertionError(f"{k}: an un_point lies {near:.2e} from threshold {thresh} * 6: pick another seed")
                    mns = {"torch": torch, "self": Record(filter_thresh=thresh), "max_uncertainty": 6, "un_points": un_points,
                           "field_outputs": {"density": density_in}, "FieldHeadNames": Record(DENSITY="density")}
                    exec(mask_block, mns)
                    out[f"{k}/mask{ti}"] = (mns["density"][..., 0] != 0).numpy()
                cns = {"torch": torch, "weights": w[..., None], "un_points": un_points, "min_uncertainty": -3,
                       "max_uncertainty": 6}
                exec(comp_block, cns)
                out[f"{k}/uncertainty"] = cns["uncertainty"].numpy()
    return out


def main():
    out = build()
    path = os.path.join(HERE, "bayesrays_functions.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(out), "arrays")
    for lod in LODS:
        for c in (0, 1):
            for si in range(len(SHAPES)):
                k = f"lod{lod}/c{c}/s{si}"
                u = out[f"{k}/un_points"]
                print(k, "un_points", float(u.min()), float(u.max()), "kept", [float(out[f"{k}/mask{t}"].mean()) for t in (0, 1)],
                      "uncertainty", float(out[f"{k}/uncertainty"].min()), float(out[f"{k}/uncertainty"].max()))


if __name__ == "__main__":
    main()
