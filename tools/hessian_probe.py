"""The BayesRays Hessian stage at a training batch's size: R rays x 48 samples of the default method, lod 8.

    python tools/hessian_probe.py 4096 [launches]     # run it under rocprofv3 --kernel-trace --stats, in a run of its own

Each launch round: cn_semantics_density_gradient, cn_field_density_position_gradient, cn_hessian_accumulate and, for comparison,
the parent route to the same position gradient -- cn_field_backward_ex with zero colour / semantic gradients into throw-away
gradient buffers.  Prints one JSON line with event-timed milliseconds per launch (medians) and the two routes' agreement.
The samples are the default method's own: the proposal sampler's 48 final bins on the P-rand scene, contraction on."""
import json, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cropnerf_amd import config as PC, ops, synthetic
from cropnerf_amd.fruit_nerf.fruit_nerf import FruitModel, Semantics
from cropnerf_amd.rays import SceneBox

LOD = 8
R = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 20
cfg = PC.FruitNerfModelConfig()
params = synthetic.p_rand(cfg.field_spec(100), cfg.proposal_specs(), seed=0, device="cuda")
m = FruitModel(cfg, SceneBox(torch.tensor(synthetic.SCENE_AABB)), 100, {"semantics": Semantics()}, device="cuda",
               test_mode="test", params=params)
g = torch.Generator().manual_seed(0)
d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
o = (-d * 2.5 + (torch.rand(R, 3, generator=g) - 0.5)).cuda().contiguous()
d = d.cuda().contiguous()
nears, fars = torch.full((R, 1), 0.05, device="cuda"), torch.full((R, 1), 6.0, device="cuda")
scene = ops.scene_struct(m.scene_box.aabb, True)
eu = ops.proposal_sample(m.proposal_networks, scene, o, d, nears, fars, cfg.num_proposal_samples_per_ray, 48)["euclidean_bins"]
starts, ends = eu[:, :-1].contiguous(), eu[:, 1:].contiguous()
fo = ops.field_eval(m.field, scene, o, d, None, starts, ends)
grads = {k: torch.zeros_like(v) for k, v in params.items()}
gh = ops.FieldHandle(grads, m.field.spec).enable_scatter_scratch(R * 48)
cam = torch.zeros(R, dtype=torch.int64, device="cuda")
zero3, zero1 = torch.zeros(R, 48, 3, device="cuda"), torch.zeros(R, 48, device="cuda")
d_pos_bwd = torch.empty(R, 48, 3, device="cuda")
hessian = torch.zeros((2 ** LOD + 1) ** 3, device="cuda")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


ms = {"semantics_density_gradient": [], "field_density_position_gradient": [], "hessian_accumulate": [], "field_backward_ex": []}
for i in range(LAUNCHES + 2):
    t1, k1 = timed(lambda: ops.semantics_density_gradient(starts, ends, fo["density"], fo["semantics"]))
    t2, k2 = timed(lambda: ops.field_density_position_gradient(m.field, scene, o, d, starts, ends, k1["d_density"]))
    t3, _ = timed(lambda: ops.hessian_accumulate(o, d, starts, ends, k2["d_positions"], scene, LOD, hessian))
    t4, _ = timed(lambda: ops.field_backward(m.field, gh, scene, o, d, cam, starts, ends, k1["d_density"], zero3, zero1,
                                             d_positions=d_pos_bwd))
    if i >= 2:  # two warm-up rounds
        for k, t in zip(ms, (t1, t2, t3, t4)):
            ms[k].append(t)
rel = float((k2["d_positions"] - d_pos_bwd).norm() / d_pos_bwd.norm())
print(json.dumps({"rays": R, "samples": 48, "lod": LOD, "launches": LAUNCHES,
                  "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                  "rel_l2_position_gradient_vs_backward": rel, "hessian_max": float(hessian.max()),
                  "hessian_nonzero": int((hessian != 0).sum())}))
