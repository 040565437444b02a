"""The BayesRays consumer at a user's size: an 800 x 800 image's rays x 48 samples against a lod-8 Hessian (257^3 vertices, 68 MB).

    python tools/uncertainty_probe.py kernels   # 20 launches of each of the three kernels (run it under rocprofv3 --kernel-trace --stats)
    python tools/uncertainty_probe.py image     # ms per image: get_outputs_with_uncertainty (unfused path) next to the model's eval render

The samples are the default method's own: the proposal sampler's 48 final bins on the P-rand scene, contraction on."""
import json, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cropnerf_amd import _lib as L, config as PC, ops, synthetic
from cropnerf_amd.fruit_nerf import bayesrays as B
from cropnerf_amd.fruit_nerf.fruit_nerf import FruitModel, Semantics
from cropnerf_amd.rays import Cameras, SceneBox

LOD = 8
mode = sys.argv[1] if len(sys.argv) > 1 else "image"
cfg = PC.FruitNerfModelConfig()
params = synthetic.p_rand(cfg.field_spec(100), cfg.proposal_specs(), seed=0, device="cuda")
c2w, intr = synthetic.orbit_cameras(100)
cams = Cameras(c2w, intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 800, 800).to("cuda")
m = FruitModel(cfg, SceneBox(torch.tensor(synthetic.SCENE_AABB)), 100, {"semantics": Semantics()}, device="cuda",
               test_mode="test", params=params)
g = torch.Generator().manual_seed(0)
n = (2 ** LOD + 1) ** 3
hessian = 10.0 ** (torch.rand(n, generator=g) * 11.0 - 8.0) * B.DEFAULT_N
state = B.UncertaintyState(hessian, lod=LOD)

if mode == "kernels":
    rb = m._prepared(cams.generate_rays(3, keep_shape=False))
    o, d, nears, fars = rb.origins, rb.directions, rb.nears, rb.fars
    scene = ops.scene_struct(m.scene_box.aabb, True)
    ps = ops.proposal_sample(m.proposal_networks, scene, o, d, nears, fars, cfg.num_proposal_samples_per_ray, 48)
    eu = ps["euclidean_bins"]
    starts, ends = eu[:, :-1].contiguous(), eu[:, 1:].contiguous()
    density = torch.rand(starts.shape, device="cuda") ** 3 * 40
    weights = ops.composite(starts, ends, density, want_weights=True)["weights"]
    h = hessian.cuda()
    for _ in range(20):
        un = ops.uncertainty_table(h, B.DEFAULT_N, LOD)
        up = ops.uncertainty_lookup(o, d, starts, ends, scene, un, LOD)
        ops.uncertainty_lookup(o, d, starts, ends, scene, un, LOD, density, 3.0)
        unc = ops.uncertainty_composite(weights, up)
    torch.cuda.synchronize()
    print(json.dumps({"rays": o.shape[0], "samples": 48, "lod": LOD, "table_MB": round(n * 4 / 1e6, 1),
                      "uncertainty_mean": float(unc.mean()), "kept": float((density != 0).float().mean())}))
else:
    res = {}
    CHUNK = 1 << 17

    def unfused(i):
        flat = cams.generate_rays(i, keep_shape=False)
        return [B.get_outputs_with_uncertainty(m, flat[k:k + CHUNK], state)["uncertainty"] for k in range(0, len(flat), CHUNK)]

    for name, fn in (("eval_image_fused", lambda i: m.get_outputs_for_camera_ray_bundle(cams.generate_rays(i, keep_shape=True))),
                     ("uncertainty_image_unfused", unfused)):
        fn(3)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(5):
            fn(i)
        torch.cuda.synchronize()
        res[name] = {"ms_per_image": round((time.perf_counter() - t) / 5 * 1e3, 2)}
    res["uncertainty_image_unfused"]["rays_per_call"] = CHUNK
    print(json.dumps(res))
