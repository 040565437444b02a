"""cn_splat_points at the size the result views run at: 16 frames of 1280 x 720 over 10^7 points clumped like the C4 export's
kept points (thin spherical caps around an orbit of cameras, the cloud of tools/knn_probe.py), timed with HIP events --
median of LAUNCHES launches after warm-up -- for the library as built and for a variant with the pre-test load compiled out,
the two alternating in one process:

    VARIANT_SRC=splat bash tools/build_variant.sh nopretest -DCN_SPLAT_NO_PRETEST
    python tools/splat_probe.py [N]

Profiling aid, not a test."""
import ctypes as C, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cropnerf_amd import _lib as L
from cropnerf_amd.segmentation import video_renderer as VR

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
F, H, W, SIZE, NEAR = 16, 720, 1280, 2, 1e-3
LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", 12)), 3
variant_path = os.environ.get("SPLAT_VARIANT_LIB", os.path.join(ROOT, "tools", "scratch", "variants", "libcropnerf_nopretest.so"))
if not os.path.exists(variant_path):
    raise SystemExit(f"{variant_path} not found: build it with the command in this file's docstring")
variant = C.CDLL(variant_path)
for name in ("cn_splat_workspace_bytes", "cn_splat_points"):
    getattr(variant, name).restype, getattr(variant, name).argtypes = L.SIGNATURES[name]
variant.cn_last_error.restype = C.c_char_p
libs = {"pretest": L.load(), "no_pretest": variant}

g = torch.Generator(device="cuda").manual_seed(0)
cam = torch.randint(0, 100, (N,), device="cuda", generator=g)
ang = cam.float() * (2 * 3.14159265 / 100)
centre = torch.stack([0.8 * ang.cos(), 0.8 * ang.sin(), 0.2 * (cam % 2).float() - 0.1], -1)
d = torch.nn.functional.normalize(-centre + 0.35 * torch.randn(N, 3, device="cuda", generator=g), dim=-1)
pts = (centre + d * (0.75 + 0.003 * torch.randn(N, 1, device="cuda", generator=g))).contiguous()
cols = torch.randint(0, 256, (N, 3), device="cuda", generator=g).to(torch.uint8).contiguous()
# the reference's orbit, far enough out to see the whole cloud (its own radius of 1 would sit inside this one)
cams = torch.from_numpy(VR.pack_cameras(VR.orbit_cameras(pts.mean(0).cpu().numpy(), F, radius=2.2, height=1.0),
                                        VR.default_intrinsics(W, H))).cuda()
images = torch.empty(F, H, W, 3, dtype=torch.uint8, device="cuda")
index = torch.empty(F, H, W, dtype=torch.int32, device="cuda")
ws = torch.empty(libs["pretest"].cn_splat_workspace_bytes(F, H, W), dtype=torch.uint8, device="cuda")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr())


def launch(lib):
    rc = lib.cn_splat_points(p(pts), p(cols), N, p(cams), F, H, W, SIZE, NEAR, 0xFFFFFF, p(images), p(index), None, p(ws),
                             ws.numel(), stream)
    assert rc == 0, lib.cn_last_error()


times = {k: [] for k in libs}
results = {}
for it in range(WARMUP + LAUNCHES):
    for name, lib in libs.items():  # alternating: both see the same clocks and the same neighbours on the machine
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch(lib)
        b.record()
        b.synchronize()
        if it >= WARMUP:
            times[name].append(a.elapsed_time(b))
        elif it == 0:
            results[name] = (images.clone(), index.clone())
assert torch.equal(results["pretest"][0], results["no_pretest"][0]) and torch.equal(results["pretest"][1], results["no_pretest"][1])
covered = float((index >= 0).float().mean())
out = {"points": N, "frames": F, "image": [H, W], "point_size": SIZE, "launches": LAUNCHES, "covered_pixel_fraction": round(covered, 4),
       "projections": N * F}
for name, t in times.items():
    med = statistics.median(t)
    out[name] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                 "projections_per_sec": N * F / (med * 1e-3)}
print(json.dumps(out))
