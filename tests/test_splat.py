"""``cn_splat_points`` / ``ops.splat_points`` (``csrc/splat.hip``): the z-tested point splat behind the result views, against
the float64 restatement of its geometry in ``tests/_splat_ref.py``."""

import ctypes as C

import numpy as np
import pytest

import _splat_ref as REF

H, W = 64, 96  # not square: a row / column swap shows
NEAR = 0.05


def _cam(R=np.eye(3), t=(0.0, 0.0, 0.0), fx=10.0, fy=10.0, cx=0.0, cy=0.0):
    return np.concatenate([np.concatenate([np.asarray(R, float), np.asarray(t, float).reshape(3, 1)], 1).reshape(-1), [fx, fy, cx, cy]])


# ------------------------------------------------------------------------------------------------------------------
# CPU tier
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import cropnerf_amd
    from cropnerf_amd import _lib

    if not _lib.LIB_PATH.exists():
        cropnerf_amd.build_library()
    return _lib.load()


def test_null_arguments_are_refused_on_the_host(lib):
    rc = lib.cn_splat_points(None, None, 0, None, 1, 4, 4, 2, 0.0, 0, None, None, None, None, 0, None)
    assert rc == -1
    assert b"cn_splat_points" in lib.cn_last_error()
    # the other host-side refusals, each before any HIP call (the pointers are never dereferenced)
    p = C.c_void_p(64)
    for kwargs in (dict(point_size=0), dict(num_points=1 << 32), dict(workspace_bytes=4 * 4 * 8 - 1)):
        a = dict(num_points=3, point_size=2, workspace_bytes=4 * 4 * 8)
        a.update(kwargs)
        rc = lib.cn_splat_points(p, p, a["num_points"], p, 1, 4, 4, a["point_size"], 0.0, 0, p, None, None, p,
                                 a["workspace_bytes"], None)
        assert rc == -1 and b"cn_splat_points" in lib.cn_last_error(), kwargs


def test_workspace_is_eight_bytes_per_pixel_per_frame(lib):
    assert lib.cn_splat_workspace_bytes(3, 64, 96) == 3 * 64 * 96 * 8
    assert lib.cn_splat_workspace_bytes(0, 64, 96) == 0


@pytest.mark.parametrize("point_size, rows, cols", [
    (1, [3], [5]),                 # u = 5.3: 4.8 <= j < 5.8; v = 2.6: 2.1 <= i < 3.1
    (2, [2, 3], [5, 6]),           # 4.3 <= j < 6.3; 1.6 <= i < 3.6
    (3, [2, 3, 4], [4, 5, 6]),     # 3.8 <= j < 6.8; 1.1 <= i < 4.1
])
def test_reference_footprint_is_the_one_the_definition_lists(point_size, rows, cols):
    pts = np.array([[0.53, 0.26, 1.0]])  # u = 10 * 0.53 = 5.3, v = 2.6
    img, idx, dep, _ = REF.splat(pts, np.array([[9, 8, 7]], np.uint8), [_cam()], 8, 12, point_size, 0.01, (1, 2, 3))
    want = np.full((8, 12), -1)
    want[np.ix_(rows, cols)] = 0
    assert np.array_equal(idx[0], want)
    assert np.array_equal(img[0][want == 0], np.tile([9, 8, 7], (len(rows) * len(cols), 1)))
    assert np.array_equal(img[0][want < 0], np.tile([1, 2, 3], (8 * 12 - len(rows) * len(cols), 1)))
    assert np.all(dep[0][want == 0] == 1.0) and np.all(np.isinf(dep[0][want < 0]))


def test_reference_nearer_point_wins_and_equal_depth_goes_to_the_lower_index():
    # three points on one pixel: 1 and 2 coincide, in front of 0
    pts = np.array([[1.06, 0.52, 2.0], [0.53, 0.26, 1.0], [0.53, 0.26, 1.0]])
    cols = np.array([[10, 0, 0], [0, 20, 0], [0, 0, 30]], np.uint8)
    img, idx, dep, margin = REF.splat(pts, cols, [_cam()], 8, 12, 1, 0.01)
    assert idx[0, 3, 5] == 1 and dep[0, 3, 5] == 1.0 and tuple(img[0, 3, 5]) == (0, 20, 0)
    assert (idx[0] >= 0).sum() == 1
    assert margin[0, 3, 5] == pytest.approx(1.0)  # the runner-up that is no duplicate of the winner is twice as far
    img, idx, _, _ = REF.splat(pts[::-1].copy(), cols[::-1].copy(), [_cam()], 8, 12, 1, 0.01)
    assert idx[0, 3, 5] == 0 and tuple(img[0, 3, 5]) == (0, 0, 30)  # again the lower index of the equal pair
    # behind the near plane: dropped; a footprint entirely outside the image: nothing
    _, idx, _, _ = REF.splat(np.array([[0.0, 0.0, 0.01], [0.0, 0.0, -1.0], [5.0, 0.0, 1.0]]), cols, [_cam()], 8, 12, 3, 0.01)
    assert (idx >= 0).sum() == 0


# ------------------------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------------------------

def _orbit(num_frames=5):
    from cropnerf_amd.segmentation import video_renderer as VR

    return VR.pack_cameras(VR.orbit_cameras([0.0, 0.0, 0.0], num_frames), VR.default_intrinsics(W, H))  # float32 [F,16]


_CLOUD = {}


def _cloud(point_size):
    """The cloud of the issue, the points a float32 / float64 disagreement could decide removed (see the test), and the
    float64 reference of what is left -- computed once per point size."""
    if point_size in _CLOUD:
        return _CLOUD[point_size]
    rng = np.random.default_rng(7)
    inner = rng.uniform(-0.45, 0.45, size=(5000, 3))
    outer = rng.uniform(-1.5, 1.5, size=(500, 3))
    pts = np.concatenate([inner, outer, inner[:100]]).astype(np.float32)
    cols = rng.integers(0, 256, size=(len(pts), 3), dtype=np.uint8)
    cols[-100:] = cols[:100] ^ 0x55  # the repeated points differ from their originals in colour only
    cams = _orbit()
    keep = np.ones(len(pts), bool)
    h = point_size / 2.0
    near_int = lambda x: np.abs(x - np.rint(x)) < 1e-2
    for cam in cams:
        cz, u, v = REF.project(pts, cam)
        front = cz > NEAR
        edge = near_int(u - h) | near_int(u + h) | near_int(v - h) | near_int(v + h)
        keep &= ~((front & edge) | (np.abs(cz - NEAR) < 1e-3))
    survive = keep.mean()
    pts, cols = np.ascontiguousarray(pts[keep]), np.ascontiguousarray(cols[keep])
    ref = REF.splat(pts, cols, cams, H, W, point_size, NEAR)
    _CLOUD[point_size] = (pts, cols, cams, survive, ref)
    return _CLOUD[point_size]


@pytest.mark.gpu
@pytest.mark.parametrize("point_size", [1, 2, 3])
def test_splat_matches_reference(point_size):
    """Five orbit frames of 64 x 96, two frames per launch (a chunk boundary and a short last chunk), near plane 0.05, over
    5 000 points in +-0.45, 500 in +-1.5 (behind a camera, nearer than the near plane, straddling the border, missing the
    image) and the first 100 again with other colours; N is no multiple of 64.

    float32 on the device and float64 here may disagree where a footprint edge sits on a pixel boundary or where two depths
    nearly tie.  Those cases are removed from the INPUT: every point for which, in any frame, one of u +- s/2, v +- s/2 lies
    within 1e-2 px of an integer or c.z within 1e-3 of the near plane is dropped before either side runs (duplicates go with
    their originals: same coordinates, same verdict), and pixels whose two nearest candidates differ by less than 1e-4
    relative in depth are left out of the comparison -- exact duplicates excepted, where the lower index must win.  Both
    exclusions are capped: at least 75 % of the points survive, at most 0.5 % of the covered pixels are left out."""
    import torch

    from cropnerf_amd import ops

    pts, cols, cams, survive, (r_img, r_idx, r_dep, margin) = _cloud(point_size)
    n = len(pts)
    print(f"point_size {point_size}: {n} points ({survive:.1%} survive)")
    assert survive >= 0.75 and n % 64 != 0
    # the reference sees every kind of point the cloud was built for
    kinds = dict(behind=0, near=0, straddle=0, miss=0)
    for cam in cams:
        alive, j0, j1, i0, i1, cz = REF.footprints(pts, cam, H, W, point_size, NEAR)
        kinds["behind"] += int((cz <= 0).sum())
        kinds["near"] += int(((cz > 0) & (cz <= NEAR)).sum())
        inside = alive & (j1 >= 0) & (j0 <= W - 1) & (i1 >= 0) & (i0 <= H - 1)
        kinds["miss"] += int((alive & ~inside).sum())
        kinds["straddle"] += int((inside & ((j0 < 0) | (j1 > W - 1) | (i0 < 0) | (i1 > H - 1))).sum())
    _, counts = np.unique(pts, axis=0, return_counts=True)
    n_dup = int((counts > 1).sum())  # the repeated points that survived, at the end of the cloud as they were built
    assert n_dup > 0 and np.array_equal(pts[n - n_dup:], pts[:n_dup]) and counts.max() == 2
    dup_wins = int((r_idx >= n - n_dup).sum())
    orig_wins = int(((r_idx >= 0) & (r_idx < n_dup)).sum())
    print(kinds, "repeated points:", n_dup, "pixels won by an original / by its repeat:", orig_wins, dup_wins)
    if point_size == 1:  # a footprint of one pixel is inside the image or outside it: nothing can straddle the border
        assert kinds.pop("straddle") == 0
    assert all(v > 0 for v in kinds.values()), kinds
    assert orig_wins > 0 and dup_wins == 0  # a repeated point never beats its original (the lower index)
    covered = r_idx >= 0
    compare = ~(covered & (margin < 1e-4))
    left_out = (~compare).sum() / covered.sum()
    print(f"covered {covered.mean():.1%} of the pixels, {left_out:.3%} of them left out")
    assert left_out <= 0.005

    dev = "cuda"
    img, idx, dep = ops.splat_points(torch.from_numpy(pts).to(dev), torch.from_numpy(cols).to(dev), torch.from_numpy(cams).to(dev),
                                     H, W, point_size, NEAR, (255, 255, 255), return_index=True, return_depth=True,
                                     max_frames_per_launch=2)
    torch.cuda.synchronize()
    img, idx, dep = img.cpu().numpy(), idx.cpu().numpy(), dep.cpu().numpy()
    assert img.shape == (5, H, W, 3) and idx.shape == (5, H, W) and dep.shape == (5, H, W)
    print("index mismatches on compared pixels:", int((idx != r_idx)[compare].sum()))
    assert np.array_equal(idx[compare], r_idx[compare])
    assert np.array_equal(img[compare], r_img[compare])  # the winner's colour, or the background
    hit = compare & covered
    rel = np.abs(dep[hit].astype(np.float64) - r_dep[hit]) / r_dep[hit]
    print("max relative depth error:", float(rel.max()))
    assert rel.max() <= 1e-5
    assert np.all(np.isposinf(dep[compare & ~covered]))


@pytest.mark.gpu
def test_splat_edge_cases():
    import torch

    from cropnerf_amd import ops

    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cams = _orbit()
    # no points: background everywhere
    img, idx, dep = ops.splat_points(torch.empty(0, 3, device=dev), torch.empty(0, 3, dtype=torch.uint8, device=dev), t(cams), H, W,
                                     background=(10, 20, 30), return_index=True, return_depth=True)
    assert img.shape == (5, H, W, 3) and bool((img == torch.tensor([10, 20, 30], dtype=torch.uint8, device=dev)).all())
    assert bool((idx == -1).all()) and bool(torch.isposinf(dep).all())
    # one point of size 3 centred on pixel (0, 0): rows and columns -1 .. 1, of which the 2 x 2 corner survives clipping
    one = _cam(fx=20.0, fy=20.0).astype(np.float32)[None]
    img, idx = ops.splat_points(t(np.array([[0.0, 0.0, 1.0]], np.float32)), t(np.array([[1, 2, 3]], np.uint8)), t(one), H, W, 3,
                                return_index=True)
    want = np.full((H, W), -1)
    want[:2, :2] = 0
    assert np.array_equal(idx[0].cpu().numpy(), want)
    assert np.array_equal(img[0, :2, :2].cpu().numpy().reshape(-1, 3), np.tile([1, 2, 3], (4, 1)))
    assert bool((img[0, 2:] == 255).all()) and bool((img[0, :, 2:] == 255).all())
    # chunked = unchunked; reversed point order = the same picture, indices mapped back (no exact duplicates in this cloud)
    rng = np.random.default_rng(11)
    pts = rng.uniform(-0.45, 0.45, size=(3001, 3)).astype(np.float32)
    cols = rng.integers(0, 256, size=(3001, 3), dtype=np.uint8)
    assert len(np.unique(pts, axis=0)) == len(pts)
    whole = ops.splat_points(t(pts), t(cols), t(cams), H, W, 2, NEAR, return_index=True, return_depth=True)
    for per_launch in (1, 2):
        parts = ops.splat_points(t(pts), t(cols), t(cams), H, W, 2, NEAR, return_index=True, return_depth=True,
                                 max_frames_per_launch=per_launch)
        assert all(torch.equal(a, b) for a, b in zip(whole, parts)), per_launch
    rev = ops.splat_points(t(pts[::-1]), t(cols[::-1]), t(cams), H, W, 2, NEAR, return_index=True, return_depth=True)
    back = torch.where(rev[1] >= 0, len(pts) - 1 - rev[1], rev[1])
    assert torch.equal(whole[0], rev[0]) and torch.equal(whole[1], back) and torch.equal(whole[2], rev[2])
    assert int((whole[1] >= 0).sum()) > 0.1 * whole[1].numel()
