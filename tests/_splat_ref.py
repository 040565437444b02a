"""float64 restatement of the point-splat geometry of ``include/cropnerf_hip.h`` (``cn_splat_points``), for
``tests/test_splat.py``:

* camera space ``c = R p + t`` (x right, y down, z forward); a point with ``c.z <= near_plane`` is dropped;
* ``u = fx c.x / c.z + cx``, ``v = fy c.y / c.z + cy``, pixel centres at integer coordinates;
* the point covers the columns ``ceil(u - s/2) .. ceil(u + s/2) - 1`` and the rows alike from ``v``, clipped to the image;
* per pixel the smallest ``c.z`` wins, ties go to the smallest point index.
"""

import numpy as np


def project(points, camera):
    """One camera row [16] -> (cz, u, v) per point, float64.  u, v are NaN where cz <= 0."""
    cam = np.asarray(camera, dtype=np.float64)
    Rt = cam[:12].reshape(3, 4)
    c = np.asarray(points, dtype=np.float64) @ Rt[:, :3].T + Rt[:, 3]
    cz = c[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(cz > 0, cam[12] * c[:, 0] / cz + cam[14], np.nan)
        v = np.where(cz > 0, cam[13] * c[:, 1] / cz + cam[15], np.nan)
    return cz, u, v


def footprints(points, camera, height, width, point_size, near_plane):
    """Per point of one frame: (alive [N] bool, j0, j1, i0, i1 [N] int64, UNCLIPPED, inclusive; garbage where not alive)."""
    cz, u, v = project(points, camera)
    alive = cz > near_plane
    h = point_size / 2.0
    uu, vv = np.where(alive, u, 0.0), np.where(alive, v, 0.0)
    j0, j1 = np.ceil(uu - h).astype(np.int64), np.ceil(uu + h).astype(np.int64) - 1
    i0, i1 = np.ceil(vv - h).astype(np.int64), np.ceil(vv + h).astype(np.int64) - 1
    return alive, j0, j1, i0, i1, cz


def candidates(points, camera, height, width, point_size, near_plane):
    """Every (pixel, point) pair of one frame after clipping: (pixel = row * width + col, point index, cz)."""
    alive, j0, j1, i0, i1, cz = footprints(points, camera, height, width, point_size, near_plane)
    pix, idx = [], []
    ids = np.arange(len(cz))
    for di in range(point_size + 1):  # a footprint is point_size wide; one more for a float64 edge case
        for dj in range(point_size + 1):
            r, c = i0 + di, j0 + dj
            ok = alive & (r <= i1) & (c <= j1) & (r >= 0) & (r < height) & (c >= 0) & (c < width)
            pix.append((r * width + c)[ok])
            idx.append(ids[ok])
    pix, idx = np.concatenate(pix), np.concatenate(idx)
    return pix, idx, cz[idx]


def splat(points, colors, cameras, height, width, point_size, near_plane, background=(255, 255, 255)):
    """The whole op in float64: images [F,H,W,3] uint8, index [F,H,W] int64 (-1 = empty), depth [F,H,W] float64 (+inf = empty)
    and ``margin`` [F,H,W]: the relative depth gap between the winner and the nearest candidate that is not an exact
    duplicate of it (same coordinates), +inf where there is none."""
    points = np.asarray(points)
    F = len(cameras)
    images = np.empty((F, height, width, 3), np.uint8)
    images[...] = np.asarray(background, np.uint8)
    index = np.full((F, height * width), -1, np.int64)
    depth = np.full((F, height * width), np.inf)
    margin = np.full((F, height * width), np.inf)
    _, group = np.unique(points, axis=0, return_inverse=True)  # exact duplicates share a group
    group = group.reshape(-1)
    for f in range(F):
        pix, idx, cz = candidates(points, cameras[f], height, width, point_size, near_plane)
        if not len(pix):
            continue
        order = np.lexsort((idx, cz, pix))  # by pixel, then depth, then point index
        pix, idx, cz = pix[order], idx[order], cz[order]
        first = np.r_[True, pix[1:] != pix[:-1]]
        index[f, pix[first]] = idx[first]
        depth[f, pix[first]] = cz[first]
        # the runner-up: the first candidate of the pixel that is not a duplicate of the winner
        start = np.flatnonzero(first)
        seg = np.cumsum(first) - 1
        other = group[idx] != group[idx[start[seg]]]
        rel = np.where(other, (cz - cz[start[seg]]) / cz[start[seg]], np.inf)
        np.minimum.at(margin[f], pix, rel)
        img = images[f].reshape(-1, 3)
        img[pix[first]] = np.asarray(colors)[idx[first]]
    return images, index.reshape(F, height, width), depth.reshape(F, height, width), margin.reshape(F, height, width)
