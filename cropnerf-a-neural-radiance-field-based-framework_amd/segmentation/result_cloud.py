"""The labelled cloud the merger ends in -- mirror of ``crop_nerf/segmentation/merger.py:100-143`` without the window.

``create_pcd_with_labels`` (``:130-143``) paints every sub-cluster of one super-cluster with the instance label the graph
stage gave it; ``labelled_result`` does so for all of them (``main``, ``:433-443``); ``label_colors`` is the 40-entry
"tab40" lookup both of the reference's viewers colour labels with (``merger.py:105-110`` divides by the largest label
first, ``evaluation/generate_video.py:28-33`` indexes by the label itself)."""

from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

_TAB40 = None


def tab40() -> np.ndarray:
    """matplotlib's ``tab20`` colours followed by its ``tab20c`` colours, [40,3] float64 in [0,1] (taken from the installed
    matplotlib, as ``fruit_nerf/image_metrics.py`` takes "turbo")."""
    global _TAB40
    if _TAB40 is None:
        import matplotlib

        _TAB40 = np.asarray(tuple(matplotlib.colormaps["tab20"].colors) + tuple(matplotlib.colormaps["tab20c"].colors),
                            dtype=np.float64)
    return _TAB40


def label_colors(labels, normalise: bool) -> np.ndarray:
    """Labels [M] -> uint8 [M,3].  ``normalise=True``: the listed map called with the float ``labels / max(labels)`` (the
    largest label taken as 1 when it is not positive), i.e. entry ``floor(x * 40)`` with x = 1 on the last entry;
    ``normalise=False``: the map called with the integer label, i.e. that entry, clipped to 39.  Negative labels are black.
    Bytes are ``floor(colour * 255)``, what open3d writes for a float colour."""
    labels = np.asarray(labels)
    table = tab40()
    n = len(table)
    if normalise:
        lab = labels.astype(np.float64)
        top = lab.max() if lab.size else 0.0
        xa = lab / (top if top > 0 else 1.0) * n
        idx = np.where(xa == n, n - 1, np.floor(xa))  # a listed map sends 1.0 to its last entry, not past it
    else:
        idx = labels.astype(np.int64)
    idx = np.clip(idx, 0, n - 1).astype(np.int64)
    out = np.floor(table[idx] * 255.0).astype(np.uint8)
    out[labels < 0] = 0
    return out


def create_pcd_with_labels(pcd_data, super_cluster_id: int, super_point_labels: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """``pcd_data``: the list ``all_super_cluster_info*.npy`` holds; entry ``super_cluster_id``'s ``'pcd'`` maps sub-cluster
    index -> points [m,3].  Returns the sub-clusters concatenated in dict order and, per point, its sub-cluster's label."""
    sub = pcd_data[super_cluster_id]["pcd"]
    points, labels = [], []
    for cluster_idx in sub:
        p = np.asarray(sub[cluster_idx], dtype=np.float64).reshape(-1, 3)
        points.append(p)
        labels.append(np.full(len(p), super_point_labels[cluster_idx], dtype=np.float64))
    if not points:
        return np.zeros((0, 3)), np.zeros(0)
    return np.concatenate(points), np.concatenate(labels)


def labelled_result(pcd_data, labels_all) -> Tuple[np.ndarray, np.ndarray]:
    """All super-clusters that ``count_from_projection_dir`` labelled (its third return value: per super-cluster, the
    sub-cluster labels already shifted to be unique over the whole tree) -> (points [M,3], labels [M])."""
    parts = [create_pcd_with_labels(pcd_data, i, labels) for i, labels in enumerate(labels_all)]
    if not parts:
        return np.zeros((0, 3)), np.zeros(0)
    return np.concatenate([p for p, _ in parts]), np.concatenate([l for _, l in parts])


def super_cluster_labels(pcd_data) -> Tuple[np.ndarray, np.ndarray]:
    """``view_super_clusters`` (``evaluation/vis_semantic_seg.py:59-91``, ``generate_video.py:119-146``): every point of
    super-cluster i carries the label i + 1."""
    return labelled_result(pcd_data, [{k: i + 1 for k in entry["pcd"]} for i, entry in enumerate(pcd_data)])
