"""The definition of ``cn_instance_labels`` in numpy (include/cropnerf_hip.h): per frame, key = B << 16 | G << 8 | R, black ->
0, any other pixel -> 1 + the number of smaller distinct non-zero keys of the frame."""

import numpy as np


def labels_from_rgb(frames):
    """frames [F,H,W,3] uint8 RGB -> (labels [F,H,W] uint8, colors [F,256] int64, num_colors [F] int32).  Raises
    ``ValueError`` for a frame with more than 255 non-black colours."""
    frames = np.asarray(frames)
    assert frames.ndim == 4 and frames.shape[3] == 3 and frames.dtype == np.uint8, (frames.shape, frames.dtype)
    F, H, W, _ = frames.shape
    f = frames.astype(np.int64)
    keys = (f[..., 2] << 16) | (f[..., 1] << 8) | f[..., 0]
    labels = np.zeros((F, H, W), np.uint8)
    colors = np.zeros((F, 256), np.int64)
    num_colors = np.zeros(F, np.int32)
    for i in range(F):
        uniq = np.unique(keys[i][keys[i] != 0])
        if len(uniq) > 255:
            raise ValueError(f"frame {i}: {len(uniq)} non-black colours")
        labels[i] = np.where(keys[i] == 0, 0, np.searchsorted(uniq, keys[i]) + 1).astype(np.uint8)
        colors[i, 1:len(uniq) + 1] = uniq
        num_colors[i] = len(uniq)
    return labels, colors, num_colors


def labels_only(frames):
    """The ``convert=`` callable of ``convert_img_to_label`` / ``load_projection_tree``."""
    return labels_from_rgb(frames)[0]
