"""float64 restatement of the ray-side sampler arithmetic (``csrc/sampler.hip``, ``csrc/sampler_dev.hpp``, ``csrc/composite_dev.hpp``
and the sampler of ``csrc/proposal.hip``), for ``tests/test_gpu_sampler_big_shapes.py``.  Plain numpy, float64 throughout, nothing
imported from the package under test or from ``oracle/`` (``oracle/samplers.py`` stays the fp32 oracle: it builds ``linspace`` /
``zeros`` in the default dtype).

* spacing functions: uniform ``s(x) = x``; piecewise ``s(x) = x / 2`` for ``x < 1`` else ``1 - 1 / (2 x)``, inverse ``2 x`` for
  ``x < 0.5`` else ``1 / (2 - 2 x)``;  euclidean ``= s^-1(b s(far) + (1 - b) s(near))``;
* spaced bins: ``linspace(0, 1, S + 1)``; jittered ``lower + (upper - lower) t`` with lower / upper from the bin centres
  (``t`` [R,1] single jitter or [R,S+1]);
* ``get_weights``: ``nan_to_num((1 - exp(-delta sigma)) exp(-cumsum_exclusive(delta sigma)))``;
* median depth: the first index with ``cumsum(w) >= 0.5``, clamped to ``S - 1``, and how far the decision was from a tie;
* PDF resampling: ``w' = w^anneal + 0.01``; eps padding ``relu(1e-5 - sum w')`` spread over the samples; ``cdf = [0, min(1,
  cumsum(w' / sum))]``; ``u = linspace(0, 1 - 1/nb, nb) + 1 / (2 nb)`` (eval) or ``+ rand / nb``; ``searchsorted(right)``, clamped
  gather, ``t = clip(nan_to_num((u - c0) / (c1 - c0)), 0, 1)``, lerp of the previous bins.
"""

import numpy as np

UNIFORM, PIECEWISE = "uniform", "piecewise"


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def spacing_fn(spacing, x):
    x = _f64(x)
    if spacing == UNIFORM:
        return x
    with np.errstate(divide="ignore"):
        return np.where(x < 1.0, x / 2.0, 1.0 - 1.0 / (2.0 * x))


def spacing_inv(spacing, x):
    x = _f64(x)
    if spacing == UNIFORM:
        return x
    with np.errstate(divide="ignore"):
        return np.where(x < 0.5, 2.0 * x, 1.0 / (2.0 - 2.0 * x))


def spacing_to_euclidean(spacing, bins, nears, fars):
    """bins [R,N] in the spacing domain, nears / fars [R,1] -> euclidean [R,N]."""
    sn, sf = spacing_fn(spacing, nears), spacing_fn(spacing, fars)
    b = _f64(bins)
    return spacing_inv(spacing, b * sf + (1.0 - b) * sn)


def spaced_bins(num_samples, t_rand=None):
    """[1,S+1] (no jitter) or [R,S+1] spacing bins."""
    bins = np.linspace(0.0, 1.0, num_samples + 1, dtype=np.float64)[None, :]
    if t_rand is None:
        return bins
    centers = (bins[:, 1:] + bins[:, :-1]) / 2.0
    upper = np.concatenate([centers, bins[:, -1:]], -1)
    lower = np.concatenate([bins[:, :1], centers], -1)
    return lower + (upper - lower) * _f64(t_rand)


def get_weights(deltas, densities):
    """[R,S] x [R,S] -> weights [R,S]."""
    dd = _f64(deltas) * _f64(densities)
    with np.errstate(over="ignore", invalid="ignore"):
        alphas = 1.0 - np.exp(-dd)
        excl = np.concatenate([np.zeros_like(dd[:, :1]), np.cumsum(dd[:, :-1], -1)], -1)
        return np.nan_to_num(alphas * np.exp(-excl))


def median_index(weights):
    """-> (index [R], margin [R]): the first sample whose running weight reaches 0.5 (S - 1 when none does) and
    ``min(|cum[index] - 0.5|, |cum[index - 1] - 0.5|)`` -- how large an error of the running sum it takes to move the index.
    A ray that never reaches 0.5 has the margin ``0.5 - cum[S - 1]``."""
    cum = np.cumsum(_f64(weights), -1)
    S = cum.shape[-1]
    reached = cum >= 0.5
    idx = np.where(reached.any(-1), reached.argmax(-1), S - 1)
    rows = np.arange(cum.shape[0])
    at = np.abs(cum[rows, idx] - 0.5)
    before = np.where(idx > 0, np.abs(cum[rows, np.maximum(idx - 1, 0)] - 0.5), np.inf)
    never = ~reached.any(-1)
    margin = np.where(never, 0.5 - cum[:, -1], np.minimum(at, before))
    return idx, margin


def median_depth(weights, starts, ends):
    """-> (depth [R], index [R], margin [R])."""
    idx, margin = median_index(weights)
    mid = (_f64(starts) + _f64(ends)) / 2.0
    return mid[np.arange(mid.shape[0]), idx], idx, margin


def pdf_cdf(weights, anneal=1.0, histogram_padding=0.01, eps=1e-5):
    """weights [R,S_in] -> cdf [R,S_in+1]."""
    w = _f64(weights)
    if anneal != 1.0:
        w = np.power(w, anneal)
    w = w + histogram_padding
    total = w.sum(-1, keepdims=True)
    padding = np.maximum(eps - total, 0.0)
    w = w + padding / w.shape[-1]
    total = total + padding
    cdf = np.minimum(1.0, np.cumsum(w / total, -1))
    return np.concatenate([np.zeros_like(cdf[:, :1]), cdf], -1)


def pdf_u(num_samples, num_rays, u_rand=None):
    """[R,S_out+1]: bin centres (eval) or ``u + rand / nb`` (``u_rand`` [R,1] or [R,S_out+1])."""
    nb = num_samples + 1
    u = np.linspace(0.0, 1.0 - 1.0 / nb, nb, dtype=np.float64)[None, :]
    u = u + (1.0 / (2 * nb) if u_rand is None else _f64(u_rand) / nb)
    return np.broadcast_to(u, (num_rays, nb)).copy()


def pdf_resample(prev_bins, weights, num_samples, anneal=1.0, u_rand=None, histogram_padding=0.01, eps=1e-5):
    """prev_bins [R,S_in+1] (spacing domain), weights [R,S_in] -> spacing bins [R,S_out+1]."""
    prev = _f64(prev_bins)
    cdf = pdf_cdf(weights, anneal, histogram_padding, eps)
    R, n = cdf.shape
    prev = np.broadcast_to(prev, (R, n))
    u = pdf_u(num_samples, R, u_rand)
    inds = np.stack([np.searchsorted(cdf[r], u[r], side="right") for r in range(R)])
    below, above = np.clip(inds - 1, 0, n - 1), np.clip(inds, 0, n - 1)
    c0, c1 = np.take_along_axis(cdf, below, -1), np.take_along_axis(cdf, above, -1)
    b0, b1 = np.take_along_axis(prev, below, -1), np.take_along_axis(prev, above, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip(np.nan_to_num((u - c0) / (c1 - c0), nan=0.0), 0.0, 1.0)
    return b0 + t * (b1 - b0)


def composite(starts, ends, densities, rgb=None, background="last_sample"):
    """Weights, accumulation, median depth and (eval-mode, clamped) rgb of materialised samples.  rgb [R,S,3];
    ``background``: "last_sample" or three floats."""
    w = get_weights(_f64(ends) - _f64(starts), densities)
    depth, idx, margin = median_depth(w, starts, ends)
    out = {"weights": w, "accumulation": w.sum(-1, keepdims=True), "depth": depth[:, None], "index": idx, "margin": margin}
    if rgb is not None:
        c = np.nan_to_num(_f64(rgb))
        bg = c[:, -1, :] if isinstance(background, str) else np.broadcast_to(_f64(background), (c.shape[0], 3))
        out["rgb"] = np.clip((w[..., None] * c).sum(1) + bg * (1.0 - out["accumulation"]), 0.0, 1.0)
    return out
