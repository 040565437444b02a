"""The ray-side sampler at the sample counts of ``fruit_nerf_big`` (512, 256 -> 128) and ``fruit_nerf_huge`` (512, 512 -> 64), against
the float64 restatement in ``tests/_sampler_ref.py``.  512 is ``PROP_MAX_SAMPLES`` of ``csrc/proposal.hip``: a ray is eight 64-lane
chunks, ``wave_cdf_from_weights`` runs with 8 entries per lane, and the bins ping-pong with ``smax`` taken from a proposal level.
Counts and proposal networks are read from the shipped method configs; only the hash tables (``log2_T`` 12), the image (16 x 16)
and the batch (67 rays: no multiple of the 4 rays of a workgroup) are shrunk.

How a bar is set (``_held``).  Every quantity has a bar the suite already uses for it (named where it is used).  The fp32 CPU oracle
(``oracle/``) is run on the same stage inputs as the kernel and its error against float64 is measured in units of that bar: ``k``.
The kernel is held to ``max(1, 4 k)`` times the bar -- both sides are fp32 and differ in summation order; 4 leaves room for
``v_rcp`` / ``expf`` differences.  Every entry is compared.  The measured ``k`` are printed and recorded in the docstrings.

LDS of the kernels that take it dynamically, at their accepted maxima (four waves per workgroup, 64 KiB granted without opt-in):
``cn_sample_pdf`` 16 (3 s_in + 2) B = 65 504 B at s_in 1364 (the host bound, tested below); the fused sampler
16 (4 smax + 4) + 16 enc_rows 80 B = 32 832 + 20 480 = 53 312 B at smax 512 with a 7-level net (a ``static_assert`` in
``csrc/proposal.hip``; the formula is not exposed through the C interface, so no test reads it); the training unit at its
``TRAIN_MAX_S`` of 512: ``cn_train_render_backward`` and ``cn_distortion_metric`` 32 S = 16 384 B, ``cn_interlevel_backward`` and
``cn_interlevel_backward_levels`` 16 (5 S + 3) = 41 008 B.  All fit.

Measured on the MI355X (k = the fp32 oracle's worst error in units of the suite's bar, then the kernel's worst entry in the same
units; the largest over all cases of a test).  Where k is above 1 / 4 the rule widens the bar ("bar x ..." below); the kernel's
worst entry is below 1 everywhere, that is inside the suite's own bar:
  training sampler, stage by stage: level-0 bins k 0.049, kernel 0.049; starts / ends k 0.10, kernel 0.10; density k 0.033,
    kernel 0.037; resampled spacing bins k 0.16, kernel 0.20; final euclidean bins k 0.097, kernel 0.097
  cn_sample_spaced at 512: spacing bins k 0.049, kernel 0.049; starts / ends k 0.41 (bar x1.6), kernel 0.41
  cn_sample_pdf at 512 -> 256 / 512 / 64 and 256 -> 128: spacing bins k 0.39 (bar x1.6), kernel 0.74; euclidean bins k 0.12, kernel 0.12
  cn_composite at 512 / 128: weights k 0.30 (bar x1.2), kernel 0.41; accumulation k 0.18, kernel 0.18; rgb k 0.05, kernel 0.05
  fused eval sampler against the composed chain: spacing bins at 0.045 of rtol 1e-5 / atol 1e-6, euclidean bins at 0.10 (box rays,
    same bar) and 0.44 (model rays, error model)
"""

import ctypes as C
import dataclasses
import types

import numpy as np
import pytest
import torch

import _sampler_ref as REF
from oracle import field as OF
from oracle import model as OM
from oracle import rays as ORY
from oracle import samplers as OSM
from oracle import tcnn as TC

R = 67        # not a multiple of the 4 rays per workgroup
LOG2_T = 12   # shrunk hash tables
HW = 16       # 16 x 16 pixels, as the 7-level test
FOCAL = 20.0
METHODS = ("fruit_nerf_big", "fruit_nerf_huge")
CN_ERR_INVALID, CN_ERR_UNSUPPORTED = -1, -2

# the suite's bars, as tolerance(|reference|)
BAR_SPACED_SPACING = lambda x: 1e-7 + 1e-6 * np.abs(x)            # test_sample_spaced: spacing_starts / spacing_ends
BAR_SPACED_EUCLID = lambda x: 1e-6 + 2e-6 * np.abs(x)             # test_sample_spaced: starts / ends
BAR_PDF_SPACING = lambda x: 1e-6 + 1e-5 * np.abs(x)               # ..._stage_by_stage_on_the_oracles_inputs: spacing bins
BAR_EUCLID = lambda x: 1e-6 + 2e-5 * np.abs(x) + 1e-6 * x * x     # the same test's error model of euclidean bins
BAR_DENSITY = lambda x: 2e-5 + 2e-4 * np.abs(x)                   # test_proposal_density (RTOL, ATOL)
BAR_WEIGHTS = lambda x: 1e-7 + 2e-4 * np.abs(x)                   # test_composite: weights
BAR_RENDER = lambda x: 2e-5 + 2e-4 * np.abs(x)                    # test_composite: rgb, accumulation


def tie_margin(S):
    """A running fp32 sum of S weights in [0, 1] whose total is at most 1 is off by at most S 2^-24 in the worst (sequential) order;
    the weights themselves carry the error of the running optical depth (again at most S 2^-24 relative at the median, where it is
    ln 2) -- together S 2^-23.  Twice that is the margin below which a ray's median index is not compared."""
    return 2.0 * S * 2.0 ** -23


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _held(name, got, ref, oracle, bar):
    """``got`` (kernel) against ``ref`` (float64) under ``max(1, 4 k)`` x ``bar``, k = the fp32 oracle's error in units of the bar."""
    got, ref, oracle = (np.asarray(a, np.float64) for a in (got, ref, oracle))
    assert got.shape == ref.shape == oracle.shape, f"{name}: shapes {got.shape} {ref.shape} {oracle.shape}"
    tol = bar(ref)
    k = float(np.max(np.abs(oracle - ref) / tol))
    factor = max(1.0, 4.0 * k)
    ratio = np.abs(got - ref) / tol
    worst = float(np.max(ratio))
    print(f"[bar] {name}: fp32 oracle at {k:.3g} of the suite's bar -> x{factor:.3g}; kernel at {worst:.3g}")
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    assert worst <= factor, (f"{name}: {int((ratio > factor).sum())} / {ratio.size} entries outside {factor:.3g} x the bar, worst "
                             f"{worst:.3g} at {np.unravel_index(ratio.argmax(), ratio.shape)} (ref {ref.flat[ratio.argmax()]:.6g})")
    return k, worst


# ------------------------------------------------------------------------------------------------------------------
# the shipped configs, shrunk
# ------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Setup:
    method: str
    layout: str
    s_prop: tuple
    s_final: int
    model_config: object
    net_args: list
    ofspec: OF.FieldSpec
    ospecs: list
    params: dict   # CPU fp32, oracle names
    aabb: torch.Tensor
    c2w: torch.Tensor
    intr: torch.Tensor


_SETUPS = {}


def _model_config(method):
    from cropnerf_amd.fruit_nerf.fruit_nerf_config import native_method

    return native_method(method).config.pipeline.model


def _setup(method, layout="torch", grid_scale=0.3):
    if (method, layout, grid_scale) in _SETUPS:
        return _SETUPS[(method, layout, grid_scale)]
    from cropnerf_amd import synthetic

    cfg = _model_config(method)
    n = cfg.num_proposal_iterations
    args = [dict(cfg.proposal_net_args_list[min(i, len(cfg.proposal_net_args_list) - 1)]) for i in range(n)]
    for a in args:
        a["log2_hashmap_size"] = LOG2_T
    ospecs = [OF.ProposalSpec(OF.GridSpec(a["num_levels"], a.get("base_res", 16), a["max_res"], LOG2_T), a["hidden_dim"],
                              implementation=layout) for a in args]
    ofspec = OF.FieldSpec(grid=OF.GridSpec(cfg.num_levels, 16, cfg.max_res, LOG2_T), geo_feat_dim=cfg.geo_feat_dim,
                          num_layers_semantic=cfg.num_layers_semantic, hidden_dim_semantics=cfg.hidden_dim_semantics,
                          num_images=3, implementation=layout)
    seed = 20 + METHODS.index(method)
    if layout == "tcnn":
        params = TC.random_params(ofspec, ospecs, seed=seed, grid_scale=grid_scale)
        for k in list(params):  # the values tcnn computes with: the oracle rounds them itself, the importer keeps float32 masters
            if k.endswith("tcnn_encoding.params"):
                params[k] = params[k].to(torch.float16).to(torch.float32)
    else:
        params = OF.random_params(ofspec, ospecs, seed=seed, grid_scale=grid_scale)
    c2w, intr = synthetic.orbit_cameras(3, height=HW, width=HW, focal=FOCAL)
    s = Setup(method, layout, tuple(int(x) for x in cfg.num_proposal_samples_per_ray), int(cfg.num_nerf_samples_per_ray), cfg, args,
              ofspec, ospecs, params, torch.tensor(synthetic.SCENE_AABB, dtype=torch.float32), c2w, intr)
    _SETUPS[(method, layout, grid_scale)] = s
    return s


def _rays(setup, kind, cam=1):
    """67 rays of one camera.  "model": near 0 / far 1000 with scene contraction, as FruitModel runs the sampler; "box": near / far
    from the scene box."""
    rb = ORY.image_rays(setup.c2w, setup.intr, cam, HW, HW)
    if kind == "box":
        rb = ORY.with_aabb_near_far(rb, setup.aabb.reshape(-1))
        rb.nears = rb.nears + 0.01
    else:
        rb.nears, rb.fars = torch.zeros(len(rb), 1), torch.full((len(rb), 1), 1000.0)
    rb = rb.slice(90, 90 + R)
    assert len(rb) == R and bool((rb.fars > rb.nears + 0.5).all())
    return rb.origins, rb.directions, rb.nears.contiguous(), rb.fars.contiguous()


def _tcnn_density_f64(p01, vec, gspec):
    """The tcnn-layout proposal network (``oracle/tcnn.py``: ``network_with_grid``, one hidden layer of 16, no biases) in float64."""
    n_mlp = TC.mlp_param_count(gspec.out_dim, 1, 16, 1)
    w0, w1 = (m.numpy() for m in TC.mlp_matrices(torch.from_numpy(vec[:n_mlp]), gspec.out_dim, 1, 16, 1))
    table = vec[n_mlp:].reshape(-1, gspec.features_per_level)
    offs = gspec.offset_table()
    enc = []
    for l, (scale, res) in enumerate(zip(gspec.scales(), gspec.resolutions())):
        pos = p01 * float(scale) + 0.5
        fl = np.floor(pos)
        frac = pos - fl
        pg = fl.astype(np.int64).astype(np.uint32)
        acc = np.zeros((p01.shape[0], gspec.features_per_level))
        for idx in range(8):
            w = np.ones(p01.shape[0])
            corner = pg.copy()
            for d in range(3):
                if idx & (1 << d):
                    w = w * frac[:, d]
                    corner[:, d] += np.uint32(1)
                else:
                    w = w * (1.0 - frac[:, d])
            acc += table[TC.grid_index(corner, res, offs[l + 1] - offs[l]) + offs[l]] * w[:, None]
        enc.append(acc)
    enc = np.concatenate(enc, -1)
    hid = np.maximum(enc @ w0[:, : enc.shape[1]].T, 0.0)
    return np.exp(hid @ w1[0])


def _density_f64(setup, lvl, pos, contraction=True):
    """float64 proposal density at positions [R,S,3] (float64 tensor) -> numpy [R,S]."""
    spec = setup.ospecs[lvl]
    if setup.layout == "tcnn":
        p, sel = OF.normalized_positions(pos, setup.aabb.double(), contraction)
        vec = setup.params[f"proposal_networks.{lvl}.mlp_base.tcnn_encoding.params"].double().numpy()
        den = _tcnn_density_f64(p.reshape(-1, 3).numpy(), vec, TC.grid_spec_of(spec.grid)).reshape(pos.shape[:-1])
        return den * sel.numpy()
    p64 = {k: v.double() for k, v in setup.params.items() if k.startswith(f"proposal_networks.{lvl}.")}
    return OF.proposal_density(pos, p64, lvl, spec, setup.aabb.double(), contraction)[..., 0].numpy()


def _density_f32(setup, lvl, o, d, starts, ends, contraction=True):
    """The fp32 oracle's density on the intervals [R,S] (fp32 tensors), positions formed as the oracle forms them."""
    pos = o[:, None, :] + d[:, None, :] * ((starts + ends) / 2)[..., None]
    return OF.proposal_density(pos, setup.params, lvl, setup.ospecs[lvl], setup.aabb, contraction)[..., 0]


def _positions_f64(o, d, starts, ends):
    mid = (starts.double() + ends.double()) / 2.0
    return o.double()[:, None, :] + d.double()[:, None, :] * mid[..., None]


def _oracle_euclid(bins, n, f):
    fn, inv = OSM.SPACING["piecewise"]
    return inv(bins * fn(f) + (1 - bins) * fn(n))


def _oracle_resample(prev_bins, starts, ends, den, n, f, s_next, anneal, u_rand):
    """fp32 oracle: weights of the intervals, then the PDF resampling step -> spacing bins [R, s_next + 1]."""
    w = OSM.get_weights((ends - starts)[..., None], den[..., None])
    prev = OSM.RaySamples(None, None, None, None, prev_bins[:, :-1, None], prev_bins[:, 1:, None], None, n, f, "piecewise")
    nxt = OSM.pdf_sampler(prev, torch.pow(w, anneal), s_next, u_rand=u_rand)
    return torch.cat([nxt.spacing_starts[..., 0], nxt.spacing_ends[:, -1:, 0]], -1)


def _f64_chain(setup, o, d, n, f, anneal=1.0, jitter=None, contraction=True):
    """The whole sampler in float64 (eval when ``jitter`` is None) -> per proposal level (bins, starts, ends, density, weights),
    and the final spacing bins."""
    n64, f64 = n.double().numpy(), f.double().numpy()
    bins = np.broadcast_to(REF.spaced_bins(setup.s_prop[0], None if jitter is None else _np(jitter[0])), (len(o), setup.s_prop[0] + 1))
    levels = []
    for lvl, S in enumerate(setup.s_prop):
        eu = REF.spacing_to_euclidean(REF.PIECEWISE, bins, n64, f64)
        st, en = torch.from_numpy(eu[:, :-1].copy()), torch.from_numpy(eu[:, 1:].copy())
        den = _density_f64(setup, lvl, _positions_f64(o, d, st, en), contraction)
        w = REF.get_weights(eu[:, 1:] - eu[:, :-1], den)
        levels.append(dict(bins=bins, starts=eu[:, :-1], ends=eu[:, 1:], density=den, weights=w))
        s_next = setup.s_prop[lvl + 1] if lvl + 1 < len(setup.s_prop) else setup.s_final
        bins = REF.pdf_resample(bins, w, s_next, anneal, None if jitter is None else _np(jitter[lvl + 1]))
    return levels, bins


def _depth_coverage(weights, S):
    """What the median-depth comparison of one level covers: (index, keep mask, chunks crossed among the kept rays, number of kept
    rays that cross in the fifth chunk or later with more than 0.05 of weight carried in from the chunks before: the rays a lost
    or mis-scaled carry of the running weight would move)."""
    idx, margin = REF.median_index(weights)
    keep = margin >= tie_margin(S)
    chunk = idx // 64
    cum = np.cumsum(weights, -1)
    carried = np.where(chunk > 0, cum[np.arange(len(idx)), np.maximum(64 * chunk - 1, 0)], 0.0)
    return idx, keep, sorted(set(chunk[keep].tolist())), int((keep & (chunk >= 4) & (carried > 0.05)).sum())


# ------------------------------------------------------------------------------------------------------------------
# CPU tier: the restatement itself, the coverage conditions on the reference alone, the host-side limits
# ------------------------------------------------------------------------------------------------------------------

def test_shipped_configs_are_the_shapes_this_file_is_about():
    big, huge = _setup("fruit_nerf_big"), _setup("fruit_nerf_huge")
    assert (big.s_prop, big.s_final) == ((512, 256), 128) and [a["num_levels"] for a in big.net_args] == [5, 5]
    assert (huge.s_prop, huge.s_final) == ((512, 512), 64) and [(a["num_levels"], a["max_res"]) for a in huge.net_args] == [(5, 512), (7, 2048)]
    # smax comes from a proposal level, not from the final count, and is the kernel's maximum
    assert max(big.s_prop) == max(huge.s_prop) == 512 > max(big.s_final, huge.s_final)


@pytest.mark.parametrize("spacing", ["uniform", "piecewise"])
@pytest.mark.parametrize("jitter", [None, "single", "full"])
def test_reference_spaced_bins_agree_with_the_fp32_oracle(spacing, jitter):
    S = 512
    g = torch.Generator().manual_seed(5)
    n = torch.rand(R, 1, generator=g) + 0.05
    f = n + 1 + 4 * torch.rand(R, 1, generator=g)
    t = None if jitter is None else torch.rand(R, 1 if jitter == "single" else S + 1, generator=g)
    rb = ORY.RayBundle(torch.zeros(R, 3), torch.zeros(R, 3), torch.zeros(R, 1), None, n, f)
    rs = OSM.spaced_sampler(rb, S, spacing, t_rand=t)
    bins = np.broadcast_to(REF.spaced_bins(S, None if t is None else _np(t)), (R, S + 1))
    eu = REF.spacing_to_euclidean(spacing, bins, _np(n), _np(f))
    assert np.abs(_np(rs.spacing_starts[..., 0].expand(R, S)) - bins[:, :-1]).max() < 2e-7   # three ulps of a value below 1
    assert np.abs(_np(rs.spacing_ends[..., 0].expand(R, S)) - bins[:, 1:]).max() < 2e-7
    assert (np.abs(_np(rs.starts[..., 0]) - eu[:, :-1]) <= BAR_SPACED_EUCLID(eu[:, :-1])).all()
    assert (np.abs(_np(rs.ends[..., 0]) - eu[:, 1:]) <= BAR_SPACED_EUCLID(eu[:, 1:])).all()
    assert (np.diff(bins, axis=-1) > 0).all() and bins.min() >= 0.0 and bins.max() <= 1.0


def _pdf_case(s_in, s_out, train, seed=3):
    """Inputs of one resampling step: jittered previous bins, random weights and the designed rows (all-zero, one-hot)."""
    g = torch.Generator().manual_seed(seed + s_in + s_out)
    n = torch.rand(R, 1, generator=g) * 0.5 + 0.05
    f = n + 1 + 3 * torch.rand(R, 1, generator=g)
    prev = torch.from_numpy(np.broadcast_to(REF.spaced_bins(s_in, _np(torch.rand(R, 1, generator=g))), (R, s_in + 1)).copy()).float()
    w = torch.rand(R, s_in, generator=g) ** 4
    w[::9] *= 1e-3  # faint rays: the padding dominates
    hot = [k for k in (0, 63, 64, 447, 448, 511) if k < s_in]
    w[5] = 0.0
    for row, k in zip(range(6, 6 + len(hot)), hot):
        w[row] = 0.0
        w[row, k] = 1.0
    u = torch.rand(R, 1, generator=g) if train else None
    return prev, w, n, f, u, hot


PDF_SHAPES = [(512, 256), (512, 512), (256, 128), (512, 64)]


@pytest.mark.parametrize("anneal", [1.0, 0.35])
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("s_in,s_out", PDF_SHAPES)
def test_reference_resampling_agrees_with_the_fp32_oracle(s_in, s_out, train, anneal):
    prev, w, n, f, u, _ = _pdf_case(s_in, s_out, train)
    ref = REF.pdf_resample(_np(prev), _np(w), s_out, anneal, None if u is None else _np(u))
    rs = OSM.RaySamples(None, None, None, None, prev[:, :-1, None], prev[:, 1:, None], None, n, f, "piecewise")
    nxt = OSM.pdf_sampler(rs, torch.pow(w[..., None], anneal), s_out, u_rand=u)
    got = _np(torch.cat([nxt.spacing_starts[..., 0], nxt.spacing_ends[:, -1:, 0]], -1))
    # fp32 rounding of a 512-term running sum (3e-5 of a cdf step of 1.6e-3 at the least) times a bin: a few 1e-6 at the most
    err = np.abs(got - ref)
    assert err.max() < 2e-5, err.max()
    assert (np.diff(ref, axis=-1) >= 0).all() and ref.min() >= 0 and ref.max() <= 1


def test_reference_resampling_known_answers():
    S, nb = 512, 257
    prev = REF.spaced_bins(S)
    u = REF.pdf_u(nb - 1, 1)
    # uniform weights: the cdf is linear in the bins, so the new bins are u itself
    assert np.abs(REF.pdf_resample(prev, np.full((1, S), 0.37), nb - 1) - u).max() < 1e-14
    # all-zero weights: 0.01 padding per sample already exceeds eps, the pdf is uniform
    assert np.abs(REF.pdf_resample(prev, np.zeros((1, S)), nb - 1) - u).max() < 1e-14
    # ... and without the histogram padding the eps branch spreads 1e-5 over the samples: uniform again, not 0 / 0
    cdf = REF.pdf_cdf(np.zeros((1, S)), histogram_padding=0.0)
    assert np.allclose(np.diff(cdf), 1.0 / S, rtol=1e-12, atol=0) and cdf[0, -1] <= 1.0
    assert np.abs(REF.pdf_resample(prev, np.zeros((1, S)), nb - 1, histogram_padding=0.0) - u).max() < 1e-12
    # one-hot: the interval holds (1 + 0.01) / (1 + 0.01 S) of the mass, so that share of the new bins falls inside it
    for k in (0, 63, 64, 447, 448, 511):
        w = np.zeros((1, S))
        w[0, k] = 1.0
        b = REF.pdf_resample(prev, w, nb - 1)[0]
        inside = ((b >= prev[0, k]) & (b <= prev[0, k + 1])).sum()
        share = 1.01 / (1.0 + 0.01 * S)
        assert abs(inside - share * nb) <= 1.0, (k, inside, share * nb)
        # and the cdf where it can be checked by hand (a 512-term float64 running sum: 512 x 1.1e-16)
        c = REF.pdf_cdf(w)[0]
        assert abs(c[k] - 0.01 * k / (1 + 0.01 * S)) < 1e-13 and abs(c[k + 1] - (0.01 * k + 1.01) / (1 + 0.01 * S)) < 1e-13
    # annealing: w^0 = 1 for every positive weight -> uniform
    assert np.abs(REF.pdf_resample(prev, np.random.default_rng(0).uniform(0.1, 1, (1, S)), nb - 1, anneal=0.0) - u).max() < 1e-13
    # jitter: u + rand / nb
    assert np.abs(REF.pdf_u(nb - 1, 1, np.array([[0.25]])) - (np.arange(nb) / nb + 0.25 / nb)).max() < 1e-15


def test_reference_homogeneous_medium_known_answer():
    """The closed form of ``test_composite_homogeneous_known_answer``, and the weights against the oracle."""
    import math

    S, near, far, sigma = 192, 0.5, 2.5, 3.0
    eu = REF.spacing_to_euclidean(REF.UNIFORM, REF.spaced_bins(S), np.array([[near]]), np.array([[far]]))
    out = REF.composite(eu[:, :-1], eu[:, 1:], np.full((1, S), sigma))
    assert abs(out["accumulation"][0, 0] - (1 - math.exp(-sigma * (far - near)))) < 1e-13
    delta = (far - near) / S
    k = math.ceil(math.log(2) / (sigma * delta)) - 1
    assert out["index"][0] == k and abs(out["depth"][0, 0] - (near + (k + 0.5) * delta)) < 1e-13
    cum = np.cumsum(out["weights"][0])
    assert abs(out["margin"][0] - min(abs(cum[k] - 0.5), abs(cum[k - 1] - 0.5))) < 1e-15
    g = torch.Generator().manual_seed(0)
    den = torch.rand(5, S, 1, generator=g) * 20
    st, en = torch.from_numpy(eu[:, :-1]).float().expand(5, S), torch.from_numpy(eu[:, 1:]).float().expand(5, S)
    w = OSM.get_weights((en - st)[..., None], den)[..., 0]
    assert np.abs(_np(w) - REF.get_weights(_np(en) - _np(st), _np(den[..., 0]))).max() < 1e-6
    # a ray that never reaches 0.5 takes the last sample; one that reaches it at sample 0 has no "before"
    idx, margin = REF.median_index(np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.0]]))
    assert idx.tolist() == [2, 0] and np.allclose(margin, [0.2, 0.1])


@pytest.mark.parametrize("layout", ["torch", "tcnn"])
@pytest.mark.parametrize("method", METHODS)
def test_reference_density_agrees_with_the_fp32_oracle(method, layout):
    setup = _setup(method, layout)
    o, d, n, f = _rays(setup, "model")
    eu = torch.from_numpy(REF.spacing_to_euclidean(REF.PIECEWISE, np.broadcast_to(REF.spaced_bins(96), (R, 97)), _np(n), _np(f))).float()
    st, en = eu[:, :-1].contiguous(), eu[:, 1:].contiguous()
    for lvl in range(2):
        ref = _density_f64(setup, lvl, _positions_f64(o, d, st, en))
        got = _np(_density_f32(setup, lvl, o, d, st, en))
        assert ref.min() > 0 and (np.abs(got - ref) <= 4 * BAR_DENSITY(ref)).all(), np.abs((got - ref) / BAR_DENSITY(ref)).max()


DEPTH_DENSITY = (12.0, 50.0)


def _depth_setup(method):
    """The median-depth comparison wants crossings that are far from a tie, spread over the chunks of a ray, and fed by weight from
    the chunks before.  A random network is a haze of density about 1, whose crossings are none of these.  So: the shipped networks
    with ln 12 (level 0) and ln 50 (level 1) added to the output bias -- density about 12 and 50 wherever there is any -- no scene
    contraction (nothing outside the scene box), and rays that start outside the box (``_depth_rays``): each ray runs through
    empty space first and crosses 0.5 some tens of samples into the box.  The two figures are chosen so that the float64 chain
    alone meets the conditions asserted in ``test_depth_comparison_covers_four_chunks_on_the_reference_alone``."""
    key = (method, "depth")
    if key not in _SETUPS:
        base = _setup(method)
        params = dict(base.params)
        for lvl in range(len(base.ospecs)):
            name = f"proposal_networks.{lvl}.mlp.layers.1.bias"
            params[name] = params[name] + float(np.log(DEPTH_DENSITY[lvl]))
        _SETUPS[key] = dataclasses.replace(base, method=method + "/depth", params=params)
    return _SETUPS[key]


def _depth_rays(setup):
    """The camera's rays with their origins pulled back out of the scene box, ray by ray, so that the box is entered at a spacing
    coordinate between 8 % and 92 % of the ray (near 0, far 10): entries in every chunk of the 512 samples."""
    o, d, _, _ = _rays(setup, "model")
    _, behind = ORY.intersect_aabb(o, -d, setup.aabb.reshape(-1))  # the camera sits inside the box: distance to the wall behind it
    fars = torch.full((R, 1), 10.0)
    s_entry = torch.linspace(0.08, 0.92, R, dtype=torch.float64) * float(REF.spacing_fn(REF.PIECEWISE, 10.0))
    t_entry = torch.from_numpy(REF.spacing_inv(REF.PIECEWISE, s_entry.numpy())).float()
    o = o - d * (behind.reshape(R, 1) + t_entry[:, None])
    return o.contiguous(), d, torch.zeros(R, 1), fars


@pytest.mark.parametrize("method", METHODS)
def test_depth_comparison_covers_four_chunks_on_the_reference_alone(method):
    """The eval test below compares ``prop_depth`` exactly outside the tie margin.  On the float64 chain alone: at most 2 % of the
    rays are left out at either level, the crossings of a 512-sample level fall into at least four different 64-sample chunks, and
    at least three of them, in the fifth chunk or later, are reached on weight carried in from earlier chunks."""
    setup = _depth_setup(method)
    o, d, n, f = _depth_rays(setup)
    levels, _ = _f64_chain(setup, o, d, n, f, contraction=False)
    for lvl, S in enumerate(setup.s_prop):
        idx, keep, chunks, carried = _depth_coverage(levels[lvl]["weights"], S)
        print(f"{method} level {lvl}: {int((~keep).sum())} of {R} rays inside the tie margin {tie_margin(S):.3g}; chunks {chunks}; "
              f"{carried} rays cross on carried weight")
        assert (~keep).sum() <= 0.02 * R
        assert levels[lvl]["weights"].sum(-1).min() > 0.99  # every ray does cross
        if S == 512:
            assert len(chunks) >= 4, chunks
            assert carried >= 3, carried


@pytest.fixture(scope="module")
def lib():
    import cropnerf_amd
    from cropnerf_amd import _lib

    if not _lib.LIB_PATH.exists():
        cropnerf_amd.build_library()
    return _lib.load()


def test_sample_pdf_refuses_rows_that_cannot_launch(lib):
    """16 (3 s_in + 2) bytes of dynamic LDS per workgroup: s_in <= 1364 fits 64 KiB; anything longer is CN_ERR_UNSUPPORTED before
    any HIP call (the pointers are never dereferenced)."""
    p = C.c_void_p(64)
    for s_in in (1365, 3412, 4096, 4097, 1 << 20):
        rc = lib.cn_sample_pdf(p, p, p, p, 3, s_in, 8, 1.0, 1, None, 0, p, p, None)
        assert rc == CN_ERR_UNSUPPORTED, s_in
        msg = lib.cn_last_error()
        assert b"cn_sample_pdf" in msg and str(s_in).encode() in msg and b"1364" in msg
        assert 16 * (3 * s_in + 2) > 65536
    assert 16 * (3 * 1364 + 2) <= 65536
    for s_in, s_out in ((0, 8), (-1, 8), (8, 0)):
        assert lib.cn_sample_pdf(p, p, p, p, 3, s_in, s_out, 1.0, 1, None, 0, p, p, None) == CN_ERR_INVALID
    assert lib.cn_sample_pdf(p, p, p, p, 0, 1364, 8, 1.0, 1, None, 0, p, p, None) == 0  # accepted; no rays, no launch


def test_513_samples_are_refused_by_every_fused_entry_point(lib):
    """PROP_MAX_SAMPLES: 513 at level 0 or as s_final is CN_ERR_UNSUPPORTED from all four entry points, before any HIP call and
    before the networks are looked at; the message names the level.  (Level 1: the GPU tier, it needs a valid first network.)"""
    from cropnerf_amd import _lib as L
    from cropnerf_amd import config as PC
    from cropnerf_amd import ops

    p = C.c_void_p(64)
    nets = (C.POINTER(L.DensityParams) * 2)(C.pointer(L.DensityParams()), C.pointer(L.DensityParams()))
    outs = (L.ProposalLevelOut * 2)()
    scene = L.Scene()

    def call(name, s_prop, s_final):
        sp = (C.c_int32 * 2)(*s_prop)
        head = (nets, 2, C.byref(scene), p, p, p, p, 3, sp, s_final)
        if name == "cn_proposal_sample":
            return lib.cn_proposal_sample(*head, 1.0, p, p, p, None, 0, None)
        if name == "cn_proposal_sample_mp":
            return lib.cn_proposal_sample_mp(*head, 1.0, p, p, p, L.MATRIX_F16, None)
        if name == "cn_proposal_sample_train":
            return lib.cn_proposal_sample_train(*head, 1.0, p, outs, p, p, p, p, None)
        return lib.cn_proposal_sample_train_dev(*head, p, p, outs, p, p, p, p, None)

    for name in ("cn_proposal_sample", "cn_proposal_sample_mp", "cn_proposal_sample_train", "cn_proposal_sample_train_dev"):
        assert call(name, (513, 256), 128) == CN_ERR_UNSUPPORTED, name
        msg = lib.cn_last_error()
        assert name.encode() in msg and b"513 samples at level 0" in msg, msg
        assert call(name, (512, 512), 513) == CN_ERR_UNSUPPORTED, name
        msg = lib.cn_last_error()
        assert name.encode() in msg and b"s_final 513" in msg, msg
    nets5 = [types.SimpleNamespace(spec=PC.ProposalSpec(PC.GridSpec(5, 16, 512, LOG2_T, 2, "torch"), 16)) for _ in range(2)]
    for s_prop, s_final, ok in (((512, 512), 512, True), ((513, 256), 128, False), ((512, 513), 64, False), ((512, 512), 513, False)):
        assert ops.proposal_sample_fused_supported(nets5, s_prop, s_final) is ok


# ------------------------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from cropnerf_amd import ops as _ops

    return _ops


def _dev(t):
    return None if t is None else t.to("cuda").contiguous()


_HANDLES = {}


def _handles(ops, setup):
    """(device parameters, product proposal specs, density handles), fp32 tables in either layout."""
    key = (setup.method, setup.layout)
    if key not in _HANDLES:
        from cropnerf_amd import config as PC

        ps = [PC.ProposalSpec(PC.GridSpec(a["num_levels"], a.get("base_res", 16), a["max_res"], LOG2_T, 2, setup.layout), a["hidden_dim"])
              for a in setup.net_args]
        if setup.layout == "tcnn":
            from cropnerf_amd.fruit_nerf import tcnn_params as TP

            g = setup.ofspec.grid
            fs = PC.FieldSpec(grid=PC.GridSpec(g.num_levels, g.min_res, g.max_res, LOG2_T, 2, "tcnn"), geo_feat_dim=setup.ofspec.geo_feat_dim,
                              num_layers_semantic=setup.ofspec.num_layers_semantic,
                              hidden_dim_semantics=setup.ofspec.hidden_dim_semantics, num_images=3)
            dp = TP.from_tcnn_state_dict(setup.params, fs, ps, "cuda", torch.float32)
        else:
            dp = {k: v.to("cuda").contiguous() for k, v in setup.params.items()}
        _HANDLES[key] = (dp, ps, [ops.DensityHandle(dp, i, s) for i, s in enumerate(ps)])
    return _HANDLES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("anneal", [1.0, 0.35])
@pytest.mark.parametrize("layout", ["torch", "tcnn"])
@pytest.mark.parametrize("method", METHODS)
def test_training_sampler_stage_by_stage_on_its_own_outputs(ops, method, layout, anneal):
    """``cn_proposal_sample_train`` at the big / huge counts: every stage against float64 fed with the kernel's OWN previous stage
    (level i + 1 is an inverse cdf of level i, so errors would compound otherwise), both ray set-ups, every entry:
    level-0 bins vs the jittered spaced bins; starts / ends vs spacing -> euclidean of the kernel's bins; density vs the float64
    network on the kernel's intervals; the next level's (and the final) spacing bins vs float64 resampling of the kernel's bins with
    float64 weights of the kernel's densities; final starts / ends bit-equal to the slices of the euclidean bins.
    Bars: the rule of the module docstring, whose last paragraph has the measured k (fp32 oracle, in units of the suite's bar)
    and the kernel's worst entry per quantity; both are printed again on every run."""
    setup = _setup(method, layout)
    dp, ps, dh = _handles(ops, setup)
    assert ops.proposal_sample_fused_supported(dh, setup.s_prop, setup.s_final)
    sc = ops.scene_struct(setup.aabb, True)
    for kind in ("model", "box"):
        o, d, n, f = _rays(setup, kind)
        g = torch.Generator().manual_seed(31)
        jitter = [torch.rand(R, 1, generator=g) for _ in range(3)]
        fused = ops.proposal_sample_train(dh, sc, _dev(o), _dev(d), _dev(n), _dev(f), setup.s_prop, setup.s_final, anneal,
                                          _dev(torch.cat([j.reshape(1, R) for j in jitter], 0)))
        n64, f64 = _np(n), _np(f)
        tag = f"{method} {layout} anneal {anneal} {kind}"
        lv0 = fused["levels"][0]
        rb = ORY.RayBundle(o, d, torch.zeros(R, 1), None, n, f)
        rs0 = OSM.spaced_sampler(rb, setup.s_prop[0], "piecewise", t_rand=jitter[0])
        oracle0 = torch.cat([rs0.spacing_starts[..., 0], rs0.spacing_ends[:, -1:, 0]], -1)
        _held(f"{tag}: level 0 bins", _np(lv0["bins"]), REF.spaced_bins(setup.s_prop[0], _np(jitter[0])), _np(oracle0), BAR_SPACED_SPACING)
        for lvl, S in enumerate(setup.s_prop):
            lv = {k: v.cpu() for k, v in fused["levels"][lvl].items()}
            assert lv["bins"].shape == (R, S + 1) and lv["density"].shape == (R, S)
            assert bool((lv["bins"][:, 1:] >= lv["bins"][:, :-1]).all())
            eu = REF.spacing_to_euclidean(REF.PIECEWISE, _np(lv["bins"]), n64, f64)
            eu32 = _np(_oracle_euclid(lv["bins"], n, f))
            _held(f"{tag}: level {lvl} starts", _np(lv["starts"]), eu[:, :-1], eu32[:, :-1], BAR_EUCLID)
            _held(f"{tag}: level {lvl} ends", _np(lv["ends"]), eu[:, 1:], eu32[:, 1:], BAR_EUCLID)
            den64 = _density_f64(setup, lvl, _positions_f64(o, d, lv["starts"], lv["ends"]))
            den32 = _density_f32(setup, lvl, o, d, lv["starts"], lv["ends"])
            _held(f"{tag}: level {lvl} density", _np(lv["density"]), den64, _np(den32), BAR_DENSITY)
            last = lvl + 1 == len(setup.s_prop)
            s_next = setup.s_final if last else setup.s_prop[lvl + 1]
            nxt = fused["spacing_bins"].cpu() if last else fused["levels"][lvl + 1]["bins"].cpu()
            w64 = REF.get_weights(_np(lv["ends"]) - _np(lv["starts"]), _np(lv["density"]))
            ref = REF.pdf_resample(_np(lv["bins"]), w64, s_next, anneal, _np(jitter[lvl + 1]))
            orc = _oracle_resample(lv["bins"], lv["starts"], lv["ends"], lv["density"], n, f, s_next, anneal, jitter[lvl + 1])
            _held(f"{tag}: spacing bins after level {lvl}", _np(nxt), ref, _np(orc), BAR_PDF_SPACING)
        sp = fused["spacing_bins"].cpu()
        eu = REF.spacing_to_euclidean(REF.PIECEWISE, _np(sp), n64, f64)
        _held(f"{tag}: final euclidean bins", _np(fused["euclidean_bins"]), eu, _np(_oracle_euclid(sp, n, f)), BAR_EUCLID)
        assert torch.equal(fused["starts"], fused["euclidean_bins"][:, :-1]) and torch.equal(fused["ends"], fused["euclidean_bins"][:, 1:])


def _composed_chain(ops, dh, sc, o, d, n, f, s_prop, s_final):
    """cn_sample_spaced + cn_proposal_density + cn_composite + cn_sample_pdf on the device, eval mode."""
    from cropnerf_amd import _lib as L

    sm = ops.sample_spaced(n, f, s_prop[0], L.SPACING_PIECEWISE)
    bins = torch.cat([sm["spacing_starts"], sm["spacing_ends"][:, -1:]], -1).contiguous()
    starts, ends = sm["starts"], sm["ends"]
    levels = []
    for lvl in range(len(s_prop)):
        den = ops.proposal_density(dh[lvl], sc, o, d, starts, ends)
        comp = ops.composite(starts, ends, den, want_weights=True)
        levels.append(dict(starts=starts.cpu(), ends=ends.cpu(), density=den.cpu(), depth=comp["depth"].cpu()))
        bins, eu = ops.sample_pdf(bins, comp["weights"], n, f, s_prop[lvl + 1] if lvl + 1 < len(s_prop) else s_final)
        starts, ends = eu[:, :-1].contiguous(), eu[:, 1:].contiguous()
    return levels, bins.cpu(), eu.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["torch", "tcnn"])
@pytest.mark.parametrize("method", METHODS)
def test_eval_sampler_matches_the_composed_chain(ops, method, layout):
    """``cn_proposal_sample`` at the big / huge counts == the four materialising calls composed on the device, in the pattern and
    under the bars of ``test_unfused_proposal_chain_matches_fused`` (euclidean bins, rtol 1e-5, atol 1e-6) on the box rays.  On
    the model's rays (near 0, far 1000) that bar cannot be met by anything but identical bits: a euclidean bin is
    1 / (2 - 2 x) of a spacing bin x, so one fp32 ulp of x (6e-8) is 1.2e-7 eu^2, 0.12 at eu = 1000 against the bar's 0.01.  There
    the spacing bins are held to rtol 1e-5 / atol 1e-6 and the euclidean bins to the suite's error model for them,
    1e-6 + 2e-5 |x| + 1e-6 x^2."""
    setup = _setup(method, layout)
    dp, ps, dh = _handles(ops, setup)
    sc = ops.scene_struct(setup.aabb, True)
    for kind in ("box", "model"):
        o, d, n, f = (_dev(x) for x in _rays(setup, kind))
        fused = ops.proposal_sample(dh, sc, o, d, n, f, setup.s_prop, setup.s_final)
        _, sp, eu = _composed_chain(ops, dh, sc, o, d, n, f, setup.s_prop, setup.s_final)
        got_sp, got_eu = _np(fused["spacing_bins"]), _np(fused["euclidean_bins"])
        sp, eu = _np(sp), _np(eu)
        r_sp = np.abs(got_sp - sp) / BAR_PDF_SPACING(sp)
        r_eu = np.abs(got_eu - eu) / (1e-6 + 1e-5 * np.abs(eu) if kind == "box" else BAR_EUCLID(eu))
        print(f"[bar] {method} {layout} {kind}: fused vs composed, spacing bins at {r_sp.max():.3g} of the bar, euclidean at {r_eu.max():.3g}")
        assert r_sp.max() <= 1.0, f"{kind}: spacing bins, worst {r_sp.max():.3g} of the bar"
        assert r_eu.max() <= 1.0, f"{kind}: euclidean bins, worst {r_eu.max():.3g} of the bar"


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_eval_prop_depth_is_the_float64_median_sample(ops, method):
    """``prop_depth`` of both levels of ``cn_proposal_sample``: the sample it names must be the one float64 finds on the composed
    chain's intervals and densities -- exactly, on every ray whose decision is further from a tie than ``tie_margin(S)``
    (S 2^-23 x 2: 1.2e-4 at 512, 6.1e-5 at 256).  At most 2 % of the rays are left out, and the compared crossings of a 512-sample
    level lie in at least four different 64-sample chunks, three or more of them reached on weight carried in from earlier chunks
    (asserted on the float64 chain alone in the CPU tier, and here).  Measured on the MI355X: no ray left out at level 0, at most
    one at level 1; all eight chunks crossed at level 0; 3 (big) and 6 (huge) level-0 rays cross on carried weight -- the rays that
    come out wrong when ``composite_chunk`` drops ``carry_w`` from the fifth chunk on."""
    setup = _depth_setup(method)
    dp, ps, dh = _handles(ops, setup)
    sc = ops.scene_struct(setup.aabb, False)
    o, d, n, f = (_dev(x) for x in _depth_rays(setup))
    fused = ops.proposal_sample(dh, sc, o, d, n, f, setup.s_prop, setup.s_final)
    levels, _, _ = _composed_chain(ops, dh, sc, o, d, n, f, setup.s_prop, setup.s_final)
    rows = np.arange(R)
    for lvl, S in enumerate(setup.s_prop):
        lv = levels[lvl]
        w64 = REF.get_weights(_np(lv["ends"]) - _np(lv["starts"]), _np(lv["density"]))
        idx, keep, chunks, carried = _depth_coverage(w64, S)
        assert (~keep).sum() <= 0.02 * R, f"level {lvl}: {(~keep).sum()} rays inside the tie margin"
        if S == 512:
            assert len(chunks) >= 4 and carried >= 3, (chunks, carried)
        mids = ((lv["starts"] + lv["ends"]) / 2).numpy()  # fp32, as the kernels form them
        got = fused["prop_depth"][lvl].cpu().numpy()
        got_idx = np.abs(mids.astype(np.float64) - got[:, None].astype(np.float64)).argmin(-1)
        print(f"{method} level {lvl}: {int((~keep).sum())} rays left out, chunks {chunks}, "
              f"{int((got_idx != idx)[keep].sum())} kept rays off, {int((got_idx != idx)[~keep].sum())} left-out rays off")
        assert (got_idx == idx)[keep].all(), f"level {lvl}: rays {rows[keep & (got_idx != idx)]} name sample {got_idx[keep & (got_idx != idx)]}, float64 {idx[keep & (got_idx != idx)]}"
        ref = mids[rows, idx]
        assert (np.abs(got - ref)[keep] <= 1e-5 + 1e-5 * np.abs(ref[keep])).all()  # and its value (the bar of _depth_match)
        # the composed chain's own cn_composite depth names the same sample, bit for bit
        assert (lv["depth"][:, 0].numpy()[keep] == ref[keep]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("spacing", ["uniform", "piecewise"])
@pytest.mark.parametrize("jitter", [None, "single", "full"])
def test_sample_spaced_at_512(ops, spacing, jitter):
    """``cn_sample_spaced`` at S = 512 against float64, bars of ``test_sample_spaced`` under the rule of the module docstring."""
    from cropnerf_amd import _lib as L

    S = 512
    g = torch.Generator().manual_seed(5)
    n = torch.rand(R, 1, generator=g) + 0.05
    f = n + 1 + 4 * torch.rand(R, 1, generator=g)
    t = None if jitter is None else torch.rand(R, 1 if jitter == "single" else S + 1, generator=g)
    rs = OSM.spaced_sampler(ORY.RayBundle(torch.zeros(R, 3), torch.zeros(R, 3), torch.zeros(R, 1), None, n, f), S, spacing, t_rand=t)
    out = ops.sample_spaced(_dev(n), _dev(f), S, L.SPACING_UNIFORM if spacing == "uniform" else L.SPACING_PIECEWISE, _dev(t))
    bins = np.broadcast_to(REF.spaced_bins(S, None if t is None else _np(t)), (R, S + 1))
    eu = REF.spacing_to_euclidean(spacing, bins, _np(n), _np(f))
    tag = f"spaced {spacing} {jitter}"
    _held(f"{tag}: spacing_starts", _np(out["spacing_starts"]), bins[:, :-1], _np(rs.spacing_starts[..., 0].expand(R, S)), BAR_SPACED_SPACING)
    _held(f"{tag}: spacing_ends", _np(out["spacing_ends"]), bins[:, 1:], _np(rs.spacing_ends[..., 0].expand(R, S)), BAR_SPACED_SPACING)
    _held(f"{tag}: starts", _np(out["starts"]), eu[:, :-1], _np(rs.starts[..., 0]), BAR_SPACED_EUCLID)
    _held(f"{tag}: ends", _np(out["ends"]), eu[:, 1:], _np(rs.ends[..., 0]), BAR_SPACED_EUCLID)


@pytest.mark.gpu
@pytest.mark.parametrize("anneal", [1.0, 0.35])
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("s_in,s_out", PDF_SHAPES)
def test_sample_pdf_at_big_and_huge_lengths(ops, s_in, s_out, train, anneal):
    """``cn_sample_pdf`` at 512 -> 256, 512 -> 512, 256 -> 128 and 512 -> 64 against float64: random rows, faint rows, an all-zero
    row and one-hot rows at 0, 63, 64, 447, 448 and 511 (where they exist).  Spacing bins: the bar of the stage-by-stage test
    (rtol 1e-5, atol 1e-6); euclidean bins: its error model; both under the rule of the module docstring."""
    prev, w, n, f, u, hot = _pdf_case(s_in, s_out, train)
    assert len(hot) == (6 if s_in == 512 else 3) and bool((w[5] == 0).all()) and all(float(w[6 + i, k]) == 1.0 for i, k in enumerate(hot))
    sp, eu = ops.sample_pdf(_dev(prev), _dev(w), _dev(n), _dev(f), s_out, anneal=anneal, u_rand=_dev(u))
    ref = REF.pdf_resample(_np(prev), _np(w), s_out, anneal, None if u is None else _np(u))
    rs = OSM.RaySamples(None, None, None, None, prev[:, :-1, None], prev[:, 1:, None], None, n, f, "piecewise")
    nxt = OSM.pdf_sampler(rs, torch.pow(w[..., None], anneal), s_out, u_rand=u)
    orc = torch.cat([nxt.spacing_starts[..., 0], nxt.spacing_ends[:, -1:, 0]], -1)
    tag = f"pdf {s_in}->{s_out} train={train} anneal={anneal}"
    _held(f"{tag}: spacing bins", _np(sp), ref, _np(orc), BAR_PDF_SPACING)
    ref_eu = REF.spacing_to_euclidean(REF.PIECEWISE, _np(sp), _np(n), _np(f))  # of the kernel's own spacing bins
    _held(f"{tag}: euclidean bins", _np(eu), ref_eu, _np(_oracle_euclid(sp.cpu(), n, f)), BAR_EUCLID)


@pytest.mark.gpu
def test_sample_pdf_at_its_longest_accepted_row(ops):
    """s_in = 1364, the longest row the host accepts (65 504 B of LDS): 3 rays against float64."""
    s_in, s_out = 1364, 200
    g = torch.Generator().manual_seed(8)
    n, f = torch.full((3, 1), 0.1), torch.tensor([[2.0], [30.0], [1000.0]])
    prev = torch.from_numpy(np.broadcast_to(REF.spaced_bins(s_in), (3, s_in + 1)).copy()).float()
    w = torch.rand(3, s_in, generator=g) ** 4
    w[1] = 0.0
    w[1, 1363] = 1.0
    sp, eu = ops.sample_pdf(_dev(prev), _dev(w), _dev(n), _dev(f), s_out)
    ref = REF.pdf_resample(_np(prev), _np(w), s_out)
    rs = OSM.RaySamples(None, None, None, None, prev[:, :-1, None], prev[:, 1:, None], None, n, f, "piecewise")
    nxt = OSM.pdf_sampler(rs, w[..., None], s_out)
    _held("pdf 1364->200: spacing bins", _np(sp), ref, _np(torch.cat([nxt.spacing_starts[..., 0], nxt.spacing_ends[:, -1:, 0]], -1)), BAR_PDF_SPACING)
    _held("pdf 1364->200: euclidean bins", _np(eu), REF.spacing_to_euclidean(REF.PIECEWISE, _np(sp), _np(n), _np(f)),
          _np(_oracle_euclid(sp.cpu(), n, f)), BAR_EUCLID)
    from cropnerf_amd._lib import CropNerfHipError

    with pytest.raises(CropNerfHipError, match="1365") as e:
        ops.sample_pdf(_dev(torch.zeros(3, 1366)), _dev(torch.zeros(3, 1365)), _dev(n), _dev(f), s_out)
    assert e.value.code == CN_ERR_UNSUPPORTED


OPAQUE_AT = (0, 63, 64, 127, 128, 255, 256, 447, 448, 511)


def _composite_case(S):
    """Designed rays first, random rays after.  -> starts, ends, density, rgb (fp32 tensors) and the designed rows."""
    g = torch.Generator().manual_seed(S)
    n_rand = 300
    ks = [k for k in OPAQUE_AT if k < S]
    Rc = len(ks) + 3 + n_rand
    nears = torch.rand(Rc, 1, generator=g)
    fars = nears + 1 + torch.rand(Rc, 1, generator=g)
    bins = torch.from_numpy(REF.spacing_to_euclidean(REF.UNIFORM, np.broadcast_to(REF.spaced_bins(S), (Rc, S + 1)), _np(nears), _np(fars))).float()
    st, en = bins[:, :-1].contiguous(), bins[:, 1:].contiguous()
    # random rays: a faint haze with a dense sample here and there (3 % of them, optical depth up to 0.6 each), so that the
    # median is decided by a weight of 0.1 or so, somewhere along the ray
    dense = torch.rand(Rc, S, generator=g) < 0.03
    dd = torch.where(dense, 0.6 * torch.rand(Rc, S, generator=g), 1e-4 * torch.rand(Rc, S, generator=g))
    den = dd / (en - st)
    den[len(ks) + 3::7] *= 0.01  # random rays that never reach 0.5
    delta = en - st
    for row, k in enumerate(ks):  # one opaque sample (delta * density = 40), 1e-6 of optical depth everywhere else
        den[row] = 1e-6 / (delta[row] * S)
        den[row, k] = 40.0 / delta[row, k]
    never, only_last, thin = len(ks), len(ks) + 1, len(ks) + 2
    den[never] = 0.3 / (delta[never] * S)                      # total optical depth 0.3: accumulation 0.26
    den[only_last] = 0.5 / (delta[only_last] * S)              # 0.39 before the last sample ...
    den[only_last, S - 1] = 1.0 / delta[only_last, S - 1]      # ... which adds 0.61 * 0.63
    den[thin] = 1e-9                                           # nothing accumulates: the background is all there is
    rgb = torch.rand(Rc, S, 3, generator=g)
    return st, en, den, rgb, dict(opaque=ks, never=never, only_last=only_last, thin=thin, first_random=len(ks) + 3)


@pytest.mark.parametrize("S", [512, 128])
def test_composite_designed_rays_are_what_they_claim_on_the_reference(S):
    st, en, den, rgb, rows = _composite_case(S)
    ref = REF.composite(_np(st), _np(en), _np(den))
    for row, k in enumerate(rows["opaque"]):
        assert ref["index"][row] == k and ref["margin"][row] > 0.49 and _np(en - st)[row, k] * float(den[row, k]) >= 30
    assert ref["accumulation"][rows["never"], 0] < 0.3 and ref["index"][rows["never"]] == S - 1
    cum = np.cumsum(ref["weights"][rows["only_last"]])
    assert cum[S - 2] < 0.45 and cum[S - 1] > 0.55 and ref["index"][rows["only_last"]] == S - 1
    assert ref["accumulation"][rows["thin"], 0] < 1e-6
    rnd = slice(rows["first_random"], None)
    keep = ref["margin"][rnd] >= tie_margin(S)
    assert (~keep).mean() <= 0.01
    assert len(set((ref["index"][rnd] // 64).tolist())) >= min(4, S // 64)
    assert (ref["accumulation"][rnd, 0] < 0.5).sum() >= 20  # random rays that never reach 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("S", [512, 128])
def test_composite_at_512_and_128(ops, S):
    """``cn_composite`` against float64.  Designed rays: one opaque sample at k in {0, 63, 64, 127, 128, 255, 256, 447, 448, 511}
    (depth == that sample's midpoint, exactly), a ray that never reaches 0.5 and one that reaches it only at the last sample (depth ==
    the last midpoint, exactly), a ray that accumulates nothing (BG_LAST_SAMPLE: the colour of sample S - 1).  Random rays: weights,
    accumulation and rgb under the bars of ``test_composite`` and the rule of the module docstring; depth exactly on every ray
    outside ``tie_margin(S)``, at most 1 % left out."""
    from cropnerf_amd import _lib as L
    from oracle import render as ORD

    st, en, den, rgb, rows = _composite_case(S)
    ref = REF.composite(_np(st), _np(en), _np(den), _np(rgb))
    out = ops.composite(_dev(st), _dev(en), _dev(den), _dev(rgb), bg_mode=L.BG_LAST_SAMPLE, want_weights=True)
    w32 = OSM.get_weights((en - st)[..., None], den[..., None])
    _held(f"composite {S}: weights", _np(out["weights"]), ref["weights"], _np(w32[..., 0]), BAR_WEIGHTS)
    _held(f"composite {S}: accumulation", _np(out["accumulation"]), ref["accumulation"], _np(ORD.render_accumulation(w32)), BAR_RENDER)
    _held(f"composite {S}: rgb", _np(out["rgb"]), ref["rgb"], _np(ORD.render_rgb(rgb, w32, "last_sample")), BAR_RENDER)
    mids = ((st + en) / 2).numpy()  # fp32, as the kernel forms them
    got = out["depth"].cpu().numpy()[:, 0]
    want = mids[np.arange(len(mids)), ref["index"]]
    for row, k in enumerate(rows["opaque"]):
        assert got[row] == mids[row, k], f"opaque sample {k}: depth {got[row]} != midpoint {mids[row, k]}"
    for name in ("never", "only_last", "thin"):
        assert got[rows[name]] == mids[rows[name], S - 1], name
    keep = ref["margin"] >= tie_margin(S)
    assert (~keep)[rows["first_random"]:].mean() <= 0.01
    assert (got == want)[keep].all(), f"depth differs on rays {np.flatnonzero(keep & (got != want))}"
    assert np.abs(_np(out["rgb"])[rows["thin"]] - _np(rgb)[rows["thin"], S - 1]).max() <= 2e-5  # the background is sample S - 1
    bg = (0.2, 0.5, 1.0)
    out2 = ops.composite(_dev(st), _dev(en), _dev(den), _dev(rgb), bg_mode=L.BG_COLOR, bg_color=bg)
    ref2 = REF.composite(_np(st), _np(en), _np(den), _np(rgb), background=bg)
    _held(f"composite {S}: rgb on a colour", _np(out2["rgb"]), ref2["rgb"],
          _np(ORD.render_rgb(rgb, w32, torch.tensor(bg, dtype=torch.float32))), BAR_RENDER)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_513_samples_at_level_1_are_refused(ops, method):
    """The level-1 refusal needs a valid first network, so it runs here: every fused entry point, the message names the level."""
    from cropnerf_amd import _lib as L

    setup = _setup(method)
    dp, ps, dh = _handles(ops, setup)
    sc = ops.scene_struct(setup.aabb, True)
    o, d, n, f = (_dev(x) for x in _rays(setup, "box"))
    assert not ops.proposal_sample_fused_supported(dh, (512, 513), setup.s_final)
    jit = torch.rand(3, R, device="cuda")
    calls = {
        "cn_proposal_sample": lambda: ops.proposal_sample(dh, sc, o, d, n, f, (512, 513), setup.s_final),
        "cn_proposal_sample_mp": lambda: ops.proposal_sample(dh, sc, o, d, n, f, (512, 513), setup.s_final, matrix_precision=L.MATRIX_F16),
        "cn_proposal_sample_train": lambda: ops.proposal_sample_train(dh, sc, o, d, n, f, (512, 513), setup.s_final, 1.0, jit),
        "cn_proposal_sample_train_dev": lambda: ops.proposal_sample_train(dh, sc, o, d, n, f, (512, 513), setup.s_final,
                                                                          torch.ones(1, device="cuda"), jit),
    }
    for name, call in calls.items():
        with pytest.raises(L.CropNerfHipError, match="513 samples at level 1") as e:
            call()
        assert e.value.code == CN_ERR_UNSUPPORTED and name in e.value.message


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_model_routes_the_shipped_counts_into_the_fused_sampler(method, monkeypatch):
    """One ``FruitModel`` from the big and one from the huge config (tables shrunk), eval mode, against ``oracle_model`` at the same
    counts: a routing check, not a precision check (the stages are held to their bars above).  The model must hand exactly the
    config's counts to ``cn_proposal_sample`` (``proposal_sample_fused_supported`` is true for them); final bins, ``prop_depth_0/1``
    and the render then agree with the oracle under the end-to-end bars of ``test_big_method_shape_runs_through_the_generic_kernels``
    (rtol 2e-3, atol 2e-3) -- on every ray; the bins under the suite's error model of euclidean bins widened by the same end-to-end
    factor of 10 that separates 2e-3 from the stage bar 2e-4; ``prop_depth`` names the oracle's sample on every ray whose oracle
    weights are outside the tie margin."""
    from cropnerf_amd import ops
    from cropnerf_amd.fruit_nerf.fruit_nerf import FruitModel, Semantics
    from cropnerf_amd.rays import Cameras, SceneBox

    setup = _setup(method)
    cfg = dataclasses.replace(setup.model_config, log2_hashmap_size=LOG2_T, proposal_net_args_list=setup.net_args)
    assert tuple(cfg.num_proposal_samples_per_ray) == setup.s_prop and cfg.num_nerf_samples_per_ray == setup.s_final
    m = FruitModel(cfg, SceneBox(setup.aabb), 3, {"semantics": Semantics()}, device="cuda", test_mode="test", params=setup.params)
    assert ops.proposal_sample_fused_supported(m.proposal_networks, cfg.num_proposal_samples_per_ray, cfg.num_nerf_samples_per_ray)
    assert [p.spec.grid.num_levels for p in m.proposal_networks] == [a["num_levels"] for a in setup.net_args]
    seen = []
    real = ops.proposal_sample

    def spy(props, scene, o, d, n, f, s_prop, s_final, **kw):
        out = real(props, scene, o, d, n, f, s_prop, s_final, **kw)
        seen.append((tuple(s_prop), s_final, out["euclidean_bins"].cpu()))
        return out

    monkeypatch.setattr(ops, "proposal_sample", spy)
    cams = Cameras(setup.c2w, setup.intr[:, 0], setup.intr[:, 1], setup.intr[:, 2], setup.intr[:, 3], HW, HW).to("cuda")
    out = m(cams.generate_rays(camera_indices=1, keep_shape=False))
    assert len(seen) == 1 and seen[0][:2] == (setup.s_prop, setup.s_final)
    ocfg = OM.ModelConfig(field=setup.ofspec, proposals=setup.ospecs, num_proposal_samples_per_ray=setup.s_prop,
                          num_nerf_samples_per_ray=setup.s_final)
    om = OM.OracleModel(setup.params, ocfg, setup.aabb, test_mode="test")
    rb = ORY.image_rays(setup.c2w, setup.intr, 1, HW, HW)
    ref = om.forward(rb)
    assert list(out) == ["rgb", "accumulation", "depth", "prop_depth_0", "prop_depth_1", "semantics", "semantics_colormap"]
    for key in ("rgb", "accumulation", "semantics"):
        got, want = _np(out[key]), _np(ref[key])
        ratio = np.abs(got - want) / (2e-3 + 2e-3 * np.abs(want))
        print(f"[bar] {method} model {key}: worst {ratio.max():.3g} of rtol 2e-3 / atol 2e-3")
        assert ratio.max() <= 1.0, f"{key}: worst {ratio.max():.3g} of the bar"
    ref_bins = _np(torch.cat([ref["_starts"][..., 0], ref["_ends"][:, -1:, 0]], -1))
    ratio = np.abs(_np(seen[0][2]) - ref_bins) / (10.0 * BAR_EUCLID(ref_bins))
    print(f"[bar] {method} model final bins: worst {ratio.max():.3g} of 10 x the error model")
    assert ratio.max() <= 1.0, f"final bins: worst {ratio.max():.3g}"
    rbo = ORY.apply_pose_adjustment(ORY.near_far_collider(rb, training=False), setup.params["camera_optimizer.pose_adjustment"])
    _, weights_list, samples_list = OSM.proposal_sampler(rbo, om._density_fns(), setup.s_prop, setup.s_final)
    for lvl, S in enumerate(setup.s_prop):
        idx, keep, _, _ = _depth_coverage(_np(weights_list[lvl][..., 0]), S)
        smp = samples_list[lvl]
        mids = ((smp.starts + smp.ends) / 2)[..., 0].numpy()
        got = out[f"prop_depth_{lvl}"].cpu().numpy()[:, 0]
        got_idx = np.abs(mids.astype(np.float64) - got[:, None].astype(np.float64)).argmin(-1)
        print(f"{method} model prop_depth_{lvl}: {int((~keep).sum())} of {len(keep)} rays inside the tie margin, "
              f"{int((got_idx != idx)[keep].sum())} kept rays off")
        assert (ref[f"prop_depth_{lvl}"].numpy()[:, 0] == mids[np.arange(len(idx)), idx])[keep].all()  # the oracle agrees with float64
        assert (got_idx == idx)[keep].all()
