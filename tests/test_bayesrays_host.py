"""CPU-side checks of the BayesRays consumer (``cropnerf_amd/fruit_nerf/bayesrays.py``, ``scripts/uncertainty.py``): the
Hessian loader, the CLI's argument surface and its missing-file error, the wrappers' refusal of CPU tensors, and the
reference-executed fixture ``tests/golden/bayesrays_functions.npz`` (what it must contain; that it regenerates equal where the
reference tree is present)."""

import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "bayesrays_functions.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(FIXTURE)


def _generator():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_golden_bayesrays as M
    finally:
        sys.path.pop(0)
    return M


@pytest.mark.parametrize("lod", [3, 4, 8])
def test_load_hessian_infers_lod(tmp_path, lod):
    from cropnerf_amd.fruit_nerf.bayesrays import load_hessian

    n = (2 ** lod + 1) ** 3
    assert n in (9 ** 3, 17 ** 3, 257 ** 3)
    path = tmp_path / "unc.npy"
    np.save(path, np.zeros(n, dtype=np.float32))
    h, got = load_hessian(path)
    assert got == lod and h.shape == (n,) and h.dtype == np.float32
    assert load_hessian(path, lod=lod)[1] == lod
    with pytest.raises(ValueError):
        load_hessian(path, lod=lod + 1)


def test_load_hessian_refuses_other_lengths(tmp_path):
    from cropnerf_amd.fruit_nerf.bayesrays import UncertaintyState, load_hessian

    path = tmp_path / "unc.npy"
    np.save(path, np.zeros(10 ** 3, dtype=np.float32))
    with pytest.raises(ValueError, match="1000"):
        load_hessian(path)
    with pytest.raises(ValueError):
        UncertaintyState(np.zeros(1000, dtype=np.float32))
    with pytest.raises(FileNotFoundError, match="unc.npy"):
        load_hessian(tmp_path / "absent" / "unc.npy")
    st = UncertaintyState(np.zeros(729, dtype=np.float64))  # the reference saves what its tensor holds
    assert st.lod == 3 and st.N == 4096 * 1000 and not st.filter_out and st.filter_thresh == 1.0


def test_cli_argument_surface():
    from cropnerf_amd.fruit_nerf.scripts import uncertainty as U

    ap = U.build_parser()
    a = ap.parse_args(["render", "--load-config", "run/config.json", "--unc-path", "unc.npy", "--output-dir", "out"])
    assert (a.cmd, str(a.load_config), str(a.unc_path), str(a.output_dir)) == ("render", "run/config.json", "unc.npy", "out")
    assert a.filter_out is False and a.filter_thresh == 0.5 and not a.white_bg and not a.black_bg
    assert a.N == 1000 * 4096 and a.num_rays > 0
    b = ap.parse_args(["render", "--load-config", "c", "--unc-path", "u", "--output-dir", "o", "--filter-out",
                       "--filter-thresh", "0.25", "--white-bg", "--num-rays", "4096", "--N", "8192"])
    assert b.filter_out and b.filter_thresh == 0.25 and b.white_bg and b.num_rays == 4096 and b.N == 8192
    for bad in (["render", "--load-config", "c", "--output-dir", "o"],                      # no --unc-path
                ["render", "--load-config", "c", "--unc-path", "u", "--output-dir", "o", "--white-bg", "--black-bg"],
                ["view", "--load-config", "c"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_cli_fails_clearly_without_the_hessian_file(tmp_path):
    """The file is looked for before the run directory is loaded: no GPU is needed to be told that it is missing."""
    from cropnerf_amd.fruit_nerf.scripts import uncertainty as U

    with pytest.raises(FileNotFoundError, match="no Hessian file"):
        U.entrypoint(["render", "--load-config", str(tmp_path / "config.json"), "--unc-path", str(tmp_path / "unc.npy"),
                      "--output-dir", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()


def test_wrappers_refuse_cpu_tensors():
    from cropnerf_amd import ops

    scene = ops.scene_struct(torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]), True)
    un = torch.ones(729)
    with pytest.raises((RuntimeError, TypeError)):
        ops.uncertainty_table(torch.zeros(729), 4096000.0)
    with pytest.raises((RuntimeError, TypeError)):
        ops.uncertainty_lookup(torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4, 8), torch.ones(4, 8), scene, un, 3)
    with pytest.raises((RuntimeError, TypeError)):
        ops.uncertainty_composite(torch.zeros(4, 8), torch.zeros(4, 8))
    assert [ops.uncertainty_lod(n ** 3) for n in (3, 9, 17, 257, 1025)] == [1, 3, 4, 8, 10]
    for n in (1000, 2 ** 3, 0, 2049 ** 3):
        with pytest.raises(ValueError):
            ops.uncertainty_lod(n)


def test_entry_points_validate_on_the_host():
    """Null pointers and a lod whose indices would not fit are refused before any HIP call."""
    import ctypes as C

    from cropnerf_amd import _lib

    lib = _lib.load()
    assert lib.cn_uncertainty_table(None, 3, 1.0, None, None) == _lib.CN_ERR_INVALID
    assert b"cn_uncertainty_table" in lib.cn_last_error()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    sc = _lib.Scene()
    for lod in (0, 11, -1):
        assert lib.cn_uncertainty_table(p, lod, 1.0, p, None) == _lib.CN_ERR_UNSUPPORTED
        assert lib.cn_uncertainty_lookup(p, p, p, p, 1, 1, C.byref(sc), p, lod, p, None, 0.0, None) == _lib.CN_ERR_UNSUPPORTED
    assert lib.cn_uncertainty_lookup(p, p, p, p, 1, 0, C.byref(sc), p, 3, p, None, 0.0, None) == _lib.CN_ERR_INVALID
    assert lib.cn_uncertainty_composite(None, p, 1, 1, p, None) == _lib.CN_ERR_INVALID
    assert lib.cn_uncertainty_composite(p, p, 0, 4, p, None) == 0  # no rays: nothing is launched


def test_fixture_holds_the_stated_cases(gold):
    """lod 3 and 4, 67 x 48 and 5 x 70, both normalisations, two thresholds; samples inside and outside the box, on cell faces and
    on normalised 0 and 1; Hessian with exact zeros and values >= 1000 N; no un_point within 1e-4 of a threshold * 6."""
    assert gold["lods"].tolist() == [3, 4] and gold["shapes"].tolist() == [[67, 48], [5, 70]]
    assert int(gold["N"]) == 1000 * 4096 and len(gold["thresholds"]) == 2
    lo, hi = torch.from_numpy(gold["aabb"])
    for si, (R, S) in enumerate(gold["shapes"].tolist()):
        assert R % 64 and S % 64
        o, d, bins = (torch.from_numpy(gold[f"s{si}/{k}"]) for k in ("origins", "directions", "bins"))
        assert tuple(bins.shape) == (R, S + 1)
        pos = o[:, None] + d[:, None] * ((bins[:, :-1] + bins[:, 1:]) / 2)[..., None]
        nrm = (pos - lo) / (hi - lo)
        inside = ((nrm > 0) & (nrm < 1)).all(-1)
        assert 0.05 < inside.float().mean() < 0.95                      # inside the box and outside it
        assert (nrm == 0).any() and (nrm == 1).any()                     # exactly on normalised 0 and 1
        assert ((nrm * 16 == (nrm * 16).floor()).all(-1) & inside).sum() >= 4   # vertices of the lod-4 grid, faces of both
        assert (pos.abs().amax(-1) > 1).float().mean() > 0.2           # beyond radius 1 under contraction
        assert (gold[f"s{si}/weights"].sum(-1) == 0).any()
        cu = gold[f"s{si}/comp_uncertainty"]
        assert cu.min() == 0.0 and cu.max() == 1.0                       # both clip ends
    for lod in (3, 4):
        h = gold[f"lod{lod}/hessian"]
        assert h.shape == ((2 ** lod + 1) ** 3,) and (h == 0).sum() > 10 and (h >= 1000.0 * float(gold["N"])).sum() > 10
        assert (h >= 0).all()
        for c in (0, 1):
            for si in range(2):
                k = f"lod{lod}/c{c}/s{si}"
                u = gold[f"{k}/un_points"]
                for ti, t in enumerate(gold["thresholds"]):
                    assert np.abs(u - t * 6).min() >= 1e-4, (k, t)
                    m = gold[f"{k}/mask{ti}"]
                    assert m.dtype == np.bool_ and np.array_equal(m, u <= t * 6) and 0 < m.mean() < 1
    assert os.path.getsize(FIXTURE) < 200 * 1024


def test_fixture_regenerates_equal(gold):
    """Executes the reference's functions again (``tests/golden/make_golden_bayesrays.py``) and compares every array."""
    M = _generator()
    if not M.available():
        pytest.skip("the reference tree is not on this machine")
    fresh = M.build()
    assert sorted(fresh) == sorted(gold.files)
    for k in gold.files:
        assert fresh[k].dtype == gold[k].dtype and np.array_equal(fresh[k], gold[k]), k
