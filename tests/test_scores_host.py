"""CPU: scoring rasters with gaps -- what can be held without a GPU.

  * the restatement tests/scores_reference.py against tests/eval_reference.py: with an all-ones mask (and with no mask) it IS
    eval_reference.metrics, exactly, on the five golden crops; what the invalid pixels hold -- NaN, inf, 0, 1e30 -- changes nothing,
  * the cases of the GPU tolerance tests have enough terms: every one of the five counts of every blob image is >= 300, and the
    smallest are the ones the masks were chosen for; the edge cases have the counts they are planted for,
  * the train-time restatement with an all-ones mask is the oracle's psnr_skimage / ssim_skimage,
  * the pins of include/sifsr_scores.h for the `sifsrv_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, every entry point that can write through a pointer has a memory-contract case in tests/test_scores_gpu.py, scratch sizes
    and error codes through the host-only paths,
  * the public names exist with the defaults that leave every existing call as it was."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import eval_reference as E
from tests import scores_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_eval_v1.npz")


def same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float64).view(np.uint64), np.asarray(y, np.float64).view(np.uint64))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def test_all_valid_is_eval_reference_exactly():
    gold = np.load(GOLDEN)
    assert len(gold["kinds"]) == 5
    for i in range(5):
        a, b = gold[f"a{i}"], gold[f"b{i}"]
        H, W = a.shape
        want, wx = E.metrics(a, b)
        for mask in (np.ones((H, W), np.uint8), np.full((H, W), 200, np.uint8), None):
            got, gx = R.metrics(a, b, mask)
            assert same_bits(got, want), (i, got, want)
            assert gx["counts"] == (H * W, (H - 2) * (W - 2), (H - 6) * (W - 6), (H - 8) * (W - 8), H * W)
            assert np.float32(gx["q25"]).tobytes() == np.float32(wx["q25"]).tobytes() and gx["strata_counts"] == wx["counts"]
            assert np.float32(gx["R"]).tobytes() == np.float32(wx["R"]).tobytes()


@pytest.mark.parametrize("hw", R.BLOB_SHAPES)
def test_invalid_pixels_are_inert_in_the_restatement(hw):
    a, b, m = R.blob_case(hw)
    for i in range(len(a)):
        want, wx = R.metrics(a[i], b[i], m[i])
        assert np.isfinite(want).all()
        for junk in (np.nan, np.inf, 0.0, 1e30):
            pa, pb = a[i].copy(), b[i].copy()
            pa[m[i] == 0] = junk
            pb[m[i] == 0] = -junk
            got, gx = R.metrics(pa, pb, m[i])
            assert same_bits(got, want) and gx["counts"] == wx["counts"]
            if junk != 1e30:                              # NaN, inf and 0 are no-data on their own: no mask needed
                for qa, qb in ((pa, b[i]), (a[i], pb)):
                    got, gx = R.metrics(qa, qb, None)
                    assert same_bits(got, want) and gx["counts"] == wx["counts"]


def test_the_tolerance_cases_have_enough_terms():
    smallest = {}
    for hw in R.BLOB_SHAPES:
        a, b, m = R.blob_case(hw)
        counts = np.array([R.metrics(a[i], b[i], m[i])[1]["counts"] for i in range(len(a))])
        print(hw, counts.tolist())
        assert (counts >= 300).all()
        assert (0.29 <= 1 - m.mean(axis=(1, 2))).all() and (1 - m.mean(axis=(1, 2)) <= 0.31).all()
        smallest[hw] = int(counts.min())
    assert smallest == {(41, 57): 308, (96, 80): 2553}


@pytest.mark.parametrize("hw", [(16, 16), (24, 40)])
def test_the_edge_cases_are_what_they_are_planted_for(hw):
    a, b, m = R.edge_case(hw)
    rows, extras = zip(*(R.metrics(a[i], b[i], m[i]) for i in range(4)))
    assert abs(float(a[0].mean())) < 1e-3 and abs(float(a[0].std()) - 1) < 1e-3            # z-scored
    assert extras[0]["counts"] == (0, 0, 0, 0, 0) and np.isnan(rows[0]).all()
    assert extras[1]["counts"] == (81, 49, 9, 1, 1)
    assert extras[2]["counts"] == (81, 49, 9, 1, 25)                                          # the clipped S is larger than E_4
    assert np.isfinite(rows[1]).all() and np.isfinite(rows[2]).all() and np.isfinite(rows[3]).all()
    g, S = extras[1]["g"], extras[1]["S"]
    assert S.sum() == 1 and extras[1]["q25"] == extras[1]["q75"] == g[S][0]                   # the percentile of one value
    assert extras[1]["strata_counts"] == (0, 1, 1) and rows[1][3] == 0 and rows[1][4] == rows[1][5] > 0
    assert min(extras[3]["counts"]) >= 3


@pytest.mark.parametrize("kelvin", [False, True])
def test_train_time_restatement_all_valid_is_the_oracle(kelvin):
    for hw in R.TRAIN_SHAPES:
        p, t = R.train_inputs(hw, kelvin)
        for scale in (1, 4):
            ps, ss, n = R.psnr_ssim(p, t, np.ones((2, hw[0] // scale, hw[1] // scale), np.uint8), scale)
            assert n == (2, 2) and ps == O.psnr_skimage(p, t) and ss == O.ssim_skimage(p, t)


@pytest.mark.parametrize("hw", R.TRAIN_SHAPES)
def test_train_time_masks(hw):
    p, t = R.train_inputs(hw, False)
    for scale in (1, 4):
        v = R.train_mask(hw, scale, "blobs")
        assert 0.25 <= 1 - (v != 0).mean() <= 0.35 and len(np.unique(v)) == 3
        assert R.psnr_ssim(p, t, v, scale)[2] == (2, 2)
        v = R.train_mask(hw, scale, "image0")
        assert not v[0].any() and R.psnr_ssim(p, t, v, scale)[2] == (1, 1)
        v = R.train_mask(hw, scale, "single")
        assert R.upsampled(v, scale).sum() == 16
        ps, ss, n = R.psnr_ssim(p, t, v, scale)
        assert n == (1, 0) and np.isfinite(ps) and np.isnan(ss)                # a 4 x 4 block holds no 7 x 7 window
        junk = p.copy()
        junk[:, 0][~R.upsampled(v, scale)] = np.nan
        assert R.psnr_ssim(junk, t, v, scale)[0] == ps
        assert R.psnr_ssim(p, t, np.zeros_like(v), scale)[2] == (0, 0)


# ---- 2. the pins of include/sifsr_scores.h (the gate itself is tests/test_capi_gate.py) -----------------------------------------
def test_every_writing_score_entry_point_has_a_contract_case(L):
    from tests import test_scores_gpu as T
    names, writers = L.declared("scores"), L.writers("scores")
    assert names == ["sifsrv_eval_metrics", "sifsrv_eval_metrics_scratch_bytes", "sifsrv_psnr_ssim", "sifsrv_psnr_ssim_scratch_bytes"]
    assert writers == {"sifsrv_eval_metrics": ["scratch", "out8", "counts5"], "sifsrv_psnr_ssim": ["scratch", "out2", "counts2"]}
    assert all(n not in writers for n in ("sifsrv_eval_metrics_scratch_bytes", "sifsrv_psnr_ssim_scratch_bytes"))
    assert sorted(T.CONTRACT) == sorted(writers)
    assert all(len(cases) >= 3 for cases in T.CONTRACT.values())


def test_host_only_entry_points(L):
    """scratch sizes; shape, argument and workspace errors are found before anything is launched (none needs a GPU)"""
    size = lambda name, *a: L.call(name, *a)
    for b, h, w in ((1, 16, 16), (3, 41, 57), (8, 335, 374), (64, 256, 256)):
        need = size("sifsrv_eval_metrics_scratch_bytes", b, h, w)
        # the unmasked layout, one byte per pixel for the validity and the per-tile counts on top
        assert need >= size("sifsr_eval_metrics_scratch_bytes", b, h, w) + b * h * w
        assert need <= size("sifsr_eval_metrics_scratch_bytes", b, h, w) + b * h * w + 16 * b * (((h + 15) // 16) * ((w + 15) // 16) + 1) + 1024
        assert size("sifsrv_psnr_ssim_scratch_bytes", b, h, w) >= size("sifsr_psnr_ssim_scratch_bytes", b, h, w)
    for b, h, w in ((0, 16, 16), (1, 15, 16), (1, 16, 15), (65536, 16, 16), (1, 65536, 65536)):
        assert size("sifsrv_eval_metrics_scratch_bytes", b, h, w) == 0
    assert size("sifsrv_psnr_ssim_scratch_bytes", 1, 6, 8) == 0 and size("sifsrv_psnr_ssim_scratch_bytes", 300, 8, 8) > 0

    one = ctypes.c_void_p(4096)
    taps = (ctypes.c_float * 9)(*([1 / 9] * 9))
    ev = L.lib().sifsrv_eval_metrics
    args = lambda **kw: [kw.get("ref", one), kw.get("pred", one), kw.get("mask", one), kw.get("B", 2), kw.get("H", 41), kw.get("W", 57),
                         kw.get("taps", taps), -1.0, kw.get("scratch", one), kw.get("nbytes", 1 << 30), kw.get("out8", one),
                         kw.get("counts5", one), None]
    for bad in (dict(B=0), dict(H=15), dict(W=8), dict(B=65536), dict(H=65536, W=65536)):
        assert ev(*args(**bad)) == 1001
    for bad in (dict(ref=None), dict(pred=None), dict(taps=None), dict(scratch=None), dict(out8=None), dict(counts5=None)):
        assert ev(*args(**bad)) == 1002
    need = size("sifsrv_eval_metrics_scratch_bytes", 2, 41, 57)
    assert ev(*args(nbytes=need - 1)) == 1003 and ev(*args(nbytes=0)) == 1003 and ev(*args(nbytes=need - 1, mask=None)) == 1003

    ps = L.lib().sifsrv_psnr_ssim
    args = lambda **kw: [kw.get("pred", one), kw.get("targ", one), kw.get("valid", one), kw.get("scale", 4), kw.get("B", 2),
                         kw.get("H", 40), kw.get("W", 24), kw.get("scratch", one), kw.get("nbytes", 1 << 30), kw.get("out2", one),
                         kw.get("counts2", one), None]
    for bad in (dict(B=0), dict(H=6), dict(W=6), dict(scale=2), dict(scale=0), dict(H=42), dict(W=26), dict(B=65536)):
        assert ps(*args(**bad)) == 1001
    for bad in (dict(pred=None), dict(targ=None), dict(valid=None), dict(scratch=None), dict(out2=None), dict(counts2=None)):
        assert ps(*args(**bad)) == 1002
    need = size("sifsrv_psnr_ssim_scratch_bytes", 2, 40, 24)
    assert ps(*args(nbytes=need - 1)) == 1003 and ps(*args(nbytes=need - 1, scale=1, H=41, W=57)) == 1003


# ---- 3. the public names ---------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import metrics, train
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    assert sig(metrics.masked_aster_metrics) == [("reference", E_), ("prediction", E_), ("valid", None), ("data_range", None),
                                                 ("return_counts", False)]
    assert sig(metrics.masked_psnr_ssim)[:3] == [("predictions", E_), ("targets", E_), ("valid", E_)]
    assert all(d is not E_ for _, d in sig(metrics.masked_psnr_ssim)[3:])
    # the existing calls are what they were
    assert sig(metrics.aster_metrics) == [("reference", E_), ("prediction", E_), ("data_range", None)]
    assert sig(metrics.psnr_ssim) == [("predictions", E_), ("targets", E_)]
    for f in (train.train_epoch, train.eval_epoch, train.fit):
        assert sig(f)[-1] == ("masked_metrics", False)
    assert sig(train.train_epoch)[-2] == ("with_metrics", True) and sig(train.eval_epoch)[-2] == ("with_metrics", True)
    z = torch.zeros((1, 1, 16, 16))
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        metrics.masked_aster_metrics(z, z)
    with pytest.raises(sifsr.SifsrError):
        metrics.masked_psnr_ssim(z, z, torch.ones((1, 1, 4, 4), dtype=torch.uint8))
    assert os.path.samefile(sifsr._lib.header_path("scores"), os.path.join(ROOT, "include", "sifsr_scores.h"))
