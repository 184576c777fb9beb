"""CPU: Fourier scores for rasters of any size -- what can be held without a GPU.

  * tests/golden/golden_spectra_v1.json (the reference's compute_2D_attenuation_spectra and get_* on the rectangles of
    make_golden_spectra.CASES, written where the reference is) against the oracle: spectra at 1e-6 dB, as the generator asserted,
  * the score algebra of sifsr.spectra (the get_* functions of sifsr.fourier, RMSE_ATT over the whole spectrum, summary_rows)
    against
    the golden and against closed forms written out here in NumPy: the order statistic with linear interpolation that np.percentile
    and DataFrame.quantile share, and both standard deviations,
  * the pins of include/sifsr_spectra.h for the `sifsrf_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, the writing entry point has memory-contract cases in tests/test_spectra_gpu.py, the scratch size and the error codes
    through the host-only paths,
  * the public names."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests.capi_host import L  # noqa: F401  (the fixture)
from tests.golden.make_golden_spectra import CASES, SCORES, fourier_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_spectra_v1.json")))
TABLE = [(41, 41), (47, 53), (33, 65), (63, 31), (48, 100), (100, 256), (256, 100), (213, 198), (1000, 48), (1024, 36)]


# ---- 1. the golden file ----------------------------------------------------------------------------------------------------------
def test_golden_cases_are_the_table():
    assert [(c["seed"], c["H"], c["W"]) for c in GOLD["cases"]] == CASES
    assert [(h, w) for _, h, w in CASES] == TABLE


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_oracle_matches_reference_golden(idx):
    c = GOLD["cases"][idx]
    imgs = fourier_case(c["seed"], c["H"], c["W"])
    specs = [O.attenuation_spectrum(O.fft2_magnitude_shifted(im)) for im in imgs]
    for s, g in zip(specs, c["spectra"]):
        assert len(s) == len(g) == min(c["H"] // 2, c["W"] // 2)
        assert g[0] == 1.0 and np.allclose(s, g, rtol=0, atol=1e-6)
    rb, xb, pb = c["spectra"]
    assert np.allclose(O.frr_fro_fru(pb, rb, xb), [c["FRR"], c["FRO"], c["FRU"]], rtol=1e-9, atol=1e-12)


# ---- 2. the score algebra --------------------------------------------------------------------------------------------------------
def test_scores_match_reference_golden():
    from sifsr import spectra
    assert spectra.SCORES == SCORES
    for c in GOLD["cases"]:
        rb, xb, pb = c["spectra"]
        got = spectra.scores_from_spectra(rb, xb, pb)
        assert got.dtype == np.float64 and got.shape == (6,)
        assert np.allclose(got, [c[k] for k in SCORES], rtol=1e-9, atol=1e-12)
        # closed forms, written out
        rb, xb, pb = (np.array(v) for v in (rb, xb, pb))
        pfr = np.clip(rb - xb, 0, None).sum()
        afr = (np.maximum(np.minimum(pb, rb), np.minimum(xb, rb)) - np.minimum(rb, xb)).sum()
        want = [pfr, afr, afr / pfr, (rb - np.maximum(pb, rb)).sum() / rb.sum(), (xb - np.minimum(pb, xb)).sum() / xb.sum(),
                np.sqrt(((pb - rb) ** 2).sum() / len(rb))]
        assert np.allclose(got, want, rtol=1e-12, atol=1e-14)
        # element 0 (1 in every spectrum) is part of RMSE_ATT's mean: dropping it changes the figure
        assert abs(got[5] - np.sqrt(np.mean((pb[1:] - rb[1:]) ** 2))) > 1e-6
        # a prediction equal to the ASTER spectrum restores everything and deviates nowhere
        same = spectra.scores_from_spectra(rb, xb, rb)
        assert same[2] == 1.0 and same[3] == 0.0 and same[5] == 0.0


def _quantile(col, q):
    """the order statistic with linear interpolation: position (n - 1) q between the sorted values"""
    s = np.sort(col)
    pos = (len(s) - 1) * q
    lo = int(np.floor(pos))
    hi = min(lo + 1, len(s) - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - lo)


@pytest.mark.parametrize("n", [1, 2, 5, 83])
def test_summary_rows(n):
    from sifsr import spectra
    assert spectra.SUMMARY == ("mean", "std", "10%", "Q1", "mediane", "Q3", "90%")
    rs = np.random.RandomState(n)
    t = rs.standard_normal((n, 7, 6)) * 3 + 1
    for ddof in (0, 1):
        got = spectra.summary_rows(t, ddof)
        assert got.shape == (7, 7, 6) and got.dtype == np.float64
        flat, g = t.reshape(n, -1), got.reshape(7, -1)
        for j in range(flat.shape[1]):
            col = flat[:, j]
            mean = col.sum() / n
            assert np.isclose(g[0, j], mean, rtol=1e-12, atol=1e-14)
            if n > ddof:
                assert np.isclose(g[1, j], np.sqrt(((col - mean) ** 2).sum() / (n - ddof)), rtol=1e-12, atol=1e-14)
            else:
                assert np.isnan(g[1, j])                                          # pandas: the std of one row is NaN
            for row, q in zip(g[2:], (0.10, 0.25, 0.50, 0.75, 0.90)):
                assert np.isclose(row[j], _quantile(col, q), rtol=1e-12, atol=1e-14)
        assert np.array_equal(got[2:], np.percentile(t, [10, 25, 50, 75, 90], axis=0))
        assert np.array_equal(spectra.summary_rows(torch.from_numpy(t), ddof), got, equal_nan=True)
    # a single column (NumPy sums a contiguous column in another order than a strided one: rounding, not bits)
    assert np.allclose(spectra.summary_rows(t[:, 0, 0], 0), spectra.summary_rows(t, 0)[:, 0, 0], rtol=1e-12, atol=1e-14)
    import sifsr
    for bad in (lambda: spectra.summary_rows(t, 2), lambda: spectra.summary_rows(np.zeros((0, 4)), 0)):
        with pytest.raises(sifsr.SifsrError):
            bad()


# ---- 3. the pins of include/sifsr_spectra.h (the gate itself is tests/test_capi_gate.py) ----------------------------------------
def test_the_signatures_are_the_existing_entry_points(L):
    names = L.declared("spectra")
    assert names == ["sifsrf_fft2_attenuation", "sifsrf_fft2_attenuation_scratch_bytes"]
    # the two signatures differ from the existing entry points' in the name alone
    old, new = L.parse_header(), L.parse_header(L.header_path("spectra"))
    for n in names:
        assert new[n] == old[n.replace("sifsrf_", "sifsr_")]
        assert [(a.pointer, a.const) for a in new[n][1]] == [(a.pointer, a.const) for a in old[n.replace("sifsrf_", "sifsr_")][1]]


def test_the_writing_entry_point_has_contract_cases(L):
    from tests import test_spectra_gpu as T
    writers = L.writers("spectra")
    assert writers == {"sifsrf_fft2_attenuation": ["scratch", "mag", "spectrum"]}
    assert sorted(T.CONTRACT) == sorted(writers)
    assert {s[:3] for s in T.CONTRACT_SHAPES} == {(2, 41, 53), (1, 100, 256), (1, 33, 65)}
    # every shape with both outputs, with each one alone
    for shape in {s[:3] for s in T.CONTRACT_SHAPES}:
        assert {s[3:] for s in T.CONTRACT_SHAPES if s[:3] == shape} == {(True, True), (True, False), (False, True)}
    assert len(T.CONTRACT["sifsrf_fft2_attenuation"]) == len(T.CONTRACT_SHAPES)


def _chirp_m(n):
    if n & (n - 1) == 0:
        return 0
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def test_host_only_entry_points(L):
    """the scratch size; shape, argument and scratch errors are found before anything is launched (none needs a GPU)"""
    size = lambda *a: L.call("sifsrf_fft2_attenuation_scratch_bytes", *a)
    old = lambda *a: L.call("sifsr_fft2_attenuation_scratch_bytes", *a)
    for bad in ((1, 3, 64), (1, 64, 3), (1, 1025, 64), (1, 64, 1025), (1, 3000, 64), (0, 64, 64), (-1, 41, 41), (1, 4096, 64), (1, 0, 0)):
        assert size(*bad) == 0, bad
    for h, w in TABLE + [(4, 4), (5, 4), (1023, 1024), (2048, 1000), (2048, 2048), (64, 128)]:
        for b in (1, 3):
            need = size(b, h, w)
            assert need > 0
            # what the radix-2 entry point needs, plus one complex double per element of each chirp axis' filter spectrum
            extra = 16 * (_chirp_m(h) + _chirp_m(w))
            assert old(b, h, w) + extra <= need <= old(b, h, w) + extra + 15
            assert need >= b * h * w * 24 and size(b + 1, h, w) > need
    assert _chirp_m(33) == 128 == 4 * 33 - 4 and _chirp_m(1000) == 2048 and _chirp_m(63) == 128 and _chirp_m(41) == 128
    for h, w in ((64, 128), (256, 256), (2048, 4)):
        assert size(2, h, w) == (old(2, h, w) + 15) // 16 * 16
    one = ctypes.c_void_p(4096)
    fn = L.lib().sifsrf_fft2_attenuation
    args = lambda **kw: [kw.get("img", one), kw.get("B", 1), kw.get("H", 41), kw.get("W", 53), kw.get("scratch", one),
                         kw.get("nbytes", 1 << 40), kw.get("mag", one), kw.get("spectrum", one), None]
    for bad in (dict(H=3, W=64), dict(H=1025, W=64), dict(H=64, W=1025), dict(B=0), dict(H=3000, W=64), dict(W=3)):
        assert fn(*args(**bad)) == 1001, bad
    for bad in (dict(img=None), dict(scratch=None), dict(mag=None, spectrum=None)):
        assert fn(*args(**bad)) == 1002, bad
        assert L.lib().sifsr_fft2_attenuation(*args(H=64, W=64, **bad)) == 1002       # the code the existing function returns for it
    need = size(1, 41, 53)
    assert fn(*args(nbytes=need - 1)) == 1003 and fn(*args(nbytes=0)) == 1003 and fn(*args(nbytes=old(1, 41, 53))) == 1003
    assert L.lib().sifsr_fft2_attenuation(*args(H=64, W=64, nbytes=old(1, 64, 64) - 1)) == 1003


# ---- 4. the public names ---------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import spectra
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    assert sifsr.spectra is spectra
    assert sig(spectra.fft2_magnitude) == [("img", E_)] and sig(spectra.attenuation_spectra) == [("img", E_)]
    assert sig(spectra.spectral_scores) == [("aster", E_), ("bicubic", E_), ("predictions", E_)]
    assert sig(spectra.summary_rows) == [("table", E_), ("ddof", E_)]
    assert os.path.samefile(sifsr._lib.header_path("spectra"), os.path.join(ROOT, "include", "sifsr_spectra.h"))
    z = torch.zeros((41, 53))
    for call in (lambda: spectra.fft2_magnitude(z), lambda: spectra.attenuation_spectra([z, torch.zeros((64, 64))]),
                 lambda: spectra.spectral_scores(z, z, z[None]), lambda: spectra.spectral_scores([z], [z], [[z, z]])):
        with pytest.raises(sifsr.SifsrError):                                      # no CPU path
            call()
    # sifsr.fourier is what it was: same names, and its docstring still states the power-of-two limit
    assert "powers of two" in sifsr.fourier.__doc__ and spectra.fourier is sifsr.fourier
