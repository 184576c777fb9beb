"""CPU: the sharpening baselines at any ratio -- what can be held without a GPU.

  * tests/rbaselines_reference.py (the float64 restatement the GPU tests compare with) reproduces the reference's own images,
    Gamma_coarse and kriging weights at scales 2 and 3 (tests/golden/golden_rbaselines_v1.npz) when given the reference's fit 2,
    and at scale 4 it is tests/baselines_reference.py and tests/dms_reference.py.  Margins: 1e-9 K on images and 1e-9 relative on
    Gamma_coarse and the weights -- those with which tests/test_baselines_host.py and tests/test_dms_host.py hold their own goldens,
  * sifsr.rbaselines' host side: its kriging geometry at s = 4 is sifsr.baselines', its own fits on the golden Gamma_coarse give
    the reference's image at the project's parity bar, the geometry rules and their error texts,
  * the gate of csrc/rbaselines_api.h, a header outside sifsr._lib.FAMILIES: the library exports exactly the declared `sifsrh_`
    names, the binding carries them with the declared types, every entry point that can write through a pointer has a row in the
    CONTRACT of tests/test_rbaselines_gpu.py, and the table of families is untouched,
  * what stays: CPU tensors raise SifsrError, sifsr.baselines and the drop-ins still refuse x3.

Four tests here pin the YARDSTICK and not the product, so they need nothing of the feature but the test-side files it adds:
test_restatement_at_scale_4_is_the_existing_restatements, test_dms_restatement_at_scale_4_and_at_5_over_2 and
test_the_gather_bicubic_is_the_resampling_matrix hold tests/rbaselines_reference.py to the restatements that were there, and
test_the_dropins_still_refuse_scale_3 holds behaviour that must not change.  Every other test needs the module, the header, the
exported symbols or the golden."""
import ctypes
import importlib
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from tests import baselines_reference as R4
from tests import dms_reference as D4
from tests import rbaselines_reference as R
from tests.capi_host import L, exported  # noqa: F401  (L is the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (2, 3)
KRIGING = [(s, i, m) for s in SCALES for i in (0, 1) for m in ("atprk", "aatprk")]
VARIO = (15.5, 4450.0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_rbaselines_v1.npz"))


@pytest.fixture(scope="module")
def RB(L):
    from sifsr import rbaselines
    return rbaselines


def _case(golden, s, i):
    return tuple(golden[f"s{s}_c{i}_{k}"].astype(np.float64) for k in ("lst", "ndvi_coarse", "ndvi_fine"))


# ---- 1. the golden and the restatement --------------------------------------------------------------------------------------------
def test_golden_holds_what_it_should(golden):
    assert float(golden["min_T"]) == 273.0 and float(golden["scc"]) == 926.0 and tuple(golden["scales"]) == SCALES
    assert np.allclose(golden["distances"], 926.0 * np.sqrt(np.array(R.KS, dtype=np.float64)), rtol=1e-14)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_rbaselines_v1.npz")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_dms_v1.npz"))
    for s in SCALES:
        for i in (0, 1, 2):
            lst, nc, nf = _case(golden, s, i)
            assert lst.shape == nc.shape == (16, 16) and nf.shape == (16 * s, 16 * s) and golden[f"s{s}_c{i}_lst"].dtype == np.float32
            assert ((lst == 0).sum() == 6) == (i in (0, 2))
        lst, nc, nf = _case(golden, s, 2)
        assert ((lst > 0) & (lst < 273)).sum() == 3 and np.isnan(nc).sum() == 1 and np.isnan(nf).sum() == s * s
        for i in (0, 1):
            for m in ("atprk", "aatprk"):
                pre = f"s{s}_c{i}_{m}"
                assert np.isfinite(golden[pre + "_fit2"]).all() and (golden[pre + "_fit2"] > 0).all()
                assert golden[pre + "_lambdas"].shape == (s * s, 25) and golden[pre + "_gamma"].shape == (15,)
                assert np.isfinite(golden[pre]).all() and golden[pre].shape == (16 * s, 16 * s)
            assert float(golden[f"s{s}_c{i}_atprk_restart_moved"]) < 1e-4


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_restatement_tsharp(golden, s, i):
    ref = golden[f"s{s}_c{i}_tsharp"]
    out = R.tsharp(*_case(golden, s, i), min_T=273.0)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan) and nan.sum() == (2 * s * s if i == 2 else 0)
    assert np.abs(out - ref)[~nan].max() <= 1e-9


@pytest.mark.parametrize("s,i,method", KRIGING)
def test_restatement_kriging(golden, s, i, method):
    """with the reference's recorded fit 2: images to 1e-9 K, Gamma_coarse to 1e-9 relative, the weights of kriging_weights(s)
    to 1e-9, the image from the recorded weights; the regularised model is the one the reference's second fit minimised"""
    pre = f"s{s}_c{i}_{method}"
    ref, gref, fit2, lref = golden[pre], golden[pre + "_gamma"], golden[pre + "_fit2"], golden[pre + "_lambdas"]
    out, g = getattr(R, method)(*_case(golden, s, i), variogram=fit2, scc=926.0, min_T=273.0)
    err = np.abs(out - ref).max()
    print(f"restatement {method} x{s} case {i}: max |out - ref| = {err:.3e} K")
    assert err <= 1e-9
    assert np.array_equal(g == 0, gref == 0) and (np.abs(g - gref)[1:] / gref[1:]).max() <= 1e-9
    out_l, _ = getattr(R, method)(*_case(golden, s, i), variogram=fit2, scc=926.0, min_T=273.0, lambdas=lref)
    assert np.abs(out_l - ref).max() <= 1e-9
    assert np.abs(R.kriging_weights(fit2[0], fit2[1], 926.0, s) - lref).max() <= 1e-9
    cost = lambda p: float(((R.regularised_model(p[0], p[1], 926.0, s) - gref) ** 2).sum())
    c0 = cost(fit2)
    for ds, dr in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
        assert cost((fit2[0] * (1 + ds), fit2[1] * (1 + dr))) >= c0 * (1 - 1e-6)


def _x4_inputs(h, w, seed):
    rs = np.random.RandomState(seed)
    nf = np.clip(0.4 + 0.3 * rs.standard_normal((4 * h, 4 * w)), -1, 1).astype(np.float32).astype(np.float64)
    nc = (((nf.reshape(h, 4, w, 4) ** 4).sum((1, 3)) / 16) ** 0.25).astype(np.float32).astype(np.float64)
    lst = (310 - 12 * nc + rs.standard_normal((h, w))).astype(np.float32).astype(np.float64)
    lst[1:3, 2:4] = 0.0
    return lst, nc, nf


def test_restatement_at_scale_4_is_the_existing_restatements():
    lst, nc, nf = _x4_inputs(9, 12, 7)
    assert np.array_equal(R.fine_distances(926.0, 4), R4.fine_distances(926.0))
    assert np.abs(R.kriging_weights(*VARIO, 926.0, 4) - R4.kriging_weights(*VARIO, 926.0)).max() <= 1e-9
    assert np.abs(R.regularised_model(*VARIO, 926.0, 4) - R4.regularised_model(*VARIO, 926.0)).max() <= 1e-9 * VARIO[0]
    assert np.abs(R.tsharp(lst, nc, nf) - R4.tsharp(lst, nc, nf)).max() <= 1e-9
    for m in ("atprk", "aatprk"):
        a, ga = getattr(R, m)(lst, nc, nf, VARIO)
        b, gb = getattr(R4, m)(lst, nc, nf, VARIO)
        assert np.abs(a - b).max() <= 1e-9 and np.array_equal(ga, gb)
    nf[5:9, 3:6] = np.nan                                                     # a whole cell and part of one
    for pow4 in (False, True):
        for a, b in zip(R.aggregate(nf, (9, 12), pow4), D4.aggregate(nf, pow4)):
            assert np.array_equal(a, b, equal_nan=True)
    sr = (300 + 5 * np.random.RandomState(3).standard_normal(nf.shape)).astype(np.float32)
    lst = np.where(lst == 0, 300.0, lst)                                      # (a radicand near 0 has no stable fourth root)
    # stage 5 at x4 before the float32 store: the gather bicubic against the x4 restatement's, at its own margin (1e-9 relative)
    res = (lst * lst) * (lst * lst) - D4.aggregate(sr, pow4=True)[0]
    up, up4 = R.bicubic(res, sr.shape), D4.bicubic_up4(res)
    assert np.abs(up - up4).max() <= 1e-9 * np.abs(up4).max()
    rad, rad4 = up + sr.astype(np.float64) ** 4, up4 + sr.astype(np.float64) ** 4
    assert (np.abs(rad ** 0.25 - rad4 ** 0.25) / rad4 ** 0.25).max() <= 1e-9
    a, b = R.correct(lst, sr), D4.correct(lst, sr)
    assert a.dtype == b.dtype == np.float32 and np.array_equal(np.isnan(a), np.isnan(b))
    assert np.nanmax(np.abs(a.astype(np.float64) - b)) <= 1e-4               # two float32 roundings of the same float64 value


def test_dms_restatement_at_scale_4_and_at_5_over_2():
    rs = np.random.RandomState(11)
    lst, _, nf = _x4_inputs(8, 8, 5)
    lst = np.where(lst == 0, 300.0, lst)
    counts = rs.poisson(1.0, (2, 64))
    a, ia = R.dms(lst, nf, counts)
    b, ib = D4.dms(lst, nf, counts)
    assert ia["ts"]["n_train"] == ib["ts"]["n_train"] >= 10 and np.array_equal(ia["sr"], ib["sr"], equal_nan=True)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a.astype(np.float64) - b)) <= 1e-4
    # 5 / 2 on (6, 8): cells of 2 or 3 pixels per axis; the cell means of the corrected image's fourth power return lst^4
    nf = np.clip(0.4 + 0.3 * rs.standard_normal((15, 20)), -1, 1).astype(np.float32).astype(np.float64)
    mean, _ = R.aggregate(nf, (6, 8))
    assert mean[0, 0] == (nf[0, 0] + nf[0, 1] + nf[0, 2] + nf[1, 0] + nf[1, 1] + nf[1, 2] + nf[2, 0] + nf[2, 1] + nf[2, 2]) / 9
    assert mean[1, 1] == (nf[3, 3] + nf[3, 4] + nf[4, 3] + nf[4, 4]) / 4
    assert list(R.cells(6, 15)) == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 5, 5]
    lst = (300 + 8 * mean + rs.standard_normal((6, 8))).astype(np.float32).astype(np.float64)
    out, info = R.dms(lst, nf, rs.poisson(1.0, (3, 48)))
    assert out.shape == (15, 20) and info["ts"]["n_train"] >= 10 and np.isfinite(out).all()
    m4, _ = R.aggregate(out, (6, 8), pow4=True)                               # the correction returns most of the residual
    assert np.abs(m4 ** 0.25 - lst).max() < np.abs(R.aggregate(info["sr"], (6, 8), pow4=True)[0] ** 0.25 - lst).max()


def test_the_gather_bicubic_is_the_resampling_matrix():
    """the restatement's bicubic in gather form (so that a NaN keeps to its footprint) is tests/ratio_reference.upsample_ref"""
    from tests import ratio_reference as RR
    x = np.random.RandomState(2).standard_normal((6, 9)) * 1e9
    for shape in ((15, 24), (16, 24), (12, 18), (48, 72)):
        a, b = R.bicubic(x, shape), RR.upsample_ref(x, shape)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    y = x.copy()
    y[2, 3] = np.nan
    assert np.isnan(R.bicubic(y, (16, 24))).sum() <= (4 * 8 // 3 + 3) ** 2 and np.isnan(RR.upsample_ref(y, (16, 24))).sum() > 200


# ---- 2. the host side of sifsr.rbaselines -----------------------------------------------------------------------------------------
def test_host_geometry_at_scale_4_is_baselines(RB):
    from sifsr import baselines as BL
    for sill, ran in (VARIO, (7.0, 1000.0), (31.9, 3999.3)):
        assert np.array_equal(RB.kriging_weights(sill, ran, 926.0, 4), BL.kriging_weights(sill, ran, 926.0))
        assert np.array_equal(RB.regularised_model(sill, ran, 926.0, 4), BL.regularised_model(sill, ran, 926.0))
    assert RB._geometry(4) is RB._geometry(4)                                  # built once per scale
    for s in range(2, 9):
        lam = RB.kriging_weights(*VARIO, 926.0, s)
        assert lam.shape == (s * s, 25) and np.abs(lam.sum(1) - 1).max() <= 1e-9          # unbiased: the weights sum to 1
        assert np.abs(lam - R.kriging_weights(*VARIO, 926.0, s)).max() <= 1e-9
        assert np.abs(RB.regularised_model(*VARIO, 926.0, s) - R.regularised_model(*VARIO, 926.0, s)).max() <= 1e-9 * VARIO[0]
    with pytest.raises(ValueError, match="scale"):
        RB.kriging_weights(*VARIO, 926.0, 9)


@pytest.mark.parametrize("s,i,method", KRIGING)
def test_host_fit_gives_the_reference_image(RB, golden, s, i, method):
    """rbaselines.fit_variogram + kriging_weights on the golden Gamma_coarse -> image through the restatement, against the
    reference's: the project's parity bar, 1e-4 of the image's maximum (tests/test_baselines_host.py)"""
    pre = f"s{s}_c{i}_{method}"
    ref, gref = golden[pre], golden[pre + "_gamma"]
    fit1, fit2 = RB.fit_variogram(gref, 926.0, 7.0, 1000.0, s)
    assert np.isfinite(fit2).all() and (fit2 > 0).all()
    lam = RB.kriging_weights(fit2[0], fit2[1], 926.0, s)
    out, _ = getattr(R, method)(*_case(golden, s, i), variogram=fit2, scc=926.0, min_T=273.0, lambdas=lam)
    err = np.abs(out - ref).max()
    print(f"host fit {method} x{s} case {i}: fit1 {fit1} fit2 {fit2} (reference {golden[pre + '_fit1']} {golden[pre + '_fit2']}); "
          f"max |image - ref| = {err:.3e} K = {err / np.abs(ref).max():.3e} of the maximum")
    assert err <= 1e-4 * np.abs(ref).max()


def test_geometry_rules_and_their_error_texts(RB):
    assert RB.geometry((6, 8), (15, 20)) == (5, 2) and RB.geometry((6, 9), (16, 24)) == (8, 3)
    assert RB.geometry((5, 7), (40, 56)) == (8, 1) and RB.geometry((16, 16), (32, 32)) == (2, 1)
    with pytest.raises(ValueError, match="multiples of 2"):
        RB.geometry((6, 7), (15, 18))                                          # 5 / 2 with an odd coarse width
    with pytest.raises(ValueError, match="at most 8"):
        RB.geometry((5, 5), (45, 45))
    with pytest.raises(ValueError, match="above 1"):
        RB.geometry((8, 8), (8, 8))
    with pytest.raises(ValueError, match="above 1"):
        RB.geometry((8, 8), (4, 4))
    with pytest.raises(ValueError, match="per-axis"):
        RB.geometry((6, 8), (15, 24))                                          # 5 / 2 down, 3 across
    with pytest.raises(ValueError, match="per-axis"):
        RB.geometry((8, 8), (16, 24))


def test_public_interface_and_refusals(RB, monkeypatch):
    import sifsr
    from sifsr import baselines as BL
    assert sifsr.rbaselines is RB
    for name in ("tsharp", "atprk", "aatprk", "dms", "dms_model", "dms_apply"):
        assert inspect.signature(getattr(RB, name)) == inspect.signature(getattr(BL, name)), name
    # dms_aggregate: baselines' parameters, kinds and defaults, then the one addition -- a keyword-only coarse shape, since one
    # raster does not tell the ratio
    new, old = inspect.signature(RB.dms_aggregate).parameters, inspect.signature(BL.dms_aggregate).parameters
    assert list(new) == list(old) + ["coarse"] and all(new[k] == old[k] for k in old)
    assert new["coarse"].kind is inspect.Parameter.KEYWORD_ONLY and new["coarse"].default is None
    z = torch.zeros((1, 1, 8, 8))
    E = sifsr.SifsrError
    for fine in (torch.zeros((1, 1, 24, 24)), torch.zeros((1, 1, 20, 20))):
        for fn in (RB.tsharp, RB.atprk, RB.aatprk):
            with pytest.raises(E):                                             # no CPU path
                fn(z, z, fine)
        with pytest.raises(E):
            RB.dms(z, fine)
        with pytest.raises(E):
            RB.dms_aggregate(fine, coarse=(8, 8))
    # past the device check, the rules are checked on the host before any launch
    monkeypatch.setattr(sifsr._lib, "require_gpu", lambda t, what="tensor": None)
    for fn in (RB.atprk, RB.aatprk):
        with pytest.raises(NotImplementedError, match="integer scales"):
            fn(z, z, torch.zeros((1, 1, 20, 20)))                              # 5 / 2
    with pytest.raises(ValueError, match="per-axis"):
        RB.tsharp(z, z, torch.zeros((1, 1, 16, 24)))
    with pytest.raises(ValueError, match="at least 5 x 5"):
        RB.tsharp(z[:, :, :4], z[:, :, :4], torch.zeros((1, 1, 8, 16)))
    with pytest.raises(ValueError, match="coarse="):
        RB.dms_aggregate(torch.zeros((1, 1, 24, 24)))
    with pytest.raises(ValueError, match=r"expected \(B,1,H,W\)"):
        RB.dms_aggregate(torch.zeros((1, 24, 24)), coarse=(8, 8))
    with pytest.raises(E):
        RB.dms_aggregate(np.zeros((1, 1, 24, 24)), coarse=(8, 8))
    with pytest.raises(NotImplementedError):
        RB.dms(z, torch.zeros((1, 1, 24, 24)), moving_window_size=3)
    with pytest.raises(NotImplementedError):
        RB.dms(z, torch.zeros((1, 2, 24, 24)))
    # sifsr.baselines keeps refusing anything but x4
    for fn in (BL.tsharp, BL.atprk, BL.aatprk):
        with pytest.raises(ValueError, match="exactly 4x"):
            fn(z, z, torch.zeros((1, 1, 24, 24)))
    with pytest.raises(ValueError, match="exactly 4x"):
        BL.dms(z, torch.zeros((1, 1, 24, 24)))


def test_the_dropins_still_refuse_scale_3():
    saved = {k: sys.modules.pop(k, None) for k in ("model", "dataset", "utils")}
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        us = importlib.import_module("utils")
        a, f = np.zeros((8, 8)), np.zeros((24, 24))
        for fn, args in ((us.TsHARP, (a, a, f, 3)), (us.ATPRK, (a, a, f, 3, 926)), (us.AATPRK, (a, a, f, 3, 926)), (us.DMS, (a, f, 3))):
            with pytest.raises(NotImplementedError, match="scale"):
                fn(*args)
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


# ---- 3. the gate of csrc/rbaselines_api.h -----------------------------------------------------------------------------------------
NAMES = ["sifsrh_aggregate", "sifsrh_correct", "sifsrh_predict", "sifsrh_sharpen"]


def test_exported_symbols_are_the_declared_ones(L, RB):
    decls = L.parse_header(RB.API_HEADER)
    assert sorted(decls) == NAMES and os.path.dirname(RB.API_HEADER).endswith("csrc")
    assert {n for n in exported(L.LIB_PATH) if n.startswith("sifsrh_")} == set(NAMES)
    # outside every family of the table, and outside the core header's export check
    assert len(L.FAMILIES) == 18 and not any(p.startswith("sifsrh") or "sifsrh_".startswith(p) for _, p in L.FAMILIES.values())
    assert not [n for n in NAMES if "sifsr_" in n]
    assert not os.path.exists(os.path.join(ROOT, "include", "rbaselines_api.h"))
    assert not set(NAMES) & {n for f in L.FAMILIES for n in L.declared(f)}
    bound = RB.bound()
    assert sorted(bound) == NAMES and RB.bound() is bound                      # bound once
    for n, (ret, args) in decls.items():
        fn = getattr(L.lib(), n)
        assert fn.restype is ret is ctypes.c_int, n
        assert list(fn.argtypes) == [t for _, t in args] and len(args) >= 10, n
        assert args[-1][0] == "stream" and args[-1].pointer
    assert L.call("sifsr_abi_version") == L.ABI_VERSION == 3


def test_every_writing_entry_point_has_a_contract_case(L, RB):
    from tests import test_rbaselines_gpu as T
    writers = {}
    for name, (_, args) in L.parse_header(RB.API_HEADER).items():
        ptrs = [a[0] for a in args if a.pointer and not a.const and a[0] != "stream"]
        if ptrs:
            writers[name] = ptrs
    assert writers == {"sifsrh_aggregate": ["mean", "std"], "sifsrh_sharpen": ["out"], "sifsrh_predict": ["sr"],
                       "sifsrh_correct": ["out"]}
    assert set(T.CONTRACT) == set(writers) and all(len(cases) >= 3 for cases in T.CONTRACT.values())
