"""CPU: the sensor model at any ratio -- what can be held without a GPU.

  * the restatement tests/degrade_reference.py reproduces every output of the reference recorded in
    tests/golden/golden_degrade_v1.npz (written where the reference is, by tests/golden/make_golden_degrade.py) from inputs it
    regenerates from their seeds, and its own properties: both clamps are exercised, the fp32 coordinate rule matters within the
    limits, validity by brute force over stencils, a constant raster stays that constant,
  * output sizes: sifsr.degrade.output_shape / sifsrs_out_shape against the reference's own sizes on the whole recorded sweep,
  * the pins of include/sifsr_degrade.h for the `sifsrs_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, the writing entry point has memory-contract cases in tests/test_degrade_gpu.py, the limits and error codes through the
    host-only paths,
  * the public names and the drop-in names exist."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import degrade_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_degrade_v1.npz")
# restatement against the reference's fp32 outputs: twice the largest deviation measured over the golden cases (3.080e-4 K, at
# coarse_97x131: a 529-term fp32 sum of unknown order near 300 K); a bar above 1e-3 K would mean the restatement is wrong
MEASURED_MAX = 3.080e-4
HOST_BAR = 6.2e-4


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_every_golden_output(gold):
    """measured: the largest |reference - restatement| over the golden cases is 3.080e-4 K (coarse_97x131); the bar is twice that"""
    assert list(gold["names"]) == [c[0] for c in R.CASES]
    worst = 0.0
    for name, kind, shape, factor, mtf, hkw, crop, _ in R.CASES:
        ref = gold[name + "_out"]
        mine, ov = R.degrade_ref(R.case_input(name), factor, mtf, hkw, crop)
        assert ref.dtype == np.float32 and ref.shape == mine.shape and ov.shape == mine.shape[-2:]
        d = float(np.abs(ref.astype(np.float64) - mine).max())
        print(f"{name}: {shape} -> {ref.shape}: max |reference - restatement| = {d:.3e} K")
        worst = max(worst, d)
    print(f"largest deviation {worst:.3e} K, bar {HOST_BAR:.1e} K")
    assert HOST_BAR < 1e-3 and 2 * MEASURED_MAX <= HOST_BAR < 2.1 * MEASURED_MAX
    assert worst <= HOST_BAR


def test_the_regenerated_inputs_are_the_golden_ones(gold):
    for c in R.CASES:
        x = R.case_input(c[0])
        assert x.dtype == np.float32 and x.shape == c[2] and R.checksum(x) == int(gold[c[0] + "_crc"]), c[0]
        assert 270 < x.min() and x.max() < 330


def test_output_sizes_are_the_reference_s(L, gold):
    from sifsr import degrade
    table = gold["shapes"]
    assert table.shape == (297 * 3 * 2, 5) and table[:, 0].min() == 4 and table[:, 0].max() == 300
    oh, ow = ctypes.c_int(), ctypes.c_int()
    seen = set()
    for side, fid, crop, hw, want in table.tolist():
        factor, hkw = R.SWEEP_FACTORS[fid]
        hkw = None if crop else hkw
        assert hw == R.half_width(factor, hkw)
        rc = L.lib().sifsrs_out_shape(side, side, factor, hkw or 0, crop, ctypes.byref(oh), ctypes.byref(ow))
        if want >= 1:
            assert rc == 0 and oh.value == ow.value == want, (side, fid, crop, oh.value, want)
            assert R.out_side(side, factor, hkw, bool(crop)) == want
            if side % 37 == 0:
                assert degrade.output_shape(side, side + 1, factor, hkw, bool(crop))[0] == want
        else:                                                          # the reference cannot pad the raster, or nothing is left
            assert rc == 1001 and (side < hw + 1 or R.out_side(side, factor, hkw, bool(crop)) < 1), (side, fid, crop)
        seen.add((fid, crop, want >= 1))
    assert len(seen) >= 8                                              # refusals and sizes, for every factor


def _sampled(ax):
    return ax["coef"] != 0


def test_both_clamps_are_exercised():
    """the fine 4 x 4 and 61 x 83 cases sample index -1 -> 0; factor 2 on an even padded side samples f + 2 = Np -> Np - 1"""
    for n in (4, 61, 83):
        ax = R.axis_operator(n, R.FINE)
        assert ((ax["raw"] < 0) & _sampled(ax)).any() and ax["idx"].min() == 0
    for n in (40, 52, 4):
        ax = R.axis_operator(n, 2.0, 0.1, 3)
        assert ax["n_pad"] % 2 == 0
        over = (ax["raw"] > ax["n_pad"] - 1) & _sampled(ax)
        assert over.any() and ax["raw"][over].max() == ax["n_pad"] and ax["idx"].max() == ax["n_pad"] - 1
    ax = R.axis_operator(97, R.COARSE)                                 # and a case that clamps at neither end
    assert not ((ax["raw"] < 0) | (ax["raw"] > ax["n_pad"] - 1)).any()


def test_fp32_coordinate_rule_matters_within_the_limits():
    """below output index 16384, floor of the fp32 source coordinate differs from floor of the float64 one at no index for
    926.25 / 90 and first at 1328 for 231.656 / 90; the 4 x 3415 strip is the smallest raster that reaches it, and the restatement
    follows the fp32 rule there"""
    first = {}
    for name, factor in (("coarse", R.COARSE), ("fine", R.FINE)):
        s32, s64, f, _ = R.coords(0, factor, 16384)
        differ = np.nonzero(f != np.floor(s64).astype(np.int64))[0]
        first[name] = int(differ[0]) if differ.size else None
    assert first == {"coarse": None, "fine": R.FP32_FLOOR_SPLIT}
    o = R.FP32_FLOOR_SPLIT
    case = [c for c in R.CASES if c[0] == "fine_4x3415"][0]
    assert R.out_side(case[2][1], R.FINE) == o + 1 and R.out_side(case[2][1] - 1, R.FINE) == o
    ax = R.axis_operator(case[2][1], R.FINE)
    s32, s64, f, t = R.coords(ax["n_pad"], R.FINE, o + 1)
    assert ax["raw"][o, 1] == f[o] == math.floor(s64[o]) + 1 and t[o] < 1e-3      # fp32 rounds up across the integer
    # it is the strip's last output: f + 2 is clamped and the stencil is folded at the high edge
    assert (ax["raw"][o] > ax["n_pad"] - 1).sum() == 1 and np.nonzero(ax["R"][o])[0][-1] == case[2][1] - 1


def test_validity_by_brute_force():
    H, W = 40, 52
    valid = R.quad_valid(H, W)
    assert 0.3 < valid.mean() < 0.7 and valid[0, 0] == 0 and valid[H // 2, W // 2] == 1
    x = R.make_field((H, W), 3)
    for factor, hkw, crop in ((R.FINE, None, False), (2.0, 3, False), (R.COARSE, None, False), (4.0, None, True), (3.0, None, True)):
        out, ov = R.degrade_ref(x, factor, 0.1, hkw, crop, valid, fill_value=-1.0)
        ay, ax = R.axis_operator(H, factor, 0.1, hkw, crop), R.axis_operator(W, factor, 0.1, hkw, crop)
        want = np.zeros_like(ov)
        for oy in range(ov.shape[0]):
            ys = np.nonzero(ay["R"][oy])[0]
            for ox in range(ov.shape[1]):
                xs = np.nonzero(ax["R"][ox])[0]
                reads_ring = any(c != 0 and (q < a["hw"] or q > a["n_pad"] - 1 - a["hw"])
                                 for a, o in ((ay, oy), (ax, ox)) for q, c in zip(a["idx"][o], a["coef"][o]))
                want[oy, ox] = valid[np.ix_(ys, xs)].all() and not reads_ring
                assert len(ys) <= 2 * ay["hw"] + 4 and np.array_equal(ys, np.arange(ys[0], ys[-1] + 1))   # one run of pixels
        assert np.array_equal(ov, want) and (out[~ov] == -1.0).all() and (out[ov] > 200).all()
        if factor != R.COARSE:
            assert 0 < ov.sum() < ov.size
        # what the invalid pixels hold changes nothing
        for junk in (np.nan, 0.0, 1e30):
            p = x.copy()
            p[valid == 0] = junk
            assert np.array_equal(R.degrade_ref(p, factor, 0.1, hkw, crop, valid, fill_value=-1.0)[0], out)
    # without a map the ring is still marked and every value is computed
    out, ov = R.degrade_ref(x, R.FINE)
    assert not ov[0].any() and not ov[:, -1].any() and ov[2:-2, 2:-2].all() and np.isfinite(out).all()


def test_a_constant_raster_stays_that_constant():
    for factor, hkw, crop in ((R.COARSE, None, False), (R.FINE, None, False), (2.0, 3, False), (4.0, None, True)):
        x = np.full((61, 83), 301.25, np.float32)
        out, ov = R.degrade_ref(x, factor, 0.1, hkw, crop)
        assert ov.any() and np.abs(out[ov] - 301.25).max() < 1e-10
        if crop:
            assert ov.all()                                                   # the /4 cut removes exactly the outputs that met the ring
        else:
            assert (np.abs(out[~ov] - 301.25) > 1e-6).all() and out[0, 0] < 200   # the ring met zeros (the cubic's lobes can overshoot)


# ---- 2. the pins of include/sifsr_degrade.h (the gate itself is tests/test_capi_gate.py) ----------------------------------------
def test_the_writing_entry_point_has_contract_cases(L):
    from tests import test_degrade_gpu as T
    names, decl = L.declared("degrade"), L.writers("degrade")
    assert names == ["sifsrs_degrade", "sifsrs_out_shape", "sifsrs_workspace_bytes"]
    assert decl["sifsrs_out_shape"] == ["oh", "ow"] and "sifsrs_workspace_bytes" not in decl       # host only: two ints on the host
    writers = {n: p for n, p in decl.items() if p and n != "sifsrs_out_shape"}
    assert writers == {"sifsrs_degrade": ["out", "out_valid", "workspace"]}
    assert sorted(T.CONTRACT) == sorted(writers)
    assert all(len(cases) >= 4 for cases in T.CONTRACT.values())
    # (with valid, with out_valid) in all four combinations, crop off and on, more than one image
    assert {(s[6], s[7]) for s in T.CONTRACT_SHAPES} == {(False, False), (True, False), (False, True), (True, True)}
    assert {s[5] for s in T.CONTRACT_SHAPES} == {False, True} and any(s[0] > 1 for s in T.CONTRACT_SHAPES)


def test_host_only_entry_points(L):
    """sizes, and every limit of the header: shape, argument and workspace errors are found before anything is launched"""
    lib = L.lib()
    oh, ow = ctypes.c_int(-7), ctypes.c_int(-7)
    shape = lambda h, w, f, hkw=0, crop=0: lib.sifsrs_out_shape(h, w, f, hkw, crop, ctypes.byref(oh), ctypes.byref(ow))
    size = lambda B, h, w, f, hkw=0, crop=0: lib.sifsrs_workspace_bytes(B, h, w, f, hkw, crop)
    assert shape(700, 830, R.COARSE) == 0 and (oh.value, ow.value) == (70, 82)
    assert shape(700, 830, R.FINE) == 0 and (oh.value, ow.value) == (274, 324)
    assert shape(40, 52, 2.0, 3) == 0 and (oh.value, ow.value) == (23, 29)
    assert shape(40, 52, 4.0, 0, 1) == 0 and (oh.value, ow.value) == (10, 13)
    assert shape(16384, 16384, 16.0) == 0 and shape(17, 17, 3.7, 16) == 0 and shape(2, 2, 1.0001, 1) == 0
    assert lib.sifsrs_out_shape(40, 52, 2.0, 3, 0, None, ctypes.byref(ow)) == 1002
    assert lib.sifsrs_out_shape(40, 52, 2.0, 3, 0, ctypes.byref(oh), None) == 1002
    bad = [(11, 40, R.COARSE, 0, 0), (40, 11, R.COARSE, 0, 0), (3, 9, R.FINE, 0, 0), (16385, 40, 2.0, 0, 0), (40, 16385, 2.0, 0, 0),
           (40, 52, 1.0, 0, 0), (40, 52, 0.5, 0, 0), (40, 52, -2.0, 0, 0), (40, 52, 16.5, 0, 0), (40, 52, float("nan"), 0, 0),
           (40, 52, float("inf"), 0, 0), (40, 52, 2.0, 17, 0), (40, 52, 2.0, -1, 0), (40, 52, 2.0, 3, 2), (40, 52, 2.0, 3, -1),
           (0, 0, 2.0, 0, 0), (-5, 40, 2.0, 0, 0),
           (4, 9, 15.0, 3, 0)]                            # 10 padded rows at factor 15 give no output
    assert shape(12, 40, R.COARSE, 0, 1) == 0 and oh.value == 1         # 34 padded rows -> 3 outputs, the crop takes 2: one is left
    for b in bad:
        assert shape(*b) == 1001 and size(1, *b) == 0, b
    for h, w, f, hkw, crop, B in ((700, 830, R.COARSE, 0, 0, 1), (700, 830, R.FINE, 0, 0, 64), (40, 52, 2.0, 3, 0, 6), (4, 4, R.FINE, 0, 0, 1)):
        assert shape(h, w, f, hkw, crop) == 0
        K = 2 * R.half_width(f, hkw or None) + 4
        # float64 weights and one int4 per output on both axes, the (B, oh, w) float64 intermediate and its validity bytes
        least = (oh.value + ow.value) * (8 * K + 16) + 9 * B * oh.value * w
        assert least <= size(B, h, w, f, hkw, crop) <= least + 64
    assert size(0, 40, 52, 2.0) == 0 and size(65536, 40, 52, 2.0) == 0 and size(65535, 40, 52, 2.0) > 0
    one = ctypes.c_void_p(4096)
    fn = lib.sifsrs_degrade
    args = lambda **kw: [kw.get("x", one), kw.get("valid", one), kw.get("out", one), kw.get("out_valid", one), kw.get("ws", one),
                         kw.get("nbytes", 1 << 40), kw.get("B", 2), kw.get("h", 40), kw.get("w", 52), kw.get("factor", 2.0),
                         kw.get("mtf", 0.1), kw.get("hkw", 3), kw.get("crop", 0), kw.get("fill", 0.0), None]
    for b in (dict(h=3), dict(w=3), dict(h=16385), dict(w=16385), dict(factor=1.0), dict(factor=16.5), dict(factor=float("nan")),
              dict(hkw=17), dict(hkw=-1), dict(factor=16.5, hkw=2), dict(mtf=0.0), dict(mtf=1.0), dict(mtf=-0.1), dict(mtf=float("nan")),
              dict(B=0), dict(B=65536), dict(crop=2), dict(h=4, w=9, factor=15.0)):
        assert fn(*args(**b)) == 1001, b
    for b in (dict(x=None), dict(out=None), dict(ws=None), dict(ws=ctypes.c_void_p(4104)), dict(x=ctypes.c_void_p(4098)),
              dict(out=ctypes.c_void_p(4097))):
        assert fn(*args(**b)) == 1002, b
    need = size(2, 40, 52, 2.0, 3, 0)
    assert fn(*args(nbytes=need - 1)) == 1003 and fn(*args(nbytes=0)) == 1003 and fn(*args(nbytes=need - 1, valid=None, out_valid=None)) == 1003
    assert fn(*args(nbytes=size(1, 40, 52, 2.0, 3, 0))) == 1003


# ---- 3. the public names ---------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import degrade
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    got = sig(degrade.degrade)
    assert got[:6] == [("x", E_), ("factor", E_), ("mtf", 0.1), ("hkw", None), ("crop", False), ("valid", None)]
    assert got[6][0] == "fill_value" and math.isnan(got[6][1]) and got[7] == ("return_valid", False) and len(got) == 8
    assert sig(degrade.output_shape) == [("h", E_), ("w", E_), ("factor", E_), ("hkw", None), ("crop", False)]
    assert sig(degrade.aster_to_coarse) == sig(degrade.aster_to_fine) == [("x", E_), ("valid", None)]
    assert sig(degrade.generic_downscale) == [("x", E_), ("factor", 2.0), ("mtf", 0.1), ("hkw", 3)]
    assert sig(degrade.simulate_pair) == [("aster_90m", E_), ("valid", None)]
    assert degrade.COARSE_FACTOR == 926.25 / 90 and degrade.FINE_FACTOR == 231.656 / 90
    assert sifsr.degrade is degrade                                          # the module; its function is sifsr.degrade.degrade
    for name in ("aster_to_coarse", "aster_to_fine", "generic_downscale", "simulate_pair"):
        assert getattr(sifsr, name) is getattr(degrade, name)
    assert degrade.output_shape(700, 830, degrade.COARSE_FACTOR) == (70, 82)
    assert degrade.output_shape(40, 52, 4, crop=True) == (10, 13)
    z = torch.zeros((40, 52))
    for bad in (lambda: degrade.degrade(z, 2.0), lambda: degrade.aster_to_coarse(z), lambda: degrade.aster_to_fine(z),
                lambda: degrade.generic_downscale(z[None, None]), lambda: degrade.simulate_pair(z),
                lambda: degrade.output_shape(11, 40, degrade.COARSE_FACTOR), lambda: degrade.output_shape(40, 52, 1.0),
                lambda: degrade.output_shape(40, 52, 2.0, hkw=17), lambda: degrade.output_shape(40, 52, 16.5)):
        with pytest.raises(sifsr.SifsrError):                                  # no CPU path; limits before anything runs
            bad()
    with pytest.raises(NotImplementedError):
        degrade.degrade(torch.zeros((40, 52), requires_grad=True), 2.0)
    # the /4 operator keeps its refusals
    with pytest.raises(NotImplementedError):
        sifsr.sif_ops._taps_c(0.1, 2, None)
    assert os.path.samefile(sifsr._lib.header_path("degrade"), os.path.join(ROOT, "include", "sifsr_degrade.h"))


def test_dropin_names_resolve():
    import importlib
    saved = {k: sys.modules.pop(k, None) for k in ("model", "dataset", "utils")}
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        us = importlib.import_module("utils")
        E_ = inspect.Parameter.empty
        sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
        assert sig(us.downscale_Aster_to_coarse) == [("data", E_), ("factor", 926.25 / 90), ("mtf", 0.1), ("padding", "same"), ("hkw", None)]
        assert sig(us.downscale_Aster_to_fine) == [("data", E_), ("factor", 231.656 / 90), ("mtf", 0.1), ("padding", "same"), ("hkw", None)]
        assert sig(us.generic_downscale) == [("data", E_), ("factor", 2.0), ("mtf", 0.1), ("padding", "same"), ("hkw", 3)]
        for name in ("downscale_Aster_to_coarse", "downscale_Aster_to_fine", "generic_downscale"):
            assert hasattr(us, name) and callable(getattr(us, name))
        with pytest.raises(us.OutOfScopeAttribute):                            # what is out of scope still says so
            us.find_corners
        with pytest.raises(NotImplementedError, match="padding"):
            us.generic_downscale(torch.zeros(1, 1, 8, 8), padding="valid")
        with pytest.raises(ValueError):
            us.downscale_Aster_to_fine(np.zeros((2, 8, 8), np.float32))
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v
