"""CPU: the differentiable sensor model at any ratio -- what can be held without a GPU.

  * the restatement tests/sensor_reference.py reproduces every output and every autograd gradient of the reference recorded in
    tests/golden/golden_sensor_v1.npz (written where the reference is, by tests/golden/make_golden_sensor.py) from inputs and
    cotangents it regenerates from their seeds; the adjoint identity in float64,
  * stencil monotonicity and contiguity over a sweep of sides, factors, half widths and crops: what the device's range table
    (one run of outputs per input pixel, found by bisection) rests on,
  * the pins of include/sifsr_sensor.h for the `sifsrt_` entry points (the gate itself is tests/test_capi_gate.py): the row, the
    declared names, the writers, which entry points are host only, and what the memory-contract cases of tests/test_sensor_gpu.py cover,
  * the public names of sifsr.sensor and the error paths that need no GPU."""
import ctypes
import importlib
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import degrade_reference as R
from tests import sensor_reference as SR
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_sensor_v1.npz")
# restatement against the reference's fp32 recordings: each bar is twice the largest deviation make_golden_sensor.py measured over
# the fifteen cases.  Outputs are near 300 K (fp32 sums of (2 hw + 1)^2 terms of unknown order; the largest at factor 926.25 / 90,
# 23 x 23 taps); gradients are of unit-normal cotangents.
MEASURED_MAX = {"down": 2.546e-4, "down_grad": 7.563e-8, "low": 5.135e-4, "low_grad": 1.904e-7}
HOST_BAR = {"down": 5.1e-4, "down_grad": 1.52e-7, "low": 1.03e-3, "low_grad": 3.81e-7}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def restated(name, shape, factor):
    x, d_down, d_low = SR.case_input(name)
    return {"down": SR.downscale_ref(x, factor, SR.DOWN_MTF),
            "down_grad": SR.downscale_bwd_ref(d_down, shape[-2:], factor, SR.DOWN_MTF),
            "low": SR.lowpass_ref(x, factor, SR.LOWPASS_MTF), "low_grad": SR.lowpass_bwd_ref(d_low, factor, SR.LOWPASS_MTF)}


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_every_golden_recording(gold):
    assert list(gold["names"]) == [c[0] for c in SR.CASES] and len(SR.CASES) == 15
    assert SR.FACTORS == [2.0, 2.5, 3.0, 4.0, 926.25 / 90] and SR.SHAPES == [(2, 1, 24, 40), (1, 1, 40, 24), (1, 1, 12, 12)]
    worst = dict.fromkeys(HOST_BAR, 0.0)
    for name, shape, factor, _ in SR.CASES:
        mine = restated(name, shape, factor)
        for k, v in mine.items():
            ref = gold[f"{name}_{k}"]
            assert ref.dtype == np.float32 and ref.shape == v.shape, (name, k)
            worst[k] = max(worst[k], float(np.abs(ref.astype(np.float64) - v).max()))
    for k, bar in HOST_BAR.items():
        print(f"{k}: largest |reference - restatement| {worst[k]:.3e}, bar {bar:.2e}")
        assert 2 * MEASURED_MAX[k] <= bar < 2.1 * MEASURED_MAX[k]
        assert worst[k] <= bar, k
    assert HOST_BAR["down_grad"] < 2e-7 and HOST_BAR["low"] < 2e-3            # the orders the fp32 reference allows


def test_the_regenerated_inputs_are_the_golden_ones(gold):
    for name, shape, factor, _ in SR.CASES:
        x, d_down, d_low = SR.case_input(name)
        assert x.dtype == d_down.dtype == d_low.dtype == np.float32 and x.shape == d_low.shape == shape
        assert d_down.shape == gold[name + "_down"].shape and SR.checksum(x, d_down, d_low) == int(gold[name + "_crc"]), name


def test_adjoint_identity_in_float64():
    rs = np.random.RandomState(5)
    for factor, hkw, crop, shape in ((2.0, None, True, (24, 40)), (2.5, None, True, (40, 24)), (R.COARSE, None, False, (12, 40)),
                                     (R.FINE, None, False, (4, 4)), (1.5, 16, False, (37, 37)), (3.0, None, True, (12, 12))):
        x = rs.standard_normal(shape)
        out = SR.downscale_ref(x, factor, 0.1, hkw, crop)
        d = rs.standard_normal(out.shape)
        a, b = float((out * d).sum()), float((x * SR.downscale_bwd_ref(d, shape, factor, 0.1, hkw, crop)).sum())
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1.0), (factor, a, b)
        d = rs.standard_normal(shape)
        a, b = float((SR.lowpass_ref(x, factor, 0.25, hkw) * d).sum()), float((x * SR.lowpass_bwd_ref(d, factor, 0.25, hkw)).sum())
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1.0), (factor, a, b)


def test_lowpass_operator():
    """rows sum to 1 (a constant stays), the support is [o - hw, o + hw] clipped, and it is get_output_ftm's padding literally"""
    for n, factor, hkw in ((12, R.COARSE, None), (2, 1.5, 1), (17, 3.0, 16), (63, 2.5, None), (5, 4.0, None)):
        hw = R.half_width(factor, hkw)
        Lm = SR.lowpass_operator(n, factor, 0.25, hkw)
        assert np.abs(Lm.sum(axis=1) - 1).max() < 1e-14 and (Lm >= 0).all()
        x = np.random.RandomState(n).standard_normal(n)
        padded = np.pad(x, hw, mode="reflect")
        want = np.convolve(padded, R.taps(factor, 0.25, hkw)[::-1], mode="valid")
        assert np.abs(Lm @ x - want).max() < 1e-13
        o, j = np.nonzero(Lm)
        assert (np.abs(o - j) <= hw).all()
    with pytest.raises(ValueError):
        SR.lowpass_operator(4, 4.0)


def test_the_coordinate_is_the_one_the_table_kernel_forms():
    """sensor_reference.axis_operator differs from degrade_reference.axis_operator only in the fp32 source coordinate -- one rounding,
    as the kernel's fused multiply-add gives it, against one per step --, only at outputs whose product scale * (o + 0.5) lies in
    [2^k, 2^k + 0.5), there by one ulp of the coordinate; the 65-wide axis at 231.656 / 90 has one such output, 12 of 27"""
    assert list(SR.differing_outputs(71, R.FINE, 27)) == [12]
    a, b = SR.axis_operator(65, R.FINE), R.axis_operator(65, R.FINE)
    rows = np.nonzero((a["R"] != b["R"]).any(axis=1))[0]
    assert list(rows) == [12] and 1e-8 < np.abs(a["R"] - b["R"]).max() < 2e-7 and np.array_equal(a["idx"], b["idx"])
    assert R.coords is not SR.coords                                      # the swap inside axis_operator is undone
    total = 0
    for factor in (R.FINE, R.COARSE, 2.0, 2.5, 3.0, 1.25):
        s_one, _, _, _ = SR.coords(0, factor, 16384)
        s_two, _, _, _ = R.coords(0, factor, 16384)
        d = np.nonzero(s_one != s_two)[0]
        total += d.size
        prod = np.float64(np.float32(1.0 / (1.0 / factor))) * (d + 0.5)
        k = np.floor(np.log2(prod))
        assert (prod - 2.0 ** k < 0.5).all() and d.size <= 14, factor     # at most one per binade
        assert (np.abs(s_one[d].astype(np.float64) - s_two[d]) <= np.spacing(s_two[d]).astype(np.float64) * 1.0001).all()
    assert total > 0


def test_longest_run_exceeds_every_window():
    """37 x 37 at factor 1.5 with hkw 16, a case of tests/test_sensor_gpu.py: 34 outputs read one input pixel, K = 36 taps per output"""
    ax = SR.axis_operator(37, 1.5, 0.1, 16, False)
    runs = SR.input_ranges(ax)
    assert int((runs[:, 1] - runs[:, 0] + 1).max()) == 34 and ax["R"].shape == (46, 37)


# ---- 2. what the device's range table rests on ----------------------------------------------------------------------------------
def test_stencils_are_monotone_and_each_pixel_is_read_by_one_run_of_outputs():
    """for every (side, factor, hkw, crop) of the sweep: both ends of the stencil -- the span of non-zero weights, and the span the
    device's table stores, which holds it -- are non-decreasing in the output index, so the outputs over an input pixel are one run"""
    seen, longest = 0, 0
    for factor, hkw in SR.SWEEP:
        hw = R.half_width(factor, hkw)
        for side in list(range(hw + 1, hw + 40)) + [150, 257]:
            for crop in (False, True):
                try:
                    ax = SR.axis_operator(side, factor, 0.1, hkw, crop)
                except ValueError:
                    continue                                          # the crop leaves no output
                seen += 1
                lo, hi = SR.stencils(ax)
                tlo, thi = SR.table_stencils(ax, side)
                for a in (lo, hi, tlo, thi):
                    assert (np.diff(a) >= 0).all(), (side, factor, hkw, crop)
                assert (tlo <= lo).all() and (hi <= thi).all() and (thi - tlo < 2 * hw + 4).all() and tlo.min() >= 0 and thi.max() <= side - 1
                runs = SR.input_ranges(ax)                            # raises where the outputs over a pixel are not one run
                assert runs[:, 0].min() >= 0 and runs[:, 1].max() <= len(lo) - 1
                # the bisection the device does, on the table's stencils, covers the run of the non-zero weights
                first = np.searchsorted(thi, np.arange(side), side="left")
                last = np.searchsorted(tlo, np.arange(side), side="right") - 1
                full = runs[:, 0] <= runs[:, 1]
                assert (first[full] <= runs[full, 0]).all() and (runs[full, 1] <= last[full]).all()
                longest = max(longest, int((last - first + 1).max()))
    print(f"{seen} combinations, longest run {longest} outputs over one pixel")
    assert seen >= 900 and longest > 2 * 16 + 4                       # no small fixed bound: longer than any window K


# ---- 3. the pins of include/sifsr_sensor.h (the gate itself is tests/test_capi_gate.py) ------------------------------------------
NAMES = ["sifsrt_degrade_bwd", "sifsrt_degrade_bwd_workspace_bytes", "sifsrt_lowpass_bwd", "sifsrt_lowpass_fwd",
         "sifsrt_lowpass_workspace_bytes"]
WRITERS = {"sifsrt_degrade_bwd": ["dx", "workspace"], "sifsrt_lowpass_fwd": ["out", "workspace"],
           "sifsrt_lowpass_bwd": ["dx", "workspace"]}
HOST_ONLY = {"sifsrt_degrade_bwd_workspace_bytes", "sifsrt_lowpass_workspace_bytes"}   # no pointer at all: a size on the host


def test_the_row_and_the_declared_names(L):
    assert L.FAMILIES["sensor"] == ("sifsr_sensor.h", "sifsrt_")
    assert L.declared("sensor") == NAMES
    decls = L.parse_header(L.header_path("sensor"))
    assert {n for n in NAMES if decls[n][0] is ctypes.c_size_t} == HOST_ONLY     # every other one returns an int status
    assert not set(NAMES) & L.COUNT_RETURNING


def test_every_writing_entry_point_has_a_contract_case(L):
    T = importlib.import_module("tests.test_sensor_gpu")
    writers = L.writers("sensor")
    assert writers == WRITERS
    assert set(L.declared("sensor")) - set(writers) == HOST_ONLY             # the only entry points without a case
    for name, cases in T.CONTRACT.items():
        assert len(cases) >= 3, name
    # with and without out_valid, crop off and on, more than one image, the smallest shape of each operator
    shapes = T.DEGRADE_CONTRACT_SHAPES
    assert {s[7] for s in shapes} == {False, True} and {s[6] for s in shapes} == {False, True} and any(s[0] > 1 for s in shapes)
    assert (1, 4, 4, R.FINE, 0, False, False, False) in [tuple(s) for s in shapes]
    assert any(h == hw + 1 or w == hw + 1 for _, h, w, _, hw in T.LOWPASS_CONTRACT_SHAPES)
    # the const inputs are declared const: run_contract's arena checks them untouched
    decls = L.parse_header(L.header_path("sensor"))
    for name in writers:
        consts = [a[0] for a in decls[name][1] if a.pointer and a.const]
        assert consts == (["dout", "out_valid"] if name == "sifsrt_degrade_bwd" else ["x"] if name == "sifsrt_lowpass_fwd" else ["dout"])


# ---- 4. the public names ---------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import degrade, sensor
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    got = sig(sensor.downscale)
    assert got[:6] == [("x", E_), ("factor", E_), ("mtf", 0.1), ("hkw", None), ("crop", True), ("valid", None)]
    assert got[6][0] == "fill_value" and math.isnan(got[6][1]) and got[7] == ("return_valid", False) and len(got) == 8
    assert sig(sensor.lowpass) == [("x", E_), ("factor", E_), ("mtf", 0.1), ("hkw", None)]
    assert sig(sensor.lr_shape) == [("H", E_), ("W", E_), ("factor", E_), ("hkw", None)]
    assert [k for k, _ in sig(sensor.sif_loss)] == ["kind", "sr", "lst", "ndvi", "factor", "mean", "std", "alpha", "gamma"]
    assert sig(sensor.train_step) == [("model", E_), ("optimizer", E_), ("lst", E_), ("lst_up", E_), ("ndvi", E_), ("stats", E_), ("alpha", E_),
                                      ("gamma", E_), ("factor", E_), ("kind", "sr2"), ("sync_grads", True), ("return_sr", False)]
    assert sifsr.sensor is sensor and "F.interpolate" in sensor.train_step.__doc__
    # the LR patch shapes at the network's sizes
    assert sensor.lr_shape(192, 192, 3) == (64, 64) and sensor.lr_shape(128, 128, 2) == (64, 64) and sensor.lr_shape(160, 160, 2.5) == (64, 64)
    assert sensor.lr_shape(24, 32, 3) == (8, 10) and sensor.lr_shape(40, 52, 4) == (10, 13)
    for H, W, f, hkw in ((40, 52, 2.5, None), (97, 131, R.COARSE, None), (37, 37, 1.5, 16)):
        assert sensor.lr_shape(H, W, f, hkw) == degrade.output_shape(H, W, f, hkw, crop=True) == (R.out_side(H, f, hkw, True), R.out_side(W, f, hkw, True))
    # what existed before keeps its refusals
    with pytest.raises(NotImplementedError):
        degrade.degrade(torch.zeros((40, 52), requires_grad=True), 2.0)
    with pytest.raises(NotImplementedError):
        sifsr.get_output_ftm(torch.zeros(1, 1, 8, 8), factor=2)
    with pytest.raises(NotImplementedError):
        sifsr.downscale_LST_SR_to_LR(torch.zeros(1, 1, 8, 8), factor=3)


def test_errors_without_a_gpu():
    import sifsr
    from sifsr import sensor
    E = sifsr.SifsrError
    z = torch.zeros((1, 1, 24, 32))
    for bad in (lambda: sensor.downscale(z, 3.0), lambda: sensor.downscale(z.requires_grad_(False)[0, 0], 2.0, crop=False),
                lambda: sensor.lowpass(z, 3.0), lambda: sensor.downscale(np.zeros((24, 32), np.float32), 3.0),
                lambda: sensor.lowpass(z, 3.0, mtf=1.0), lambda: sensor.downscale(z, 3.0, mtf=0.0), lambda: sensor.lowpass(z, 3.0, hkw=17),
                lambda: sensor.lr_shape(24, 32, 1.0), lambda: sensor.lr_shape(3, 32, 3.0), lambda: sensor.lr_shape(24, 32, 16.5),
                lambda: sensor.sif_loss("sr2", z, torch.zeros(1, 1, 8, 10), z, 3.0, 300.0, 10.0, 0.5, 1.0),          # no CPU path
                lambda: sensor.sif_loss("sr3", z, torch.zeros(1, 1, 8, 10), z, 3.0, 300.0, 10.0, 0.5, 1.0),
                lambda: sensor.sif_loss("sr2", z[0], torch.zeros(1, 1, 8, 10), z[0], 3.0, 300.0, 10.0, 0.5, 1.0)):
        with pytest.raises(E):
            bad()
    # lst of another shape than lr_shape: told before anything touches a device
    for lst in (torch.zeros(1, 1, 6, 8), torch.zeros(1, 1, 8, 11), torch.zeros(1, 8, 10), torch.zeros(2, 1, 8, 10)):
        with pytest.raises(E, match=r"lst must be \(1, 1, 8, 10\) at factor 3"):
            sensor.sif_loss("sr2", z, lst, z, 3.0, 300.0, 10.0, 0.5, 1.0)
    with pytest.raises(E, match="sr and ndvi"):
        sensor.sif_loss("sr1", z, torch.zeros(1, 1, 8, 10), torch.zeros(1, 1, 24, 31), 3.0, 300.0, 10.0, 0.5, 1.0)


def test_host_only_entry_points(L):
    """sizes, and every limit of the header: shape, argument and workspace errors are found before anything is launched (the
    pointers below are not memory)"""
    lib = L.lib()
    dsize, lsize = lib.sifsrt_degrade_bwd_workspace_bytes, lib.sifsrt_lowpass_workspace_bytes
    oh, ow = ctypes.c_int(), ctypes.c_int()
    for B, h, w, f, hkw, crop in ((1, 700, 830, R.COARSE, 0, 0), (64, 192, 192, 3.0, 0, 1), (6, 40, 52, 2.0, 3, 0), (1, 4, 4, R.FINE, 0, 0)):
        assert lib.sifsrs_out_shape(h, w, f, hkw, crop, ctypes.byref(oh), ctypes.byref(ow)) == 0
        K = 2 * R.half_width(f, hkw or None) + 4
        # the forward's tables (float64 weights, one int4 per output), one int2 per input index, the (B, oh, w) float64 intermediate
        least = (oh.value + ow.value) * (8 * K + 16) + 8 * (h + w) + 8 * B * oh.value * w
        assert least <= dsize(B, h, w, f, hkw, crop) <= least + 64
        K = 2 * R.half_width(f, hkw or None) + 1
        least = (h + w) * (8 * K + 16) + 8 * (h + w) + 8 * B * h * w
        assert least <= lsize(B, h, w, f, hkw) <= least + 64
    bad = [(11, 40, R.COARSE, 0), (40, 11, R.COARSE, 0), (3, 9, R.FINE, 0), (16385, 40, 2.0, 0), (40, 16385, 2.0, 0), (40, 52, 1.0, 0),
           (40, 52, 0.5, 0), (40, 52, 16.5, 0), (40, 52, float("nan"), 0), (40, 52, float("inf"), 0), (40, 52, 2.0, 17), (40, 52, 2.0, -1),
           (0, 0, 2.0, 0), (-5, 40, 2.0, 0)]
    for h, w, f, hkw in bad:
        assert dsize(1, h, w, f, hkw, 0) == 0 and lsize(1, h, w, f, hkw) == 0, (h, w, f, hkw)
    assert dsize(1, 4, 9, 15.0, 3, 0) == 0 and lsize(1, 4, 9, 15.0, 3) > 0          # no output row at factor 15; the low-pass keeps its size
    assert dsize(1, 40, 52, 2.0, 3, 2) == 0 and dsize(1, 40, 52, 2.0, 3, -1) == 0
    for fn, extra in ((dsize, (0,)), (lsize, ())):
        assert fn(0, 40, 52, 2.0, 0, *extra) == 0 and fn(65536, 40, 52, 2.0, 0, *extra) == 0 and fn(65535, 40, 52, 2.0, 0, *extra) > 0
    assert lsize(1, 2, 2, 1.5, 1) > 0 and lsize(1, 17, 17, 3.7, 16) > 0 and lsize(1, 16, 17, 3.7, 16) == 0
    one = ctypes.c_void_p(4096)
    limits = (dict(h=3), dict(w=3), dict(h=16385), dict(w=16385), dict(factor=1.0), dict(factor=16.5), dict(factor=float("nan")),
              dict(hkw=17), dict(hkw=-1), dict(factor=16.5, hkw=2), dict(mtf=0.0), dict(mtf=1.0), dict(mtf=-0.1), dict(mtf=float("nan")),
              dict(B=0), dict(B=65536))
    # sifsrt_degrade_bwd
    fn = lib.sifsrt_degrade_bwd
    args = lambda **kw: [kw.get("dout", one), kw.get("out_valid", one), kw.get("dx", one), kw.get("ws", one), kw.get("nbytes", 1 << 40),
                         kw.get("B", 2), kw.get("h", 40), kw.get("w", 52), kw.get("factor", 2.0), kw.get("mtf", 0.1), kw.get("hkw", 3),
                         kw.get("crop", 0), None]
    for b in limits + (dict(crop=2), dict(h=4, w=9, factor=15.0)):
        assert fn(*args(**b)) == 1001, b
    for b in (dict(dout=None), dict(dx=None), dict(ws=None), dict(ws=ctypes.c_void_p(4104)), dict(dout=ctypes.c_void_p(4098)),
              dict(dx=ctypes.c_void_p(4097))):
        assert fn(*args(**b)) == 1002, b
    need = dsize(2, 40, 52, 2.0, 3, 0)
    assert fn(*args(nbytes=need - 1)) == 1003 and fn(*args(nbytes=0)) == 1003 and fn(*args(nbytes=need - 1, out_valid=None)) == 1003
    assert fn(*args(nbytes=dsize(1, 40, 52, 2.0, 3, 0))) == 1003
    # sifsrt_lowpass_fwd / _bwd
    for fn in (lib.sifsrt_lowpass_fwd, lib.sifsrt_lowpass_bwd):
        args = lambda **kw: [kw.get("x", one), kw.get("out", one), kw.get("ws", one), kw.get("nbytes", 1 << 40), kw.get("B", 2), kw.get("h", 40),
                             kw.get("w", 52), kw.get("factor", 2.0), kw.get("mtf", 0.25), kw.get("hkw", 3), None]
        for b in limits:
            assert fn(*args(**b)) == 1001, b
        for b in (dict(x=None), dict(out=None), dict(ws=None), dict(ws=ctypes.c_void_p(4104)), dict(x=ctypes.c_void_p(4098)),
                  dict(out=ctypes.c_void_p(4097))):
            assert fn(*args(**b)) == 1002, b
        need = lsize(2, 40, 52, 2.0, 3)
        assert fn(*args(nbytes=need - 1)) == 1003 and fn(*args(nbytes=0)) == 1003 and fn(*args(nbytes=lsize(1, 40, 52, 2.0, 3))) == 1003
