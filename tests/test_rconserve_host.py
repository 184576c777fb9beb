"""CPU: conservation of the observed LST at any ratio -- what can be held without a GPU.

  * the restatement tests/rconserve_reference.py against the restatements it is made of: its D with everything valid is
    degrade_ref(crop=True) exactly, its U is torch's float64 F.interpolate to 1e-12, its cells are the floor(Y h / H) rule of
    tests/ratio_reference.py, and at x4 its counted cells are those of tests/conserve_reference.py,
  * the facts the header states: which outputs touch the zero ring at each ratio, how many cells a stencil reaches, that a stencil
    holds its own cell, and that the planted gaps give 0 < counted < valid < all,
  * convergence, on the CPU: the RMSE falls with every one of three steps at x2, x2.5, x8/3, x3 and x4,
  * the tile of csrc/rconserve.hip: the staged span fits its LDS array for every ratio and side tried,
  * the pins of include/sifsr_rconserve.h (the gate itself is tests/test_capi_gate.py): the row, the literal name and writer lists,
    the contract cases, the workspace size and the refusals through the host-only paths,
  * the public names and signatures, those of ratio.predict_granule* unchanged included."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conserve_reference as R
from tests import degrade_reference as DR
from tests import ratio_reference as RR
from tests import rconserve_reference as Q
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{s[0]}x{s[1]}at{p}:{q}" for s, (p, q) in Q.SHAPES]


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(Q.SHAPES)), ids=IDS)
def test_d_and_u_are_the_pinned_operators(idx):
    shape, (p, q) = Q.SHAPES[idx]
    H, W = Q.hr_shape(shape, p, q)
    assert Q.accepted(shape, (H, W))
    sr, lst = Q.make_case(shape, (p, q), seed=idx)
    want, ov = DR.degrade_ref(sr, float(H) / float(shape[0]), 0.1, None, True)
    assert want.shape == shape and np.array_equal(Q.D(sr, shape), want)
    # everything valid: counted is degrade_ref's out_valid, which holds the ring alone
    assert np.array_equal(Q.counted(np.ones(shape, bool), (H, W)), ov)
    r = np.random.RandomState(idx).standard_normal(shape)
    ref = F.interpolate(torch.from_numpy(r)[None, None], size=(H, W), mode="bicubic", align_corners=False)[0, 0].numpy()
    assert np.abs(Q.U(r, (H, W)) - ref).max() <= 1e-12
    assert np.array_equal(Q.cells(shape[0], H), RR.cell_of(H, p, q)) and np.array_equal(Q.cells(shape[1], W), RR.cell_of(W, p, q))
    assert np.array_equal(Q.up(np.arange(shape[0] * shape[1]).reshape(shape) % 2, (H, W)) != 0,
                          RR.upsampled(np.arange(shape[0] * shape[1]).reshape(shape) % 2, p, q))


@pytest.mark.parametrize("idx", range(len(Q.SHAPES)), ids=IDS)
def test_validity_on_cells_is_the_sensor_model_s_on_pixels(idx):
    """holes planted cell by cell: counted is sifsrs_degrade(valid=)'s out_valid for the pixel mask up(c)"""
    shape, (p, q) = Q.SHAPES[idx]
    H, W = Q.hr_shape(shape, p, q)
    rs = np.random.RandomState(idx)
    c = rs.uniform(size=shape) > 0.1
    _, ov = DR.degrade_ref(np.ones((H, W)), float(H) / float(shape[0]), 0.1, None, True, valid=Q.up(c, (H, W)))
    assert np.array_equal(Q.counted(c, (H, W)), ov & c)


def test_ring_and_reach_per_ratio():
    """the facts include/sifsr_rconserve.h states, read from the operator: nothing is hard-wired in the kernels"""
    want = {(3, 1): ([], 3), (4, 1): ([], 3), (2, 1): ([0, 11], 5), (5, 2): ([0], 5), (8, 3): ([0], 5)}
    for (p, q), (ring, reach) in want.items():
        a = Q.axis(12, 12 * p // q)
        assert np.flatnonzero(a["ring"]).tolist() == ring and int(a["touch"].sum(axis=1).max()) == reach, (p, q)
        assert a["own_in_stencil"].all()
        sizes = np.bincount(Q.cells(12, 12 * p // q))
        assert set(sizes.tolist()) == {p // q, -(-p // q)} and sizes.sum() == 12 * p // q
    # at x4 the stencil is the 3 x 3 neighbourhood clipped to the raster, as in include/sifsr_conserve.h
    a = Q.axis(12, 48)
    assert np.array_equal(a["lo"], np.maximum(4 * np.arange(12) - 4, 0)) and np.array_equal(a["hi"], np.minimum(4 * np.arange(12) + 7, 47))
    # every shape of the GPU tests: the own cell lies inside the stencil
    for shape, (p, q) in Q.SHAPES:
        H, W = Q.hr_shape(shape, p, q)
        assert Q.axis(shape[0], H)["own_in_stencil"].all() and Q.axis(shape[1], W)["own_in_stencil"].all()


@pytest.mark.parametrize("kind", R.HOLES)
def test_counted_at_x4_is_f12_s(kind):
    sr, lst, mask = R.hole_case(kind)
    c = Q.cell_valid(sr, lst, mask)
    assert np.array_equal(c, R.cell_valid(sr, lst, mask)) and np.array_equal(Q.up(c, sr.shape), R.up(c))
    assert np.array_equal(Q.counted(c, sr.shape), R.counted(c))
    # and the values: f12's D has fp32 taps and no ring, this one float64 taps; they are the same sensor
    r_q, r_f = Q.residual(sr, lst, mask)[0], R.residual(sr, lst, mask, R.taps32())[0]
    assert np.abs(r_q - r_f).max() < 1e-4


@pytest.mark.parametrize("pq", Q.RATIOS, ids=lambda r: f"{r[0]}:{r[1]}")
def test_holes_and_convergence_in_the_restatement(pq):
    for kind in Q.HOLES:
        sr, lst, mask = Q.hole_case(kind, pq)
        want = Q.conserve_ref(sr, lst, mask, n_iter=2)
        c, n = want[3], want[4]
        if kind in ("checkerboard", "nothing_valid"):
            assert not n.any() and np.isnan(want[1][:, 1:]).all() and np.array_equal(want[0], sr.astype(np.float64), equal_nan=True)
        else:
            assert 0 < n.sum() < c.sum() < c.size, (kind, int(n.sum()), int(c.sum()))
        m = Q.up(c, sr.shape)
        for junk in (np.nan, 0.0, np.inf, 1e30):
            if junk == 1e30 and mask is None and kind != "sr_nan":
                continue
            psr, plst = Q.poisoned(sr, lst, mask, junk)
            got = Q.conserve_ref(psr, plst, mask, n_iter=2)
            assert np.array_equal(got[0][m], want[0][m]) and np.array_equal(got[1], want[1], equal_nan=True)
            assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], c) and np.array_equal(got[4], n)
    shape = (12, 15) if pq == (8, 3) else (12, 16)
    sr, lst = Q.make_case(shape, pq, seed=5, noise=0.5)
    rows = Q.conserve_ref(sr, lst, None, n_iter=3)[1]
    print(pq, "counted", int(rows[0, 0]), "RMSE", rows[:, 2].tolist(), "bias", rows[:, 1].tolist())
    assert np.all(np.diff(rows[:, 2]) < 0) and np.all(rows[:, 0] == rows[0, 0]) and rows[0, 0] > 0
    # a constant raster under a constant observation leaves no residual off the ring
    one = np.full(Q.hr_shape(shape, *pq), 301.25, np.float32)
    r, n, _ = Q.residual(one, np.full(shape, 301.25, np.float32))
    assert n.any() and np.abs(r).max() < 1e-10


def test_the_staged_span_fits_the_tile():
    """csrc/rconserve.hip stages whole cells, from the first a stencil of the tile touches to the last, into CAP x CAP floats"""
    assert [Q.tile_side(f) for f in (2.0, 2.5, 8 / 3, 3.0, 4.0, 5.0, 8.0)] == [16, 16, 16, 16, 16, 12, 6]
    worst = 0
    for p, q in Q.RATIOS + [(8, 1), (5, 1), (6, 1), (7, 1), (3, 2), (7, 2), (7, 3), (11, 4), (16, 3), (15, 2), (23, 3)]:
        for n in list(range(q, 36 * q + 1, q)) + [128 * q, 131 * q]:
            N = n * p // q
            if Q.accepted((n, n), (N, N)):
                worst = max(worst, Q.staged_span(n, N))
    print("most staged pixels of an axis:", worst)
    assert 64 <= worst <= Q.CAP


# ---- 2. the pins of include/sifsr_rconserve.h (the gate itself is tests/test_capi_gate.py) ---------------------------------------
def test_the_row_and_the_contract_cases(L):
    from tests import test_rconserve_gpu as T
    assert L.FAMILIES["rconserve"] == ("sifsr_rconserve.h", "sifsrc_") and list(L.FAMILIES)[16] == "rconserve"
    names, writers = L.declared("rconserve"), L.writers("rconserve")
    assert names == ["sifsrc_conserve", "sifsrc_workspace_bytes"]
    assert writers == {"sifsrc_conserve": ["out", "stats", "workspace"]}
    assert sorted(T.CONTRACT) == sorted(writers) and len(T.CONTRACT["sifsrc_conserve"]) == len(T.CONTRACT_SHAPES) >= 4
    # with and without a mask, in place and not, the pure check, a ragged raster of several tiles
    assert {(s[2], s[3]) for s in T.CONTRACT_SHAPES} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(s[1] == 0 for s in T.CONTRACT_SHAPES) and any(s[1] >= 2 for s in T.CONTRACT_SHAPES)
    tiles = lambda s: [-(-n // Q.tile_side(Q.SHAPES[s[0]][1][0] / Q.SHAPES[s[0]][1][1])) for n in Q.SHAPES[s[0]][0]]
    assert any(min(tiles(s)) >= 2 and all(n % 16 for n in Q.SHAPES[s[0]][0]) for s in T.CONTRACT_SHAPES)
    assert L.call("sifsr_abi_version") == 3


def test_host_only_entry_points(L):
    """the workspace size; shape, argument and workspace errors are found before anything is launched (none needs a GPU)"""
    size = lambda *a: L.call("sifsrc_workspace_bytes", *a)
    for shape, (p, q) in Q.SHAPES + [((1200, 1200), (3, 1)), ((1200, 1200), (5, 2))]:
        (h, w), (H, W) = shape, Q.hr_shape(shape, p, q)
        tl = Q.tile_side(float(H) / float(h))
        K = 2 * DR.half_width(float(H) / float(h)) + 4
        for n in (0, 1, 64):
            need = size(h, w, H, W, n)
            # r (fp32), the two weight tables and the two stencil tables, four float64 partials per workgroup and row, one byte per cell
            floor = 4 * h * w + 8 * K * (h + w) + 16 * (h + w) + 32 * (n + 1) * -(-h // tl) * -(-w // tl) + h * w
            assert floor <= need <= floor + 7 * 16, (shape, n)
        assert size(h, w, H, W, 65) == 0 and size(h, w, H, W, -1) == 0
    for h, w, H, W in ((16, 20, 20, 25), (12, 16, 36, 49), (12, 16, 36, 47), (12, 16, 12, 16), (12, 16, 108, 144), (1, 1, 3, 3), (0, 0, 0, 0),
                       (-1, 4, -3, 12), (12, 16, 24, 48), (8192, 8192, 24576, 24576)):
        assert size(h, w, H, W, 1) == 0 and not Q.accepted((h, w), (H, W)), (h, w, H, W)
    one = ctypes.c_void_p(4096)
    fn = L.lib().sifsrc_conserve
    args = lambda **kw: [kw.get("sr", one), kw.get("lst", one), kw.get("mask", one), kw.get("out", one), kw.get("stats", one),
                         kw.get("ws", one), kw.get("nbytes", 1 << 40), kw.get("h", 12), kw.get("w", 16), kw.get("H", 30), kw.get("W", 40),
                         kw.get("mtf", 0.1), kw.get("relax", 1.0), kw.get("n_iter", 1), None]
    for bad in (dict(h=11), dict(w=15), dict(H=31), dict(h=0), dict(h=16, w=20, H=20, W=25), dict(H=12, W=16), dict(H=108, W=144),
                dict(n_iter=-1), dict(n_iter=65), dict(mtf=0.0), dict(mtf=1.0), dict(mtf=float("nan"))):
        assert fn(*args(**bad)) == 1001, bad
    for bad in (dict(sr=None), dict(lst=None), dict(out=None), dict(stats=None), dict(ws=None), dict(ws=ctypes.c_void_p(4104)),
                dict(sr=ctypes.c_void_p(4098)), dict(out=ctypes.c_void_p(4097)), dict(stats=ctypes.c_void_p(4100)),
                dict(relax=float("nan")), dict(relax=float("-inf"))):
        assert fn(*args(**bad)) == 1002, bad
    need = size(12, 16, 30, 40, 1)
    assert fn(*args(nbytes=need - 1)) == 1003 and fn(*args(nbytes=0)) == 1003 and fn(*args(nbytes=need - 1, mask=None)) == 1003
    assert fn(*args(nbytes=size(12, 16, 30, 40, 0), n_iter=1)) == 1003


# ---- 3. the public names ---------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import conserve, ratio, rconserve
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    assert sig(rconserve.consistency) == sig(conserve.consistency) == [("sr", E_), ("lst", E_), ("mask", None), ("mtf", 0.1),
                                                                       ("return_residual", False)]
    assert sig(rconserve.conserve) == sig(conserve.conserve) == [("sr", E_), ("lst", E_), ("mask", None), ("n_iter", 1), ("relax", 1.0),
                                                                 ("mtf", 0.1), ("out", None), ("return_stats", False)]
    # the two granule calls at a ratio: the option is keyword-only, off by default and added around the call; the parameter lists
    # tests/test_ratio_host.py pins are what they were
    assert sig(ratio.predict_granule) == [("model", E_), ("lst_g", E_), ("ndvi_g", E_), ("stats", E_), ("window", 64), ("hr", 192),
                                          ("batch", 256), ("overlap", 0), ("cover_edges", False)]
    got = sig(ratio.predict_granule_gaps)
    assert [k for k, _ in got] == ["model", "lst_g", "ndvi_g", "stats", "mask", "window", "hr", "batch", "overlap", "cover_edges", "fill_value",
                                   "return_info"] and math.isnan(got[10][1]) and got[11] == ("return_info", False)
    for f in (ratio.predict_granule, ratio.predict_granule_gaps):
        outer = inspect.signature(f, follow_wrapped=False).parameters
        assert outer["conserve"].kind is inspect.Parameter.KEYWORD_ONLY and outer["conserve"].default == 0
        assert "conserve=k" in f.__doc__ and "rconserve" in f.__doc__
        with pytest.raises(sifsr.SifsrError):                                  # refused before anything runs
            f(None, None, None, None, conserve=-1)
    # the x4 calls keep their step: conserve.granule_option's default
    assert sig(conserve.granule_option) == [("fn", E_), ("correct", None)]
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        rconserve.consistency(torch.zeros((36, 48)), torch.zeros((12, 16)))
    with pytest.raises(sifsr.SifsrError):
        rconserve.conserve(torch.zeros((36, 48)), torch.zeros((12, 16)))
    assert os.path.samefile(sifsr._lib.header_path("rconserve"), os.path.join(ROOT, "include", "sifsr_rconserve.h"))
    assert sifsr.rconserve is rconserve and rconserve.MAX_ITER == 64 and rconserve.MAX_FACTOR == Q.MAX_FACTOR == 8.0
    for text in (ratio.__doc__, sifsr.rloss.__doc__):
        assert "rconserve" in text and "``conserve=`` at a ratio" not in text
