"""CPU: whole-granule prediction at any ratio -- what can be held without a GPU.

  * the restatement tests/ratio_reference.py: its integer-phase resampler IS torch's float64 bicubic ``F.interpolate`` (to 1e-12),
  * ``sifsrr_geometry`` (host only) against the restatement over a sweep that holds every rule's first violation; the tile origins
    are ``sifsrx_tile_origin``'s, mapped to whole HR pixels, and at hr = 4 win the counts are ``sifsrx_tile_count``'s,
  * the pins of include/sifsr_ratio.h for the ``sifsrr_`` entry points (the gate itself is tests/test_capi_gate.py, which also holds
    the exemption of ``sifsrr_geometry``): the row, the declared names, the writers, and what the memory-contract cases of
    tests/test_ratio_gpu.py cover,
  * the public names of ``sifsr.ratio`` and the refusals that need no GPU."""
import ctypes
import importlib
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ratio_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

SHAPE_ERR, ARG_ERR = 1001, 1002
# (h, w) -> (H, W): the network's ratios at the tile sizes of the GPU tests and of training, a non-integer one per axis, a 1-pixel
# raster (every index clamps) and a mixed case with a ratio of its own per axis
UPSAMPLE_SHAPES = [((8, 8), (24, 24)), ((16, 16), (40, 40)), ((12, 12), (32, 32)), ((64, 64), (160, 160)), ((64, 64), (192, 192)),
                   ((64, 64), (256, 256)), ((5, 5), (8, 8)), ((1, 1), (8, 8)), ((7, 64), (24, 256))]


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------
def test_restated_upsample_is_torch_float64_bicubic():
    worst = 0.0
    for k, ((h, w), (H, W)) in enumerate(UPSAMPLE_SHAPES):
        x = np.random.RandomState(k).standard_normal((2, h, w))
        want = F.interpolate(torch.from_numpy(x)[:, None], size=(H, W), mode="bicubic", align_corners=False)[:, 0].numpy()
        got = R.upsample_ref(x, (H, W))
        assert got.shape == want.shape == (2, H, W) and got.dtype == np.float64
        dev = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
        print(f"{(h, w)} -> {(H, W)}: |restatement - torch float64| = {dev:.2e}")
        worst = max(worst, dev)
    assert worst <= 1e-12


def test_phase_is_exact_and_an_equal_axis_is_the_identity():
    for n, N in ((8, 24), (16, 40), (12, 32), (5, 8), (1, 8), (64, 160), (7, 7)):
        i, r, den = R.phases(n, N)
        assert den == 2 * N and (0 <= r).all() and (r < den).all() and i.min() >= -1 and i.max() <= n - 1
        assert ((2 * np.arange(N) + 1) * n - N == i * den + r).all()
        assert (np.diff(i) >= 0).all() and (np.diff(i) <= 1).all()         # the source row advances by 0 or 1 per output row
        assert np.abs(R.axis_matrix(n, N).sum(axis=1) - 1).max() < 1e-14      # a constant stays
    assert np.array_equal(R.axis_matrix(7, 7), np.eye(7))
    # p / q = 5 / 2: HR pixels 2 and 3 straddle cells 0 and 1
    assert list(R.cell_of(10, 5, 2)) == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3]


# ---- 2. the geometry ----------------------------------------------------------------------------------------------------------------
def lib_geometry(L, h, w, win, hr, overlap, cover):
    out6 = (ctypes.c_int * 6)(*([-7] * 6))
    rc = L.lib().sifsrr_geometry(h, w, win, hr, overlap, cover, out6)
    if rc != 0:
        assert rc == SHAPE_ERR and list(out6) == [-7] * 6                 # untouched
        return None
    p, q, ty, tx, H, W = out6
    return p, q, (ty, tx), (H, W)


# the first violation of every rule, and its neighbour that is accepted: (h, w, win, hr, overlap, cover)
FIRST_VIOLATIONS = [
    ((33, 32, 16, 40, 0, 0), (32, 32, 16, 40, 0, 0)),      # n % q != 0 (q = 2)
    ((32, 33, 16, 40, 0, 0), (32, 34, 16, 40, 0, 0)),
    ((32, 32, 16, 40, 1, 0), (32, 32, 16, 40, 2, 0)),      # overlap % q != 0
    ((20, 26, 8, 28, 0, 0), (20, 26, 8, 32, 0, 0)),        # hr % 8 != 0
    ((20, 26, 8, 16, 0, 0), (20, 26, 8, 24, 0, 0)),        # hr = 16 < 24
    ((48, 48, 24, 24, 0, 0), (46, 46, 23, 24, 0, 0)),      # hr = win
    ((40, 40, 32, 24, 0, 0), (40, 40, 16, 24, 0, 0)),      # hr < win
    ((20, 26, 2, 40, 0, 0), (20, 26, 2, 32, 0, 0)),        # hr > 16 win
    ((70, 70, 32, 264, 0, 0), (70, 70, 32, 256, 0, 0)),    # hr > 256
    ((130, 130, 65, 256, 0, 0), (130, 130, 64, 256, 0, 0)),  # win > 64
    ((20, 26, 0, 24, 0, 0), (20, 26, 2, 24, 0, 0)),        # win < 1
    ((20, 26, 8, 24, 5, 1), (20, 26, 8, 24, 4, 1)),        # 2 overlap > win
    ((20, 26, 8, 24, -1, 1), (20, 26, 8, 24, 0, 1)),       # overlap < 0
    ((7, 26, 8, 24, 0, 1), (8, 26, 8, 24, 0, 1)),          # n < win
    ((20, 7, 8, 24, 0, 1), (20, 8, 8, 24, 0, 1)),
    ((16385, 8, 8, 24, 0, 0), (16384, 8, 8, 24, 0, 0)),    # the largest raster
]


def test_geometry_is_the_restatement(L):
    for bad, good in FIRST_VIOLATIONS:
        assert R.geometry_ref(bad[:2], *bad[2:]) is None and lib_geometry(L, *bad) is None, bad
        want = R.geometry_ref(good[:2], *good[2:])
        assert want is not None and lib_geometry(L, *good) == want, good
    seen = refused = 0
    for win, hr in ((8, 24), (16, 40), (12, 32), (8, 32), (64, 192), (64, 160), (64, 128), (64, 256), (6, 40), (3, 48), (24, 40), (64, 72),
                    (5, 24), (16, 16), (16, 20), (65, 256), (8, 136), (1, 8), (2, 24)):
        for n in (win - 1, win, win + 1, win + 2, 2 * win, 2 * win + 3, 20, 26, 37, 48, 150):
            for overlap in (0, 1, 2, 3, 4, 6, 8, win // 2, win // 2 + 1, 16, 32):
                for cover in (0, 1):
                    for h, w in ((n, n), (n, 2 * win + 8), (3 * win, n)):
                        want = R.geometry_ref((h, w), win, hr, overlap, cover)
                        assert lib_geometry(L, h, w, win, hr, overlap, cover) == want, (h, w, win, hr, overlap, cover)
                        seen += 1
                        refused += want is None
    print(f"{seen} geometries, {refused} refused")
    assert seen > 10000 and refused > 1000 and seen - refused > 1000
    assert L.lib().sifsrr_geometry(20, 26, 8, 24, 0, 0, None) == ARG_ERR
    assert lib_geometry(L, 20, 26, 8, 24, 2, 1) == (3, 1, (3, 4), (60, 78))
    assert lib_geometry(L, 32, 48, 16, 40, 2, 0) == (5, 2, (2, 3), (80, 120))
    assert lib_geometry(L, 1200, 1200, 64, 192, 16, 1) == (3, 1, (25, 25), (3600, 3600))


def test_origins_are_the_mosaic_s_and_whole_hr_pixels(L):
    lib = L.lib()
    for n, win, hr, overlap, cover in ((20, 8, 24, 2, 1), (26, 8, 24, 4, 0), (32, 16, 40, 2, 1), (48, 16, 40, 8, 1), (46, 16, 40, 2, 1),
                                       (27, 12, 32, 3, 1), (36, 12, 32, 6, 0), (150, 64, 160, 16, 1), (1200, 64, 192, 16, 1), (26, 8, 32, 2, 1)):
        p, q, (ty, _), (H, _) = R.geometry_ref((n, n), win, hr, overlap, cover)
        o = R.origins(n, win, overlap, cover)
        assert ty == len(o) == lib.sifsrx_tile_count(n, win, overlap, cover)
        assert o == [lib.sifsrx_tile_origin(k, n, win, overlap, cover) for k in range(ty)]
        assert all(v * p % q == 0 for v in o) and overlap * p % q == 0 and o[-1] * p // q + hr <= H
        if cover:
            assert o[-1] * p // q + hr == H
    # an odd stride: win 16, hr 40, overlap 2 -> HR stride 35
    assert [v * 5 // 2 for v in R.origins(46, 16, 2, 1)] == [0, 35, 70, 75]
    # at hr = 4 win the counts are the x4 layout's
    for h, w, win, overlap, cover in ((37, 50, 16, 0, 0), (45, 61, 16, 8, 1), (150, 100, 64, 32, 1), (200, 136, 64, 16, 1)):
        _, _, (ty, tx), hr_shape = lib_geometry(L, h, w, win, 4 * win, overlap, cover)
        assert (ty, tx) == (lib.sifsrx_tile_count(h, win, overlap, cover), lib.sifsrx_tile_count(w, win, overlap, cover))
        assert hr_shape == (4 * h, 4 * w)


# ---- 3. the pins of include/sifsr_ratio.h (the gate itself is tests/test_capi_gate.py) -------------------------------------------
NAMES = ["sifsrr_geometry", "sifsrr_tiles_blend", "sifsrr_tiles_prepare", "sifsrr_upsample"]
WRITERS = {"sifsrr_geometry": ["out6"], "sifsrr_upsample": ["out"], "sifsrr_tiles_prepare": ["x"], "sifsrr_tiles_blend": ["out"]}


def test_the_row_and_the_declared_names(L):
    assert L.FAMILIES["ratio"] == ("sifsr_ratio.h", "sifsrr_")
    assert L.declared("ratio") == NAMES
    decls = L.parse_header(L.header_path("ratio"))
    assert all(decls[n][0] is ctypes.c_int for n in NAMES)                  # every one returns a status; none a size
    assert not set(NAMES) & L.COUNT_RETURNING and len(L.COUNT_RETURNING) == 14


def test_every_writing_entry_point_has_contract_cases(L):
    T = importlib.import_module("tests.test_ratio_gpu")
    writers = L.writers("ratio")
    assert writers == WRITERS
    assert set(L.declared("ratio")) - set(writers) == set()                 # every entry point of the family takes a pointer it may write
    for name, cases in T.CONTRACT.items():
        assert len(cases) >= 3, name
    # the const inputs are declared const: run_contract's arena checks them untouched
    decls = L.parse_header(L.header_path("ratio"))
    consts = {n: [a[0] for a in decls[n][1] if a.pointer and a.const] for n in WRITERS}
    assert consts == {"sifsrr_geometry": [], "sifsrr_upsample": ["x"], "sifsrr_tiles_prepare": ["lst", "ndvi", "active", "n_active"],
                      "sifsrr_tiles_blend": ["sr", "slot", "valid"]}
    # what the cases hold
    assert {(1, 1, 1, 8, 8), (1, 2, 3, 7, 5)} <= set(T.UPSAMPLE_CONTRACT) and any(c[0] > 1 for c in T.UPSAMPLE_CONTRACT)
    assert {c[:2] for c in T.PREPARE_CONTRACT} >= {(8, 24), (16, 40), (12, 32)}
    modes = {c[6] for c in T.PREPARE_CONTRACT}
    assert {"all", "cap>n", "cap<n"} <= modes
    assert {c[4] for c in T.BLEND_CONTRACT} == {0, 1} and {c[5] for c in T.BLEND_CONTRACT} == {False, True}
    assert any(c[3] == 0 for c in T.BLEND_CONTRACT) and any(c[3] > 0 for c in T.BLEND_CONTRACT)
    assert any(c[2] == (16, 40) and c[3] == 2 for c in T.BLEND_CONTRACT)                                   # the odd stride (HR 35)
    for h, w, (win, hr), ov, cover, _ in T.BLEND_CONTRACT:
        assert R.geometry_ref((h, w), win, hr, ov, cover) is not None
    # a flush tile that overlaps its neighbour by more than `overlap`
    assert any(cover and (lambda o: len(o) > 1 and o[-2] + win - o[-1] > ov)(R.origins(h, win, ov, 1)) for h, w, (win, hr), ov, cover, _ in T.BLEND_CONTRACT)


# ---- 4. the public names and the refusals that need no GPU -------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import ratio
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    assert sifsr.ratio is ratio
    assert sig(ratio.upsample) == [("x", E_), ("size", E_)] and "sensor.train_step" in ratio.upsample.__doc__
    assert "ratio.upsample(lst, (H, W))" in ratio.upsample.__doc__
    assert sig(ratio.geometry) == [("lst_shape", E_), ("window", E_), ("hr", E_), ("overlap", 0), ("cover_edges", False)]
    assert sig(ratio.prepare_tiles) == [("lst", E_), ("ndvi", E_), ("stats", None), ("clip_ndvi", False)]
    assert sig(ratio.granule_to_tiles) == [("lst_g", E_), ("ndvi_g", E_), ("stats", E_), ("window", E_), ("hr", E_), ("clip_ndvi", True),
                                           ("overlap", 0), ("cover_edges", False), ("out", None)]
    assert sig(ratio.blend_tiles) == [("sr", E_), ("lst_shape", E_), ("window", E_), ("hr", E_), ("stats", E_), ("overlap", 0),
                                      ("cover_edges", False), ("out", None)]
    assert sig(ratio.predict_granule) == [("model", E_), ("lst_g", E_), ("ndvi_g", E_), ("stats", E_), ("window", 64), ("hr", 192),
                                          ("batch", 256), ("overlap", 0), ("cover_edges", False)]
    got = sig(ratio.predict_granule_gaps)
    assert got[:10] == [("model", E_), ("lst_g", E_), ("ndvi_g", E_), ("stats", E_), ("mask", None), ("window", 64), ("hr", 192),
                        ("batch", 256), ("overlap", 16), ("cover_edges", True)]
    assert got[10][0] == "fill_value" and math.isnan(got[10][1]) and got[11] == ("return_info", False) and len(got) == 12
    g = ratio.geometry((20, 26), 8, 24, overlap=2, cover_edges=True)
    assert g == (3, 1, (3, 4), (60, 78)) and (g.p, g.q, g.tiles, g.hr_shape) == tuple(g)
    assert ratio.geometry((1200, 1200), 64, 160, 16, True) == (5, 2, (25, 25), (3000, 3000))
    # sensor.py is not edited: its docstring still names torch's kernel
    assert "F.interpolate" in sifsr.sensor.train_step.__doc__


def test_refusals_without_a_gpu():
    import sifsr
    from sifsr import ratio
    E = sifsr.SifsrError
    for bad, _ in FIRST_VIOLATIONS:
        with pytest.raises(E, match="no tile layout"):
            ratio.geometry(bad[:2], bad[2], bad[3], bad[4], bool(bad[5]))
    with pytest.raises(E):
        ratio.geometry((20,), 8, 24)
    with pytest.raises(E):
        ratio.geometry((20, 26), "a", 24)
    stats = {"mean_lst": 300.0, "std_lst": 5.0, "mean_ndvi": 0.5, "std_ndvi": 0.2}
    lst, ndvi, sr = torch.zeros((16, 24)), torch.zeros((48, 72)), torch.zeros((6, 1, 24, 24))

    class NoForward(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("a forward ran")
    calls = [lambda: ratio.upsample(lst, (48, 72)), lambda: ratio.upsample(lst.numpy(), (48, 72)), lambda: ratio.upsample(lst.double(), (48, 72)),
             lambda: ratio.prepare_tiles(torch.zeros((2, 1, 8, 8)), torch.zeros((2, 1, 24, 24))),
             lambda: ratio.granule_to_tiles(lst, ndvi, stats, 8, 24), lambda: ratio.blend_tiles(sr, (16, 24), 8, 24, stats),
             lambda: ratio.predict_granule(NoForward(), lst, ndvi, stats, window=8, hr=24),
             lambda: ratio.predict_granule_gaps(NoForward(), lst, ndvi, stats, window=8, hr=24, overlap=2)]
    for bad in calls:                                                     # CPU tensors: there is no CPU path
        with pytest.raises(E):
            bad()
