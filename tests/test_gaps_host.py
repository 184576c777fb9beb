"""CPU: gap-aware whole-granule prediction -- what can be held without a GPU.

  * the NumPy restatement tests/gaps_reference.py checks itself: the pyramid recurrence and the closed form of the fill agree bit
    for bit on every raster of the GPU tests, with and without a mask, and the planted gaps reach the code paths they are meant to,
  * select_ref over the layout sweep of tests/test_mosaic_host.py on random masks: `active` sorted, `slot` and `active` inverse to
    each other, every tile that covers a valid pixel active,
  * the pins of include/sifsr_gaps.h for the `sifsrg_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, every entry point that can write through a pointer has a memory-contract case in tests/test_gaps_gpu.py."""
import numpy as np
import pytest

from tests import gaps_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)
from tests.test_mosaic_gpu import origins
from tests.test_mosaic_host import _sweep

RASTERS = R.make_rasters()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the restatement against itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("name", sorted(RASTERS))
def test_the_two_forms_of_the_fill_agree(name, with_mask):
    lst, mask = RASTERS[name]
    mask = mask if with_mask else None
    filled, valid, level = R.fill_ref(lst, mask, return_level=True)
    closed, valid_c = R.fill_ref_closed(lst, mask)
    assert filled.dtype == closed.dtype == np.float32 and valid.dtype == np.uint8
    assert np.array_equal(valid, valid_c) and np.array_equal(bits(filled), bits(closed))
    ok = valid != 0
    assert np.array_equal(bits(filled[ok]), bits(lst[ok])) and np.isfinite(filled).all()
    assert set(np.unique(valid)) <= {0, 1} and ((level == 0) == ok).all()
    if ok.any():
        assert filled[~ok].min(initial=300.0) >= 250.0 and filled[~ok].max(initial=300.0) <= 350.0      # a mean of LST values
    else:
        assert (filled == 0).all() and (level == -1).all()


def test_the_rasters_reach_what_they_are_planted_for():
    level = {n: R.fill_ref(a, None, True)[2] for n, (a, _) in RASTERS.items()}
    valid = {n: R.valid_ref(a) for n, (a, _) in RASTERS.items()}
    assert sorted(RASTERS) == ["150x100", "33x33", "37x50", "40x40", "45x61", "64x64"]
    assert (valid["37x50"] == 0).sum() == 5 and level["37x50"].max() == 1 and valid["37x50"][0, 0] == 0 and valid["37x50"][36, 49] == 0
    assert level["45x61"].max() >= 5                       # the aligned 16 x 16 hole is a whole level-4 cell
    assert R.select_ref(valid["45x61"], 16, 0, 0)[2] < 2 * 3
    assert level["150x100"].max() == 7                     # past the first application of a six-level reduction
    assert valid["150x100"][5, 5] == 0 and valid["150x100"][10, 90] == 0 and valid["150x100"][141].all()
    assert (R.valid_ref(*RASTERS["150x100"])[140:143] == 0).all()
    assert valid["64x64"].all() and not valid["40x40"].any()
    assert valid["33x33"].sum() == 1 and level["33x33"].max() == 6 and len(R.pyramid_ref(RASTERS["33x33"][0], valid["33x33"])) == 7
    f = R.fill_ref(*RASTERS["33x33"])[0]
    assert (f == np.float32(301.25)).all()


# ---- 2. select ---------------------------------------------------------------------------------------------------------------
def test_select_properties():
    rs = np.random.RandomState(7)
    inactive = 0
    for i, (n, w, v) in enumerate(_sweep()):
        m = w + (7 * n + 3 * i) % (2 * w + 1)                                # the other axis: anything from one window to three
        valid = np.zeros((n, m), np.uint8)
        for _ in range(rs.randint(0, 4)):                                   # a few valid pixels and one valid patch
            valid[rs.randint(n), rs.randint(m)] = 1
        y, x = rs.randint(n), rs.randint(m)
        valid[y:y + rs.randint(1, w), x:x + rs.randint(1, w)] = rs.randint(1, 256)
        if i % 50 == 0:
            valid[:] = i % 100 == 0                                         # all valid / all invalid
        for cover in (0, 1):
            slot, active, cnt = R.select_ref(valid, w, v, cover)
            oy, ox = origins(n, w, v, cover), origins(m, w, v, cover)
            T = len(oy) * len(ox)
            assert slot.shape == (T,) and active.shape == (cnt,) and slot.dtype == active.dtype == np.int32
            assert (np.diff(active) > 0).all()                              # sorted, no tile twice
            assert np.array_equal(slot[active], np.arange(cnt)) and (slot >= 0).sum() == cnt and slot.min(initial=0) >= -1
            on = set(active.tolist())
            pix = np.argwhere(valid)
            for py, px in pix[rs.permutation(len(pix))[:32]]:               # (a sample: the patch alone can hold thousands)
                cover_y = [a for a, o in enumerate(oy) if o <= py < o + w]
                cover_x = [b for b, o in enumerate(ox) if o <= px < o + w]
                assert all(a * len(ox) + b in on for a in cover_y for b in cover_x), (n, m, w, v, cover, py, px)
            for t in set(range(T)) - on:
                ty, tx = divmod(t, len(ox))
                assert not valid[oy[ty]:oy[ty] + w, ox[tx]:ox[tx] + w].any()
            inactive += T - cnt
            if valid.all():
                assert cnt == T and np.array_equal(slot, np.arange(T))
            if not valid.any():
                assert cnt == 0 and (slot == -1).all()
    assert inactive > 1000                                                  # (the sweep does skip tiles)


def test_masked_blend_restatement():
    """blend_gaps_ref: blend_ref at valid pixels whichever values the skipped tiles hold, fill_value elsewhere"""
    valid = R.valid_ref(RASTERS["45x61"][0])
    for win, overlap, cover in ((16, 8, 1), (16, 0, 0)):
        slot, active, n = R.select_ref(valid, win, overlap, cover)
        rs = np.random.RandomState(3)
        full = rs.standard_normal((len(slot), 1, 4 * win, 4 * win))
        want, m = R.blend_ref(full, valid.shape, win, overlap, cover, 307.0, 5.5)
        got, m2 = R.blend_gaps_ref(full[active], slot, valid, win, overlap, cover, 307.0, 5.5, -9999.0)
        up = R.upsampled(valid)
        assert n < len(slot) and np.array_equal(m, m2)
        assert np.array_equal(got[up], want[up]) and (got[~up] == -9999.0).all() and (got[up & ~m] == 0).all()
        assert (up & ~m).any() == (cover == 0)


# ---- 3. the pins of include/sifsr_gaps.h (the gate itself is tests/test_capi_gate.py) -------------------------------------------
def test_every_writing_gap_entry_point_has_a_contract_case(L):
    from tests import test_gaps_gpu as T
    writers = L.writers("gaps")
    assert len(L.declared("gaps")) == 5
    assert writers == {"sifsrg_fill": ["filled", "valid", "workspace"], "sifsrg_tiles_select": ["slot", "active", "n_active"],
                       "sifsrg_tiles_prepare": ["x"], "sifsrg_tiles_blend": ["out"]}
    assert "sifsrg_fill_workspace_bytes" in L.declared("gaps")                 # host only, no pointers: not a writer
    assert all(len(cases) >= 4 for cases in T.CONTRACT.values())


def test_fill_workspace_bytes(L):
    """host only: 12 bytes (a float64 sum, an int32 count) per cell of the levels above the raster; 0 for an invalid shape"""
    def cells(h, w):
        n = 0
        while True:
            h, w = (h + 1) // 2, (w + 1) // 2
            n += h * w
            if h == 1 and w == 1:
                return n
    for h, w in ((37, 50), (1200, 1200), (1, 1), (33, 33), (16384, 16384)):
        got = L.call("sifsrg_fill_workspace_bytes", h, w)
        assert got > 0 and got == 12 * cells(h, w), (h, w, got)
    for h, w in ((0, 5), (5, 0), (-1, 5), (16385, 4)):
        assert L.call("sifsrg_fill_workspace_bytes", h, w) == 0


def test_public_interface():
    import inspect

    import sifsr
    from sifsr import gaps, predict
    assert sifsr.gaps is gaps
    for name in ("fill_gaps", "select_tiles", "predict_granule_gaps"):
        assert getattr(predict, name) is getattr(gaps, name)
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(gaps.fill_gaps) == [("lst_g", E), ("mask", None)]
    assert sig(gaps.select_tiles) == [("valid", E), ("window", 64), ("overlap", 0), ("cover_edges", False)]
    got = sig(gaps.predict_granule_gaps)
    assert [k for k, _ in got] == ["model", "lst_g", "ndvi_g", "stats", "mask", "window", "batch", "overlap", "cover_edges",
                                   "fill_value", "return_info"]
    d = dict(got)
    assert (d["mask"], d["window"], d["batch"], d["overlap"], d["cover_edges"], d["return_info"]) == (None, 64, 256, 16, True, False)
    assert np.isnan(d["fill_value"])
    # the ungapped entry points keep their signatures
    assert [k for k, _ in sig(predict.predict_granule)] == ["model", "lst_g", "ndvi_g", "stats", "window", "batch", "overlap", "cover_edges"]
    import torch
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        gaps.fill_gaps(torch.zeros((8, 8)))
    with pytest.raises(sifsr.SifsrError):
        gaps.predict_granule_gaps(None, torch.zeros((64, 64)), torch.zeros((256, 256)), {})
