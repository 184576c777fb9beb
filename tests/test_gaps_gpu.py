"""GPU: gap-aware whole-granule prediction (include/sifsr_gaps.h, sifsr/gaps.py) against the NumPy restatement
tests/gaps_reference.py (held to itself by tests/test_gaps_host.py) and against the ungapped entry points.

Rasters (LST in [250, 350] K, seeded: gaps_reference.make_rasters), the smallest that reach each code path:

    37x50     single invalid pixels at two corners, on two edges and in the interior; a ragged pyramid on both axes
    45x61     a 16x16 hole aligned to a tile of window 16; a 5x9 hole across the 32-boundary of both axes
    150x100   a 70x80 hole that holds a whole 64-block, so its fill comes from level 7, out of the SECOND application of the
              six-level reduction; one NaN, one +inf and (with the mask) a stripe
    64x64     all valid            40x40   all invalid            33x33   one valid pixel at (32, 32): the fill is the top level

  * the memory contract of the four writing entry points in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is the
    table tests/test_capi_gate.py checks against the header); `x` tiles and `active` entries past n_active keep their poison, the
    fill workspace is poisoned scratch,
  * fill, select, compact prepare and masked blend for equality -- with the restatement, with sifsrx_tiles_prepare on the filled
    raster, with sifsrx_tiles_blend on the full tile set,
  * end to end: at valid pixels `predict_granule_gaps(gappy)` IS `predict_granule(fill_ref(gappy))`, NaN elsewhere; a gap-free
    raster gives `predict_granule`'s raster; and the harm of the ungapped path on a gappy raster, as a condition,
  * the argument errors.

Every comparison of kernel output is for equality except the one against the float64 blend (the bar of
test_mosaic_gpu.test_blend_restatement_and_coverage, 1e-5)."""
import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import gaps_reference as R
from tests.contract import L, S, bits, dev, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import Partial, bit_equal
from tests.test_mosaic_gpu import STATS, _granule, _model, origins

pytestmark = pytest.mark.gpu
I32, U8 = torch.int32, torch.uint8
SHAPE_ERR, ARG_ERR, WORKSPACE_ERR = 1001, 1002, 1003
RASTERS = R.make_rasters()


def ntiles(h, w, win, overlap, cover):
    return len(origins(h, win, overlap, cover)) * len(origins(w, win, overlap, cover))


def ndvi_for(h, w, seed=5):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal((4 * h, 4 * w)) * 0.6 + 0.5).astype(np.float32))


# ---- 1. memory contract --------------------------------------------------------------------------------------------------------
# (win, overlap, cover, lst_h, lst_w) and the hole that makes tiles inactive: one tile of six; four of 5 x 7; two of 4 x 3; none
LAYOUTS = [(16, 0, 0, 37, 50), (16, 8, 1, 45, 61), (64, 32, 1, 150, 100), (16, 8, 1, 16, 16)]
HOLES = [(slice(0, 16), slice(16, 32)), (slice(0, 24), slice(8, 32)), (slice(0, 100), slice(0, 70)), (slice(0, 4), slice(0, 4))]
INACTIVE = [1, 4, 2, 0]


def contract_raster(rs, i):
    win, overlap, cover, h, w = LAYOUTS[i]
    lst = rs.uniform(250.0, 350.0, (h, w)).astype(np.float32)
    lst[HOLES[i]] = 0.0
    lst[h - 1, w - 1] = 0.0
    lst[h // 2, w - 2] = 0.0
    return lst


def _partial(t, n):
    """rows < n of `t` written, the rest must keep what they held"""
    mask = (torch.arange(t.shape[0]) < n).reshape((-1,) + (1,) * (t.dim() - 1))
    init = t.clone()
    return lambda: Partial(t, mask, init)


def fill_case(i, with_mask):
    def make(k):
        _, _, _, h, w = LAYOUTS[i]
        lst = k.t("lst", torch.from_numpy(contract_raster(k.rs, i)))
        mask = k.t("mask", torch.from_numpy((k.rs.uniform(size=(h, w)) > 0.1).astype(np.uint8))) if with_mask else None
        filled, valid = k.o("filled", h, w), k.o("valid", h, w, dtype=U8)
        need = k.L.call("sifsrg_fill_workspace_bytes", h, w)
        ws = k.A.scratch(need, "workspace")                       # poisoned scratch: nothing of it may reach the outputs
        call = lambda: k.L.call("sifsrg_fill", lst, mask, filled, valid, ws, need, h, w, S())
        return call, {"filled": filled, "valid": valid}
    return make


def select_case(i):
    def make(k):
        win, overlap, cover, h, w = LAYOUTS[i]
        valid_np = R.valid_ref(contract_raster(k.rs, i))
        T, n = ntiles(h, w, win, overlap, cover), R.select_ref(valid_np, win, overlap, cover)[2]
        assert T - n == INACTIVE[i]
        valid = k.t("valid", torch.from_numpy(valid_np))
        slot, active, n_active = k.o("slot", T, dtype=I32), k.o("active", T, dtype=I32), k.o("n_active", 1, dtype=I32)
        call = lambda: k.L.call("sifsrg_tiles_select", valid, slot, active, n_active, h, w, win, overlap, cover, S())
        return call, {"slot": slot, "active": _partial(active, n), "n_active": n_active}
    return make


def prepare_case(i):
    def make(k):
        win, overlap, cover, h, w = LAYOUTS[i]
        hr = 4 * win
        lst = contract_raster(k.rs, i)
        _, active_np, n = R.select_ref(R.valid_ref(lst), win, overlap, cover)
        T = ntiles(h, w, win, overlap, cover)
        act = np.full(T, -12345, np.int32)                          # entries >= n: never to be used
        act[:n] = active_np
        filled = k.t("filled", torch.from_numpy(R.fill_ref(lst)[0]))
        ndvi = k.i("ndvi", 4 * h, 4 * w, scale=0.5)
        active, n_active = k.t("active", torch.from_numpy(act)), k.t("n_active", torch.tensor([n], dtype=I32))
        x = k.o("x", T, 2, hr, hr)                                 # cap = T: the tiles past n_active keep their poison
        call = lambda: k.L.call("sifsrg_tiles_prepare", filled, ndvi, x, active, n_active, T, h, w, win, overlap, cover, 307.2378,
                                5.5698, 0.3, 0.2, 1, S())
        return call, {"x": _partial(x, n)}
    return make


def blend_case(i):
    def make(k):
        win, overlap, cover, h, w = LAYOUTS[i]
        hr = 4 * win
        valid_np = R.valid_ref(contract_raster(k.rs, i))
        slot_np, _, n = R.select_ref(valid_np, win, overlap, cover)
        sr = k.i("sr", n, 1, hr, hr)
        slot, valid = k.t("slot", torch.from_numpy(slot_np)), k.t("valid", torch.from_numpy(valid_np))
        out = k.o("out", 4 * h, 4 * w)                              # EVERY element is the call's to write
        call = lambda: k.L.call("sifsrg_tiles_blend", sr, slot, valid, out, h, w, win, overlap, cover, 307.2378, 5.5698, -9999.0, S())
        return call, {"out": out}
    return make


R4 = range(len(LAYOUTS))
CONTRACT = {"sifsrg_fill": [fill_case(i, m) for i in R4 for m in (False, True)], "sifsrg_tiles_select": [select_case(i) for i in R4],
            "sifsrg_tiles_prepare": [prepare_case(i) for i in R4], "sifsrg_tiles_blend": [blend_case(i) for i in R4]}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output written where the header says and nowhere else -- NaN-free under the NaN poison, bit-identical under every
    poison (the poisoned fill workspace included), `x` tiles and `active` entries past n_active still holding their poison --,
    inputs untouched, nothing outside the buffers written, and the same bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=64 << 20)


def test_workspace_too_small(L):
    lst = dev(RASTERS["37x50"][0])
    need = L.call("sifsrg_fill_workspace_bytes", 37, 50)
    filled, valid = torch.full((37, 50), 77.0, device="cuda"), torch.full((37, 50), 77, dtype=U8, device="cuda")
    ws = torch.full((need,), 77, dtype=U8, device="cuda")
    fn = L.lib().sifsrg_fill
    assert fn(lst.data_ptr(), None, filled.data_ptr(), valid.data_ptr(), ws.data_ptr(), need - 1, 37, 50, S()) == WORKSPACE_ERR
    assert fn(lst.data_ptr(), None, filled.data_ptr(), valid.data_ptr(), ws.data_ptr(), 0, 37, 50, S()) == WORKSPACE_ERR
    torch.cuda.synchronize()
    assert (filled == 77).all() and (valid == 77).all() and (ws == 77).all()
    assert fn(lst.data_ptr(), None, filled.data_ptr(), valid.data_ptr(), ws.data_ptr(), need, 37, 50, S()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(filled), bits(R.fill_ref(RASTERS["37x50"][0])[0]))


# ---- 2. fill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("name", sorted(RASTERS))
def test_fill_bit_equal(sifsr, name, with_mask):
    lst, mask = RASTERS[name]
    mask = mask if with_mask else None
    want_f, want_v = R.fill_ref(lst, mask)
    filled, valid = sifsr.predict.fill_gaps(dev(lst), None if mask is None else dev(mask))
    assert filled.dtype == torch.float32 and valid.dtype == U8 and tuple(filled.shape) == tuple(valid.shape) == lst.shape
    assert np.array_equal(valid.cpu().numpy(), want_v)
    assert np.array_equal(bits(filled), bits(want_f))
    if mask is not None:                                               # a bool mask is the same mask
        f2, v2 = sifsr.gaps.fill_gaps(dev(lst), dev(mask).bool())
        assert bit_equal(f2, filled) and bit_equal(v2, valid)


# ---- 3. select -----------------------------------------------------------------------------------------------------------------
def run_select(sifsr, valid_np, win, overlap, cover):
    slot, active, n = sifsr.gaps.select_tiles(dev(valid_np), win, overlap, bool(cover))
    assert slot.dtype == active.dtype == n.dtype == I32 and tuple(n.shape) == (1,)
    return slot.cpu().numpy(), active.cpu().numpy(), int(n.item())


@pytest.mark.parametrize("name,win,overlap,cover", [("45x61", 16, 0, 0), ("45x61", 16, 8, 1), ("45x61", 16, 8, 0), ("150x100", 64, 32, 1)])
def test_select_equals_the_restatement(sifsr, name, win, overlap, cover):
    valid = R.valid_ref(RASTERS[name][0])
    want_slot, want_active, want_n = R.select_ref(valid, win, overlap, cover)
    slot, active, n = run_select(sifsr, valid, win, overlap, cover)
    assert n == want_n and np.array_equal(slot, want_slot) and np.array_equal(active[:n], want_active)
    if (name, win, overlap, cover) == ("45x61", 16, 0, 0):
        assert n < len(slot) and slot[1] == -1                       # the aligned 16 x 16 hole IS tile (0, 1)
    # a bool raster and any non-zero byte select the same tiles
    s2, a2, n2 = sifsr.gaps.select_tiles(dev(valid).bool(), win, overlap, bool(cover))
    s3, a3, n3 = sifsr.gaps.select_tiles(dev(valid * 200), win, overlap, bool(cover))
    assert int(n2) == int(n3) == n and np.array_equal(s2.cpu().numpy(), slot) and np.array_equal(s3.cpu().numpy(), slot)


def test_select_all_and_nothing(L):
    for name, win in (("40x40", 16), ("64x64", 16), ("64x64", 64)):
        valid = R.valid_ref(RASTERS[name][0])
        h, w = valid.shape
        T = ntiles(h, w, win, 8, 1)
        slot, active, n = (torch.full((T,), 77, dtype=I32, device="cuda") for _ in range(3))
        L.call("sifsrg_tiles_select", dev(valid), slot, active, n[:1], h, w, win, 8, 1, S())
        torch.cuda.synchronize()
        if valid.any():
            assert int(n[0]) == T and slot.cpu().tolist() == list(range(T)) == active.cpu().tolist()
        else:
            assert int(n[0]) == 0 and (slot == -1).all() and (active == 77).all()          # `active` untouched from n on


# ---- 4. compact prepare --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,win,overlap,cover", [("45x61", 16, 8, 1), ("45x61", 16, 0, 0), ("150x100", 64, 32, 1)])
def test_compact_prepare_is_the_full_prepare(sifsr, L, name, win, overlap, cover):
    lst = RASTERS[name][0]
    h, w = lst.shape
    filled_np, valid = R.fill_ref(lst)
    _, active, n = R.select_ref(valid, win, overlap, cover)
    T = ntiles(h, w, win, overlap, cover)
    assert 0 < n < T
    filled, ndvi = dev(filled_np), ndvi_for(h, w).cuda()
    ndvi[3, 5] = float("nan")                                          # not sanitised: the clip makes it -1 in both
    full = torch.empty((T, 2, 4 * win, 4 * win), device="cuda")
    L.call("sifsrx_tiles_prepare", filled, ndvi, full, h, w, win, overlap, cover, STATS["mean_lst"], STATS["std_lst"],
           STATS["mean_ndvi"], STATS["std_ndvi"], 1, S())
    slot_d, active_d, n_d = sifsr.gaps.select_tiles(dev(valid), win, overlap, bool(cover))
    x = sifsr.gaps.prepare_active_tiles(filled, ndvi, STATS, active_d, n_d, n, win, overlap, bool(cover))
    assert tuple(x.shape) == (n, 2, 4 * win, 4 * win)
    for i in range(n):
        assert bit_equal(x[i], full[active[i]]), i
    assert not torch.isnan(x).any()
    # cap > n_active: the tiles past it are untouched; cap < n_active: the first cap tiles
    big = torch.full((n + 2, 2, 4 * win, 4 * win), 77.0, device="cuda")
    L.call("sifsrg_tiles_prepare", filled, ndvi, big, active_d, n_d, n + 2, h, w, win, overlap, cover, STATS["mean_lst"],
           STATS["std_lst"], STATS["mean_ndvi"], STATS["std_ndvi"], 1, S())
    small = torch.full((n, 2, 4 * win, 4 * win), 77.0, device="cuda")
    L.call("sifsrg_tiles_prepare", filled, ndvi, small, active_d, n_d, n - 1, h, w, win, overlap, cover, STATS["mean_lst"],
           STATS["std_lst"], STATS["mean_ndvi"], STATS["std_ndvi"], 1, S())
    torch.cuda.synchronize()
    assert bit_equal(big[:n], x) and (big[n:] == 77).all()
    assert bit_equal(small[:n - 1], x[:n - 1]) and (small[n - 1] == 77).all()


# ---- 5. masked blend -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill_value", [float("nan"), -9999.0])
@pytest.mark.parametrize("name,win,overlap,cover", [("45x61", 16, 8, 1), ("45x61", 16, 0, 0), ("45x61", 16, 8, 0), ("150x100", 64, 32, 1)])
def test_masked_blend(sifsr, L, name, win, overlap, cover, fill_value):
    lst = RASTERS[name][0]
    h, w = lst.shape
    valid = R.valid_ref(lst)
    slot, active, n = R.select_ref(valid, win, overlap, cover)
    T = len(slot)
    assert 0 < n < T
    rs = np.random.RandomState(100 * win + 10 * overlap + cover)
    sr_full = (rs.standard_normal((T, 1, 4 * win, 4 * win)) * 1.5).astype(np.float32)
    full = torch.empty((4 * h, 4 * w), device="cuda")
    L.call("sifsrx_tiles_blend", dev(sr_full), full, h, w, win, overlap, cover, STATS["mean_lst"], STATS["std_lst"], S())
    out = sifsr.gaps.blend_active_tiles(dev(sr_full[active]), dev(slot), dev(valid), win, STATS, overlap, bool(cover), fill_value)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), full.cpu().numpy()
    up = R.upsampled(valid)
    ref, covered = R.blend_gaps_ref(sr_full[active], slot, valid, win, overlap, cover, STATS["mean_lst"], STATS["std_lst"], fill_value)
    assert np.array_equal(bits(got)[up], bits(want)[up])                                   # the ungapped blend, bit for bit
    assert (bits(got)[~up] == np.float32(fill_value).view(np.uint32)).all() and (~up).any()
    assert (got[up & ~covered] == 0).all() and (up & ~covered).any() == (cover == 0)
    m = up & covered
    err = np.abs(got[m] - ref[m]).max() / np.abs(ref[m]).max()
    print(f"masked blend {name} win {win} overlap {overlap} cover {cover}: max|out - ref| / max|ref| = {err:.3e} at valid pixels")
    assert err < 1e-5


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def gappy_200x136():
    lst_g, ndvi_g = _granule()
    lst = lst_g.numpy().copy()
    lst[:64, :] = 0.0
    lst[:, :64] = 0.0
    return lst, ndvi_g


E2E = {"45x61": dict(window=16, overlap=8, cover_edges=True, batch=4), "200x136": dict(window=64, overlap=16, cover_edges=True, batch=5)}


def e2e_inputs(name):
    if name == "45x61":
        return RASTERS["45x61"][0], ndvi_for(45, 61)
    return gappy_200x136()


@pytest.fixture(scope="module")
def model(sifsr):
    return _model(sifsr, O.synthetic_state(3))


@pytest.mark.parametrize("name", sorted(E2E))
def test_end_to_end(sifsr, model, name):
    """at valid pixels the gap-aware call IS predict_granule on the filled raster (same layout), NaN elsewhere; and on the 200x136
    case THE HARM IT REMOVES, as a condition: among the valid pixels at least 8 LST pixels from any invalid one, the ungapped call
    on the gappy raster is off by more than 1 K somewhere (a 0 K pixel is about 55 sigma), the gap-aware one by nothing."""
    lst, ndvi_g = e2e_inputs(name)
    kw = E2E[name]
    lay = (kw["window"], kw["overlap"], 1)
    filled_np, valid = R.fill_ref(lst)
    ndvi = ndvi_g.cuda()
    out, info = sifsr.predict.predict_granule_gaps(model, dev(lst), ndvi, STATS, return_info=True, **kw)
    want = sifsr.predict.predict_granule(model, dev(filled_np), ndvi, STATS, **kw)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), want.cpu().numpy()
    up = R.upsampled(valid)
    assert got.shape == (4 * lst.shape[0], 4 * lst.shape[1]) and got.dtype == np.float32
    assert np.array_equal(bits(got)[up], bits(want)[up])
    assert np.isnan(got[~up]).all() and not np.isnan(got[up]).any() and (~up).any()
    n_ref = R.select_ref(valid, *lay)[2]
    assert info["n_active"] == n_ref < info["n_tiles"] == ntiles(*lst.shape, *lay)
    assert info["valid"].dtype == torch.bool and np.array_equal(info["valid"].cpu().numpy(), valid != 0)
    print(f"{name}: {info['n_active']} of {info['n_tiles']} tiles active")
    if name == "200x136":
        assert (info["n_active"], info["n_tiles"]) == (6, 12)
        plain = sifsr.predict.predict_granule(model, dev(lst), ndvi, STATS, **kw).cpu().numpy()
        far = R.upsampled(R.min_chebyshev_distance_mask(valid, 8))
        assert far.any() and not (far & ~up).any()
        harm = np.abs(plain[far].astype(np.float64) - want[far]).max()
        print(f"ungapped predict_granule on the gappy raster, valid pixels >= 8 px from a gap: off by up to {harm:.3f} K")
        assert harm > 1.0
        assert np.array_equal(bits(got)[far], bits(want)[far])
    # a mask does what a 0 K pixel does
    mask = (valid != 0).astype(np.uint8)
    lst2 = np.where(valid != 0, lst, np.float32(333.0)).astype(np.float32)
    out2 = sifsr.predict.predict_granule_gaps(model, dev(lst2), ndvi, STATS, mask=dev(mask), **kw)
    assert bit_equal(out2, out)
    # another fill value
    out3 = sifsr.predict.predict_granule_gaps(model, dev(lst), ndvi, STATS, fill_value=-9999.0, **kw).cpu().numpy()
    assert np.array_equal(bits(out3)[up], bits(got)[up]) and (out3[~up] == -9999.0).all()


@pytest.mark.parametrize("name", sorted(E2E))
def test_gap_free_is_predict_granule(sifsr, model, name):
    lst, ndvi_g = e2e_inputs(name)
    lst = np.where(lst == 0, np.float32(300.0), lst).astype(np.float32)
    kw = E2E[name]
    out, info = sifsr.predict.predict_granule_gaps(model, dev(lst), ndvi_g.cuda(), STATS, return_info=True, **kw)
    want = sifsr.predict.predict_granule(model, dev(lst), ndvi_g.cuda(), STATS, **kw)
    assert bit_equal(out, want) and not torch.isnan(out).any()
    assert info["n_active"] == info["n_tiles"] and bool(info["valid"].all())


def test_nothing_valid_runs_no_forward(sifsr):
    class NoForward(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("a forward ran on a granule without a valid pixel")
    out, info = sifsr.predict.predict_granule_gaps(NoForward(), dev(RASTERS["40x40"][0]), ndvi_for(40, 40).cuda(), STATS, window=16,
                                                   overlap=8, return_info=True)
    assert tuple(out.shape) == (160, 160) and torch.isnan(out).all()
    assert info["n_active"] == 0 and info["n_tiles"] == 16 and not bool(info["valid"].any())
    out = sifsr.predict.predict_granule_gaps(NoForward(), dev(RASTERS["40x40"][0]), ndvi_for(40, 40).cuda(), STATS, window=16,
                                             overlap=8, fill_value=-1.0)
    assert (out == -1.0).all()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_errors(sifsr, L, model):
    lst_g, ndvi_g = _granule()
    lst_c, ndvi_c = lst_g.cuda(), ndvi_g.cuda()
    E, G = sifsr.SifsrError, sifsr.gaps
    # the bad layouts of test_mosaic_gpu.test_errors, before any launch
    bad = [dict(overlap=-1), dict(overlap=33), dict(overlap=9, window=16), dict(window=128, overlap=8), dict(window=68, cover_edges=True),
           dict(window=64, overlap=16, lst=lst_c[:40].contiguous(), ndvi=ndvi_c[:160].contiguous()),      # raster smaller than a window
           dict(overlap=16, ndvi=ndvi_c[:, :540].contiguous()), dict(cover_edges=True, ndvi=ndvi_c[:796].contiguous())]
    for kw in bad:
        kw = dict(kw)
        a, b = kw.pop("lst", lst_c), kw.pop("ndvi", ndvi_c)
        with pytest.raises(E):
            G.predict_granule_gaps(model, a, b, STATS, **kw)
    valid = torch.ones((200, 136), dtype=U8, device="cuda")
    for kw in (dict(overlap=-1), dict(overlap=33), dict(window=62), dict(window=128)):
        with pytest.raises(E):
            G.select_tiles(valid, **kw)
    # mask: shape, dtype, device; batch and cap
    for mask in (valid[:199], valid.float(), valid.to(torch.int32), valid.cpu(), np.ones((200, 136), np.uint8)):
        with pytest.raises(E):
            G.fill_gaps(lst_c, mask)
        with pytest.raises(E):
            G.predict_granule_gaps(model, lst_c, ndvi_c, STATS, mask=mask)
    with pytest.raises(E):
        G.select_tiles(valid.float())
    with pytest.raises(E):
        G.predict_granule_gaps(model, lst_c, ndvi_c, STATS, batch=0)
    slot, active, n = G.select_tiles(valid, 64, 16, True)
    for cap in (0, -3):
        with pytest.raises(E):
            G.prepare_active_tiles(lst_c, ndvi_c, STATS, active, n, cap, 64, 16, True)
    with pytest.raises(E):
        G.fill_gaps(lst_c.double())
    # the C entry points: 1001 for the same layouts and 1002 for null pointers, nothing launched (the poisoned outputs keep every bit)
    h = L.lib()
    p = lambda t: t.data_ptr()
    x = torch.full((12, 2, 256, 256), 77.0, device="cuda")
    sr = torch.zeros((12, 1, 256, 256), device="cuda")
    out = torch.full((800, 544), 77.0, device="cuda")
    filled, ws = torch.full((200, 136), 77.0, device="cuda"), torch.full((L.call("sifsrg_fill_workspace_bytes", 200, 136),), 77, dtype=U8, device="cuda")
    val = torch.full((200, 136), 77, dtype=U8, device="cuda")
    sl, ac, na = (torch.full((12,), 77, dtype=I32, device="cuda") for _ in range(3))
    one = torch.ones((1,), dtype=I32, device="cuda")
    for hh, ww, win, ov in ((200, 136, 64, -1), (200, 136, 64, 33), (200, 136, 128, 8), (200, 136, 16, 9), (40, 136, 64, 16),
                            (200, 63, 64, 0), (200, 136, 62, 0), (200, 136, 0, 0)):
        for cover in (0, 1):
            assert h.sifsrg_tiles_select(p(valid), p(sl), p(ac), p(na), hh, ww, win, ov, cover, S()) == SHAPE_ERR
            assert h.sifsrg_tiles_prepare(p(lst_c), p(ndvi_c), p(x), p(active), p(n), 12, hh, ww, win, ov, cover, 307.0, 5.5, 0.6, 0.2, 1,
                                          S()) == SHAPE_ERR
            assert h.sifsrg_tiles_blend(p(sr), p(slot), p(valid), p(out), hh, ww, win, ov, cover, 307.0, 5.5, -1.0, S()) == SHAPE_ERR
    assert h.sifsrg_tiles_prepare(p(lst_c), p(ndvi_c), p(x), p(active), p(n), 0, 200, 136, 64, 16, 1, 307.0, 5.5, 0.6, 0.2, 1, S()) == SHAPE_ERR
    assert h.sifsrg_tiles_prepare(p(lst_c), p(ndvi_c), p(x), p(active), p(n), 12, 200, 136, 64, 16, 1, 307.0, 0.0, 0.6, 0.2, 1, S()) == SHAPE_ERR
    for hh, ww in ((0, 136), (200, 0), (16385, 4)):
        assert h.sifsrg_fill(p(lst_c), None, p(filled), p(val), p(ws), ws.numel(), hh, ww, S()) == SHAPE_ERR
    assert h.sifsrg_fill(None, None, p(filled), p(val), p(ws), ws.numel(), 200, 136, S()) == ARG_ERR
    assert h.sifsrg_fill(p(lst_c), None, None, p(val), p(ws), ws.numel(), 200, 136, S()) == ARG_ERR
    assert h.sifsrg_fill(p(lst_c), None, p(filled), None, p(ws), ws.numel(), 200, 136, S()) == ARG_ERR
    assert h.sifsrg_fill(p(lst_c), None, p(filled), p(val), None, ws.numel(), 200, 136, S()) == ARG_ERR
    assert h.sifsrg_fill(p(lst_c), None, p(filled), p(val), p(ws) + 4, ws.numel() - 4, 200, 136, S()) == ARG_ERR   # not 8-byte aligned
    for i in range(4):
        a = [p(valid), p(sl), p(ac), p(na)]
        a[i] = None
        assert h.sifsrg_tiles_select(*a, 200, 136, 64, 16, 1, S()) == ARG_ERR
    for i in range(5):
        a = [p(lst_c), p(ndvi_c), p(x), p(active), p(one)]
        a[i] = None
        assert h.sifsrg_tiles_prepare(*a, 12, 200, 136, 64, 16, 1, 307.0, 5.5, 0.6, 0.2, 1, S()) == ARG_ERR
    for i in range(4):
        a = [p(sr), p(slot), p(valid), p(out)]
        a[i] = None
        assert h.sifsrg_tiles_blend(*a, 200, 136, 64, 16, 1, 307.0, 5.5, -1.0, S()) == ARG_ERR
    torch.cuda.synchronize()
    for t in (x, out, filled, val, ws, sl, ac, na):
        assert (t == 77).all()
