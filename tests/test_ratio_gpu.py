"""GPU: whole-granule prediction at any ratio (include/sifsr_ratio.h, sifsr/ratio.py) against the float64 NumPy
restatement tests/ratio_reference.py (held to torch's float64 bicubic and to the host entry points by tests/test_ratio_host.py),
against the x4 entry points where the ratio is 4, and, end to end, against the float64 oracle.

  * the memory contract of the three writing entry points in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is
    the table tests/test_ratio_host.py checks against the header); `x` tiles past min(n_active, cap) keep their poison,
  * the resampler, the per-tile pipeline and the blend for value, and for equality wherever the header promises bits,
  * the masked blend under the floor(Y q / p) rule, the two granule calls end to end, a training step at x3 fed by ``ratio.upsample``,
  * the error codes.

Bars.  Resampler and pipeline against float64: 1e-5 max(1, max|ref|), the bar of test_prepare_tiles in tests/test_pipeline_gpu.py
(with exact phases what remains is the fp32 rounding of four weights and two sums of four terms: about 1e-7).  Blend: 1e-6 for the
partition of unity and 1e-5 against the restatement, the bars of tests/test_mosaic_gpu.py.  End to end: 1e-4 relative, the project's
parity bar.  Every other comparison is for equality.  Rasters are a few thousand pixels; each case runs in well under a second."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sif_oracle as O
from tests import gaps_reference as GR
from tests import ratio_reference as R
from tests.conftest import rel_err
from tests.contract import L, S, bits, dev, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import Partial, bit_equal
from tests.test_model_gpu import make_model, normalised_per_image_err
from tests.test_mosaic_gpu import STATS, UNIT, _model
from tests.test_ratio_host import UPSAMPLE_SHAPES

pytestmark = pytest.mark.gpu
I32, U8 = torch.int32, torch.uint8
SHAPE_ERR, ARG_ERR = 1001, 1002
M, SD = STATS["mean_lst"], STATS["std_lst"]


def bar(ref):
    return 1e-5 * max(1.0, float(np.abs(ref).max()))


def rasters(seed, h, w, p, q):
    """LST in Kelvin and an NDVI raster that leaves [-1, 1] here and there (the clip has something to do)"""
    rs = np.random.RandomState(seed)
    lst = (rs.standard_normal((h, w)) * 5.5 + 307).astype(np.float32)
    ndvi = (rs.standard_normal((h * p // q, w * p // q)) * 0.6 + 0.5).astype(np.float32)
    return lst, ndvi


def ntiles(h, w, win, hr, overlap, cover):
    ty, tx = R.geometry_ref((h, w), win, hr, overlap, cover)[2]
    return ty * tx


# ---- 1. memory contract ----------------------------------------------------------------------------------------------------------
# (B, h, w, H, W): a single pixel (every index clamps), a ratio of its own per axis with H and W no multiple of anything, several
# images, more than one workgroup on both axes (H > 16, W > 256), an axis that is copied
UPSAMPLE_CONTRACT = [(1, 1, 1, 8, 8), (1, 2, 3, 7, 5), (3, 8, 8, 24, 24), (2, 5, 130, 19, 300), (2, 6, 9, 6, 23)]
# (win, hr, h, w, overlap, cover, mode): all tiles, or the compact list with cap above / below n_active
PREPARE_CONTRACT = [(8, 24, 21, 27, 2, 1, "all"), (16, 40, 38, 46, 2, 1, "all"), (12, 32, 27, 33, 3, 0, "all"),
                    (8, 24, 21, 27, 2, 1, "cap>n"), (16, 40, 38, 46, 2, 1, "cap<n"), (12, 32, 27, 33, 6, 1, "cap>n"), (8, 24, 21, 27, 0, 0, "cap<n")]
# (h, w, (win, hr), overlap, cover, masked): (16, 40) at overlap 2 is the odd stride (HR 35); no raster is a whole number of strides,
# so with cover the flush tile overlaps its neighbour by more than `overlap`
BLEND_CONTRACT = [(21, 27, (8, 24), 0, 0, False), (21, 27, (8, 24), 2, 1, False), (38, 46, (16, 40), 2, 1, False), (38, 46, (16, 40), 2, 0, True),
                  (27, 33, (12, 32), 3, 1, True), (21, 27, (8, 24), 4, 1, True), (38, 46, (16, 40), 0, 1, True), (21, 27, (8, 32), 2, 0, False)]


def _partial(t, n):
    """rows < n of `t` written, the rest must keep what they held"""
    mask = (torch.arange(t.shape[0]) < n).reshape((-1,) + (1,) * (t.dim() - 1))
    init = t.clone()
    return lambda: Partial(t, mask, init)


def upsample_case(B, h, w, H, W):
    def make(k):
        x, out = k.i("x", B, h, w, scale=5.0, shift=300.0), k.o("out", B, H, W)
        return (lambda: k.L.call("sifsrr_upsample", x, out, B, h, w, H, W, S())), {"out": out}
    return make


def prepare_case(win, hr, h, w, overlap, cover, mode):
    def make(k):
        p, q, (ty, tx), (H, W) = R.geometry_ref((h, w), win, hr, overlap, cover)
        T = ty * tx
        lst, ndvi = k.i("lst", h, w, scale=5.0, shift=300.0), k.i("ndvi", H, W, scale=0.5)
        if mode == "all":
            x = k.o("x", T, 2, hr, hr)
            call = lambda: k.L.call("sifsrr_tiles_prepare", lst, ndvi, x, None, None, T, h, w, win, hr, overlap, cover, 307.2378, 5.5698,
                                    0.3, 0.2, 1, S())
            return call, {"x": x}
        chosen = np.arange(T)[1::2]                             # every other tile, increasing
        n = len(chosen)
        cap = n + 2 if mode == "cap>n" else n - 1
        assert 1 <= cap and n >= 2
        act = np.full(T, -12345, np.int32)                                 # entries >= n: never to be used
        act[:n] = chosen
        active, n_active = k.t("active", torch.from_numpy(act)), k.t("n_active", torch.tensor([n], dtype=I32))
        x = k.o("x", cap, 2, hr, hr)
        call = lambda: k.L.call("sifsrr_tiles_prepare", lst, ndvi, x, active, n_active, cap, h, w, win, hr, overlap, cover, 307.2378,
                                5.5698, 0.3, 0.2, 1, S())
        return call, {"x": _partial(x, min(n, cap))}
    return make


def holed_valid(rs, h, w, win):
    """a validity raster with the first window all invalid, its neighbour half invalid and a few scattered invalid pixels"""
    valid = (rs.uniform(size=(h, w)) > 0.08).astype(np.uint8)
    valid[:win, :win] = 0
    valid[:win // 2, win:2 * win] = 0
    valid[h - 1, w - 1] = 0
    return valid


def blend_case(h, w, pair, overlap, cover, masked):
    def make(k):
        win, hr = pair
        p, q, (ty, tx), (H, W) = R.geometry_ref((h, w), win, hr, overlap, cover)
        out = k.o("out", H, W)                                          # EVERY element is the call's to write
        if not masked:
            sr = k.i("sr", ty * tx, 1, hr, hr)
            call = lambda: k.L.call("sifsrr_tiles_blend", sr, None, None, out, h, w, win, hr, overlap, cover, 307.2378, 5.5698, 0.0, S())
        else:
            valid_np = holed_valid(k.rs, h, w, win)
            slot_np, _, n = GR.select_ref(valid_np, win, overlap, cover)
            assert 0 < n < ty * tx
            sr = k.i("sr", n, 1, hr, hr)
            slot, valid = k.t("slot", torch.from_numpy(slot_np)), k.t("valid", torch.from_numpy(valid_np))
            call = lambda: k.L.call("sifsrr_tiles_blend", sr, slot, valid, out, h, w, win, hr, overlap, cover, 307.2378, 5.5698, -9999.0, S())
        return call, {"out": out}
    return make


CONTRACT = {"sifsrr_upsample": [upsample_case(*c) for c in UPSAMPLE_CONTRACT],
            "sifsrr_tiles_prepare": [prepare_case(*c) for c in PREPARE_CONTRACT],
            "sifsrr_tiles_blend": [blend_case(*c) for c in BLEND_CONTRACT]}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output written where the header says and nowhere else -- NaN-free under the NaN poison, bit-identical under every
    poison, `x` tiles past min(n_active, cap) still holding their poison --, inputs untouched, nothing outside the buffers
    written, and the same bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=48 << 20)


# ---- 2. the resampler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,size", UPSAMPLE_SHAPES + [((64, 64), (128, 128))], ids=lambda v: "x".join(map(str, v)))
def test_upsample_against_float64(sifsr, shape, size):
    x = np.random.RandomState(sum(shape) + sum(size)).standard_normal((2,) + shape).astype(np.float32)
    ref = R.upsample_ref(x, size)
    out = sifsr.ratio.upsample(dev(x), size)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2,) + size
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"upsample {shape} -> {size}: max|out - float64| = {err:.3e} (max|ref| {np.abs(ref).max():.2f}, bar {bar(ref):.1e})")
    assert err <= bar(ref)
    # the forms (h,w) and (B,C,h,w) are the same images
    assert bit_equal(sifsr.ratio.upsample(dev(x[0]), size), out[0])
    assert bit_equal(sifsr.ratio.upsample(dev(x[:, None]), size)[:, 0], out)


def test_upsample_equal_axis_is_a_copy(sifsr):
    x = np.random.RandomState(4).standard_normal((3, 21, 37)).astype(np.float32) * 300
    assert bit_equal(sifsr.ratio.upsample(dev(x), (21, 37)), dev(x))
    # one axis equal: that axis is the identity on the other axis' result
    wide = sifsr.ratio.upsample(dev(x), (21, 300)).cpu().numpy()
    ref = R.upsample_ref(x, (21, 300))
    assert np.abs(wide - ref).max() <= bar(ref)
    row = sifsr.ratio.upsample(dev(x[:, 5:6]), (1, 300)).cpu().numpy()
    assert np.array_equal(bits(row[:, 0]), bits(wide[:, 5]))
    tall = sifsr.ratio.upsample(dev(x), (50, 37)).cpu().numpy()
    col = sifsr.ratio.upsample(dev(np.ascontiguousarray(x[:, :, 7:8])), (50, 1)).cpu().numpy()
    assert np.array_equal(bits(col[:, :, 0]), bits(tall[:, :, 7]))


# ---- 3. prepare --------------------------------------------------------------------------------------------------------------------
LAYOUTS = [(8, 24, 21, 27, 2, 1), (16, 40, 38, 46, 2, 1), (12, 32, 27, 33, 3, 0), (64, 160, 64, 128, 0, 0), (8, 24, 21, 27, 0, 0)]


@pytest.mark.parametrize("win,hr,h,w,overlap,cover", LAYOUTS)
def test_prepare_against_float64_and_the_resampler(sifsr, win, hr, h, w, overlap, cover):
    p, q, (ty, tx), _ = R.geometry_ref((h, w), win, hr, overlap, cover)
    lst, ndvi = rasters(win + hr, h, w, p, q)
    x, tiles = sifsr.ratio.granule_to_tiles(dev(lst), dev(ndvi), STATS, win, hr, True, overlap, bool(cover))
    assert tiles == (ty, tx) and tuple(x.shape) == (ty * tx, 2, hr, hr)
    ref = R.prepare_ref(lst, ndvi, STATS, win, hr, overlap, cover, True)
    err = float(np.abs(x.cpu().numpy() - ref).max())
    print(f"prepare ({win},{hr}) {h}x{w} overlap {overlap} cover {cover}: max|x - float64| = {err:.3e} (bar {bar(ref):.1e})")
    assert err <= bar(ref)
    # unit statistics: plane 0 of every tile IS ratio.upsample of its block, plane 1 the NDVI block
    xu, _ = sifsr.ratio.granule_to_tiles(dev(lst), dev(ndvi), UNIT, win, hr, False, overlap, bool(cover))
    oy, ox = R.origins(h, win, overlap, cover), R.origins(w, win, overlap, cover)
    blocks = np.stack([lst[i:i + win, j:j + win] for i in oy for j in ox])
    nblocks = np.stack([ndvi[i * p // q:i * p // q + hr, j * p // q:j * p // q + hr] for i in oy for j in ox])
    assert bit_equal(xu[:, 0], sifsr.ratio.upsample(dev(blocks), (hr, hr)))
    assert bit_equal(xu[:, 1], dev(nblocks))
    # the training-batch form is the same device function
    xb = sifsr.ratio.prepare_tiles(dev(blocks[:, None]), dev(nblocks[:, None]), STATS, True)
    assert bit_equal(xb, x)
    # compact: the same tiles of the full call; tiles past min(n_active, cap) untouched
    T = ty * tx
    act = np.arange(T)[::2].astype(np.int32)
    n = len(act)
    active = torch.full((T,), -5, dtype=I32, device="cuda")
    active[:n] = dev(act)
    n_active = torch.tensor([n], dtype=I32, device="cuda")
    xc = sifsr.ratio.prepare_active_tiles(dev(lst), dev(ndvi), STATS, active, n_active, n + 1, win, hr, overlap, bool(cover))
    torch.cuda.synchronize()
    assert tuple(xc.shape) == (n + 1, 2, hr, hr) and bit_equal(xc[:n], x[dev(act).long()])
    if n > 1:
        small = torch.full((n, 2, hr, hr), 77.0, device="cuda")
        L_ = sifsr._lib
        L_.call("sifsrr_tiles_prepare", dev(lst), dev(ndvi), small, active, n_active, n - 1, h, w, win, hr, overlap, cover, M, SD,
                STATS["mean_ndvi"], STATS["std_ndvi"], 1, S())
        torch.cuda.synchronize()
        assert bit_equal(small[:n - 1], xc[:n - 1]) and (small[n - 1] == 77).all()


@pytest.mark.parametrize("win,h,w,overlap,cover", [(8, 20, 26, 2, 1), (64, 80, 100, 16, 1)])
def test_prepare_at_ratio_4_is_the_pipeline_s(sifsr, win, h, w, overlap, cover):
    lst, ndvi = rasters(win, h, w, 4, 1)
    want, tiles = sifsr.pipeline.granule_to_tiles(dev(lst), dev(ndvi), STATS, win, True, overlap, bool(cover))
    got, tiles2 = sifsr.ratio.granule_to_tiles(dev(lst), dev(ndvi), STATS, win, 4 * win, True, overlap, bool(cover))
    assert tiles == tiles2 and got.shape == want.shape
    err = float((got - want).abs().max())
    print(f"prepare at ({win},{4 * win}) against pipeline.granule_to_tiles: max|diff| = {err:.3e}")
    assert err <= 1e-5 * max(1.0, float(want.abs().max()))


# ---- 4. blend ----------------------------------------------------------------------------------------------------------------------
# rasters of 21 x 27, 38 x 46 and 27 x 33 LST pixels: multiples of q, and n - win a multiple of no stride used
BLENDS = [(8, 24, 21, 27, ov) for ov in (0, 2, 4)] + [(16, 40, 38, 46, ov) for ov in (0, 2, 8)] + [(12, 32, 27, 33, ov) for ov in (3, 6)] + \
         [(8, 32, 21, 27, 2)]


def _blend(sifsr, sr, shape, win, hr, stats, overlap, cover):
    out = sifsr.ratio.blend_tiles(torch.as_tensor(sr).float().contiguous().cuda(), shape, win, hr, stats, overlap, bool(cover))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("cover", [0, 1])
@pytest.mark.parametrize("win,hr,h,w,overlap", BLENDS)
def test_blend(sifsr, win, hr, h, w, overlap, cover):
    p, q, (ty, tx), (H, W) = R.geometry_ref((h, w), win, hr, overlap, cover)
    for n in (h, w):                                                   # both a ragged edge and a flush tile occur
        o = R.origins(n, win, overlap, 0)
        assert o[-1] + win < n
    # partition of unity on covered pixels, exact zeros on the others
    for c in (1.0, -2.75):
        sr = np.full((ty * tx, 1, hr, hr), c, dtype=np.float32)
        out = _blend(sifsr, sr, (h, w), win, hr, STATS, overlap, cover)
        _, m = R.blend_ref(sr, (h, w), win, hr, overlap, cover, 0.0, 1.0)
        want = float(np.float32(c)) * SD + M
        err = np.abs(out[m].astype(np.float64) - want).max() / abs(want)
        print(f"partition of unity ({win},{hr}) overlap {overlap} cover {cover} c {c}: max rel err {err:.3e}")
        assert out.shape == (H, W) and err <= 1e-6
        assert (out[~m] == 0).all() and (~m).any() == (cover == 0)
    # random tiles against the restatement, unit statistics
    rs = np.random.RandomState(100 * win + 10 * overlap + cover)
    sr = (rs.standard_normal((ty * tx, 1, hr, hr)) * 1.5).astype(np.float32)
    out1 = _blend(sifsr, sr, (h, w), win, hr, UNIT, overlap, cover)
    ref1, m = R.blend_ref(sr, (h, w), win, hr, overlap, cover, 0.0, 1.0)
    err1 = np.abs(out1 - ref1).max() / np.abs(ref1).max()
    print(f"restatement ({win},{hr}) overlap {overlap} cover {cover}: max|out - ref| / max|ref| = {err1:.3e}")
    assert err1 < 1e-5
    if cover:
        assert m.all()
    if hr == 4 * win:
        x4 = sifsr.pipeline.blend_tiles(dev(sr), (h, w), win, UNIT, overlap, bool(cover)).cpu().numpy()
        err4 = np.abs(out1 - x4).max() / np.abs(x4).max()
        print(f"  against pipeline.blend_tiles: {err4:.3e}")
        assert err4 < 1e-5


# ---- 5. masked blend ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill_value", [float("nan"), -9999.0])
@pytest.mark.parametrize("win,hr,h,w,overlap,cover", [(16, 40, 38, 46, 2, 1), (16, 40, 38, 46, 8, 0), (8, 24, 21, 27, 2, 1), (12, 32, 27, 33, 3, 1)])
def test_masked_blend(sifsr, win, hr, h, w, overlap, cover, fill_value):
    p, q, (ty, tx), (H, W) = R.geometry_ref((h, w), win, hr, overlap, cover)
    rs = np.random.RandomState(7 * win + overlap + cover)
    valid = holed_valid(rs, h, w, win)
    cy, cx = win + 1, 1                                                 # a single invalid cell among valid ones
    valid[win:win + 3, 0:3] = 1
    valid[cy, cx] = 0
    slot, active, n = GR.select_ref(valid, win, overlap, cover)
    T = ty * tx
    assert 0 < n < T
    sr_full = (rs.standard_normal((T, 1, hr, hr)) * 1.5).astype(np.float32)
    full = sifsr.ratio.blend_tiles(dev(sr_full), (h, w), win, hr, STATS, overlap, bool(cover)).cpu().numpy()
    out = sifsr.ratio.blend_active_tiles(dev(sr_full[active]), dev(slot), dev(valid), win, hr, STATS, overlap, bool(cover), fill_value)
    got = out.cpu().numpy()
    up = R.upsampled(valid, p, q)
    assert up.shape == (H, W) == got.shape and (~up).any()
    fill_bits = np.float32(fill_value).view(np.uint32)
    assert (bits(got)[~up] == fill_bits).all()                            # the fill, by its bits, exactly at the pixels of invalid cells
    assert np.array_equal(bits(got)[up], bits(full)[up])                  # the unmasked blend elsewhere, bit for bit
    rows, cols = np.nonzero(R.cell_of(H, p, q) == cy)[0], np.nonzero(R.cell_of(W, p, q) == cx)[0]
    assert (bits(got)[np.ix_(rows, cols)] == fill_bits).all()
    for Y in (rows[0] - 1, rows[-1] + 1):                                # the cells around it are valid: not one pixel more
        assert (bits(got)[Y, cols[0] - 1:cols[-1] + 2] != fill_bits).all()
    assert (bits(got)[rows[0] - 1:rows[-1] + 2, [cols[0] - 1, cols[-1] + 1]] != fill_bits).all()
    if (p, q) == (5, 2):                                                # HR pixels 2 and 3 of a row straddle cells 0 and 1
        assert list(R.cell_of(5, p, q)) == [0, 0, 0, 1, 1] and list(cols) == [3, 4]
        assert bits(got)[rows[0], 2] != fill_bits and bits(got)[rows[0], 3] == fill_bits
    ref, covered = R.blend_ref(sr_full[active], (h, w), win, hr, overlap, cover, M, SD, slot=slot, valid=valid, fill_value=fill_value)
    mk = up & covered
    assert (got[up & ~covered] == 0).all()
    err = np.abs(got[mk] - ref[mk]).max() / np.abs(ref[mk]).max()
    print(f"masked blend ({win},{hr}) overlap {overlap} cover {cover}: max|out - ref| / max|ref| = {err:.3e} at valid pixels")
    assert err < 1e-5
    # what the tiles hold at invalid pixels, and what skipped tiles predict, reaches no output bit
    oy, ox = R.origins(h, win, overlap, cover), R.origins(w, win, overlap, cover)
    sr2 = sr_full.copy()
    for a, y0 in enumerate(oy):
        for b, x0 in enumerate(ox):
            k = a * len(ox) + b
            if slot[k] < 0:
                sr2[k] = np.float32("nan")
            else:
                inv = ~up[y0 * p // q:y0 * p // q + hr, x0 * p // q:x0 * p // q + hr]
                sr2[k, 0][inv] = np.float32(1e30)
    compact = sr2[active]
    assert not np.array_equal(bits(compact), bits(sr_full[active]))
    out2 = sifsr.ratio.blend_active_tiles(dev(compact), dev(slot), dev(valid), win, hr, STATS, overlap, bool(cover), fill_value)
    assert bit_equal(out2, out)
    # a bool raster is the same mask
    out3 = sifsr.ratio.blend_active_tiles(dev(compact), dev(slot), dev(valid).bool(), win, hr, STATS, overlap, bool(cover), fill_value)
    assert bit_equal(out3, out)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(sifsr):
    return _model(sifsr, O.synthetic_state(3))


def oracle_tiles(sd, x64):
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    return torch.cat([O.modelb2_forward(sd, torch.from_numpy(x64[i:i + 1]), False) for i in range(x64.shape[0])]).numpy()


@pytest.mark.parametrize("win,hr,h,w,overlap,cover,batch", [(8, 24, 16, 24, 0, 0, 4), (16, 40, 32, 38, 2, 1, 5)])
def test_predict_granule(sifsr, model, win, hr, h, w, overlap, cover, batch):
    """the restatement's tiles through the float64 oracle in eval mode, blended by the restatement; held at rel_err < 1e-4
    de-normalised and on the network's own scale, as test_mosaic_gpu.test_predict_granule_overlapped holds the x4 call"""
    p, q, (ty, tx), (H, W) = R.geometry_ref((h, w), win, hr, overlap, cover)
    lst, ndvi = rasters(hr, h, w, p, q)
    y64 = oracle_tiles(copy.deepcopy(O.synthetic_state(3)), R.prepare_ref(lst, ndvi, STATS, win, hr, overlap, cover, True))
    ref, m = R.blend_ref(y64, (h, w), win, hr, overlap, cover, M, SD)
    ref_n, _ = R.blend_ref(y64, (h, w), win, hr, overlap, cover, 0.0, 1.0)
    assert m.all()
    out = sifsr.ratio.predict_granule(model, dev(lst), dev(ndvi), STATS, window=win, hr=hr, batch=batch, overlap=overlap, cover_edges=bool(cover))
    assert tuple(out.shape) == (H, W) and out.dtype == torch.float32 and ty * tx > batch
    e_abs = rel_err(out.cpu(), torch.from_numpy(ref))
    e_norm = normalised_per_image_err(out.cpu()[None], torch.from_numpy(ref_n)[None], M, SD)
    print(f"end to end ({win},{hr}) {h}x{w}: rel_err {e_abs:.3e}, normalised per-image err {float(e_norm.max()):.3e}")
    assert e_abs < 1e-4
    assert float(e_norm.max()) < 1e-4
    # the batch size is plumbing
    assert bit_equal(sifsr.ratio.predict_granule(model, dev(lst), dev(ndvi), STATS, window=win, hr=hr, batch=256, overlap=overlap,
                                                 cover_edges=bool(cover)), out)


def gappy_24x32():
    lst, ndvi = rasters(11, 24, 32, 3, 1)
    lst[:8, :8] = 0.0                                                   # tile (0, 0) of window 8 is all gap
    for y, x in ((9, 3), (15, 20), (23, 31), (10, 10), (0, 30)):
        lst[y, x] = 0.0
    lst[20, 5] = np.float32("nan")
    return lst, ndvi


def test_predict_granule_gaps(sifsr, model):
    lst, ndvi = gappy_24x32()
    kw = dict(window=8, hr=24, batch=7, overlap=2, cover_edges=True)
    filled_np, valid = GR.fill_ref(lst)
    out, info = sifsr.ratio.predict_granule_gaps(model, dev(lst), dev(ndvi), STATS, return_info=True, **kw)
    want = sifsr.ratio.predict_granule(model, dev(filled_np), dev(ndvi), STATS, **kw)
    got, want = out.cpu().numpy(), want.cpu().numpy()
    up = R.upsampled(valid, 3, 1)
    assert got.shape == (72, 96) and got.dtype == np.float32
    assert np.isnan(got[~up]).all() and not np.isnan(got[up]).any() and (~up).any()          # NaN exactly at the pixels of invalid cells
    assert np.array_equal(bits(got)[up], bits(want)[up])
    n_ref = GR.select_ref(valid, 8, 2, 1)[2]
    assert info["n_active"] == n_ref < info["n_tiles"] == ntiles(24, 32, 8, 24, 2, 1)
    assert info["valid"].dtype == torch.bool and np.array_equal(info["valid"].cpu().numpy(), valid != 0)
    print(f"gaps: {info['n_active']} of {info['n_tiles']} tiles active")
    # a mask does what a 0 K pixel does; another fill value
    lst2 = np.where(valid != 0, lst, np.float32(333.0)).astype(np.float32)
    out2 = sifsr.ratio.predict_granule_gaps(model, dev(lst2), dev(ndvi), STATS, mask=dev((valid != 0).astype(np.uint8)), **kw)
    assert bit_equal(out2, out)
    out3 = sifsr.ratio.predict_granule_gaps(model, dev(lst), dev(ndvi), STATS, fill_value=-9999.0, **kw).cpu().numpy()
    assert np.array_equal(bits(out3)[up], bits(got)[up]) and (out3[~up] == -9999.0).all()


def test_nothing_valid_runs_no_forward(sifsr):
    class NoForward(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("a forward ran on a granule without a valid pixel")
    lst, ndvi = np.zeros((24, 32), np.float32), rasters(3, 24, 32, 3, 1)[1]
    out, info = sifsr.ratio.predict_granule_gaps(NoForward(), dev(lst), dev(ndvi), STATS, window=8, hr=24, overlap=2, return_info=True)
    assert tuple(out.shape) == (72, 96) and torch.isnan(out).all()
    assert info["n_active"] == 0 and info["n_tiles"] == ntiles(24, 32, 8, 24, 2, 1) and not bool(info["valid"].any())
    out = sifsr.ratio.predict_granule_gaps(NoForward(), dev(lst), dev(ndvi), STATS, window=8, hr=24, overlap=2, fill_value=-1.0)
    assert (out == -1.0).all()


# ---- 7. training at x3 -------------------------------------------------------------------------------------------------------------
def test_train_step_fed_by_the_resampler(sifsr):
    """one sensor.train_step at batch 2, 24 -> 72, with lst_up from ratio.upsample, beside the same step from the same initial
    weights with torch's F.interpolate: the inputs differ by torch's fp32 coordinate rounding only, the three losses agree to 1e-4"""
    rs = np.random.RandomState(31)
    lst = dev(rs.standard_normal((2, 1, 24, 24)).astype(np.float32))
    ndvi = dev(rs.standard_normal((2, 1, 72, 72)).astype(np.float32))
    assert sifsr.sensor.lr_shape(72, 72, 3.0) == (24, 24)
    ups = {"ratio": sifsr.ratio.upsample(lst, (72, 72)),
           "torch": F.interpolate(lst, size=(72, 72), mode="bicubic", align_corners=False).contiguous()}
    assert tuple(ups["ratio"].shape) == (2, 1, 72, 72)
    d = float((ups["ratio"] - ups["torch"]).abs().max())
    print(f"lst_up: max|ratio.upsample - F.interpolate| = {d:.3e}")
    assert d <= 1e-5 * max(1.0, float(ups["torch"].abs().max()))
    losses = {}
    for name, up in ups.items():
        m = make_model(sifsr, O.synthetic_state(71))
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
        p0 = m.flat_parameters().detach().clone()
        losses[name] = [float(v) for v in sifsr.sensor.train_step(m, opt, lst, up, ndvi, STATS, 0.5, -0.25, 3.0)]
        assert not torch.equal(m.flat_parameters(), p0) and all(np.isfinite(losses[name]))
    print(f"losses (ds, percep, loss): ratio {losses['ratio']}, torch {losses['torch']}")
    for a, b in zip(losses["ratio"], losses["torch"]):
        assert abs(a - b) <= 1e-4 * abs(b)


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(sifsr, L, model):
    h, w, win, hr, ov = 20, 26, 8, 24, 2
    lst, ndvi = rasters(1, h, w, 3, 1)
    lst_c, ndvi_c = dev(lst), dev(ndvi)
    E, Q = sifsr.SifsrError, sifsr.ratio
    T = ntiles(h, w, win, hr, ov, 1)
    # Python: bad geometry and bad tensors, before any launch
    bad = [dict(window=8, hr=28), dict(window=8, hr=16), dict(window=24, hr=24), dict(window=1, hr=24), dict(window=65, hr=256),
           dict(window=8, hr=24, overlap=5), dict(window=8, hr=24, overlap=-1), dict(window=32, hr=96),      # raster smaller than a window
           dict(window=8, hr=24, ndvi=ndvi_c[:, :77].contiguous()), dict(window=8, hr=24, ndvi=ndvi_c[:59].contiguous()),
           dict(window=8, hr=24, lst=lst_c.double()), dict(window=8, hr=24, lst=lst_c[None])]
    for kw in bad:
        kw = dict(kw)
        a, b = kw.pop("lst", lst_c), kw.pop("ndvi", ndvi_c)
        with pytest.raises(E):
            Q.granule_to_tiles(a, b, STATS, kw.pop("window"), kw.pop("hr"), **kw)
    for kw in bad[:10]:
        kw = dict(kw)
        b = kw.pop("ndvi", ndvi_c)
        with pytest.raises(E):
            Q.predict_granule(model, lst_c, b, STATS, **kw)
        with pytest.raises(E):
            Q.predict_granule_gaps(model, lst_c, b, STATS, **{"overlap": 0, **kw})
    l40, n40 = rasters(2, 38, 46, 5, 2)
    for kw in (dict(overlap=1), dict(overlap=3, cover_edges=True)):                          # overlap % q != 0
        with pytest.raises(E):
            Q.predict_granule(model, dev(l40), dev(n40), STATS, window=16, hr=40, **kw)
    with pytest.raises(E):
        Q.predict_granule(model, dev(l40[:37].copy()), dev(n40), STATS, window=16, hr=40)    # lst_h % q != 0
    with pytest.raises(E, match="multiple of 4"):
        Q.predict_granule_gaps(model, dev(rasters(3, 18, 18, 4, 1)[0]), dev(rasters(3, 18, 18, 4, 1)[1]), STATS, window=6, hr=24, overlap=0)
    for kw in (dict(batch=0),):
        with pytest.raises(E):
            Q.predict_granule(model, lst_c, ndvi_c, STATS, window=8, hr=24, **kw)
        with pytest.raises(E):
            Q.predict_granule_gaps(model, lst_c, ndvi_c, STATS, window=8, hr=24, overlap=2, **kw)
    sr = torch.zeros((T, 1, hr, hr), device="cuda")
    with pytest.raises(E):
        Q.blend_tiles(sr[:T - 1], (h, w), win, hr, STATS, ov, True)                          # not this layout's tile count
    with pytest.raises(E):
        Q.blend_tiles(sr, (h, w), win, hr, STATS, ov, True, out=torch.zeros((60, 77), device="cuda"))
    with pytest.raises(E):
        Q.blend_tiles(sr.cpu(), (h, w), win, hr, STATS, ov, True)
    for x, size in ((lst_c, (19, 78)), (lst_c, (60, 25)), (lst_c, (60,)), (lst_c.double(), (60, 78)), (lst_c[None, None, None], (60, 78)),
                    (lst_c.cpu(), (60, 78))):
        with pytest.raises(E):
            Q.upsample(x, size)
    with pytest.raises(E):
        Q.prepare_tiles(lst_c[None, None, :8, :8].contiguous(), ndvi_c[None, None, :28, :28].contiguous())
    # the C entry points: 1001 / 1002 and nothing launched (the poisoned outputs keep every bit)
    lib = L.lib()
    p_ = lambda t: t.data_ptr()
    x = torch.full((T, 2, hr, hr), 77.0, device="cuda")
    out = torch.full((60, 78), 77.0, device="cuda")
    up = torch.full((2, 60, 78), 77.0, device="cuda")
    valid = torch.ones((h, w), dtype=U8, device="cuda")
    slot = torch.arange(T, dtype=I32, device="cuda")
    active, one = slot.clone(), torch.ones((1,), dtype=I32, device="cuda")
    for hh, ww, wn, hrr, o in ((20, 26, 8, 28, 0), (20, 26, 8, 16, 0), (20, 26, 24, 24, 0), (20, 26, 0, 24, 0), (130, 130, 65, 256, 0),
                               (20, 26, 8, 264, 0), (20, 26, 1, 24, 0), (20, 26, 8, 24, 5), (20, 26, 8, 24, -1), (7, 26, 8, 24, 0),
                               (20, 7, 8, 24, 0), (37, 46, 16, 40, 0), (38, 45, 16, 40, 0), (38, 46, 16, 40, 1), (16385, 26, 8, 24, 0)):
        for cover in (0, 1):
            args = (hh, ww, wn, hrr, o, cover)
            assert lib.sifsrr_tiles_prepare(p_(lst_c), p_(ndvi_c), p_(x), None, None, T, *args, 307.0, 5.5, 0.6, 0.2, 1, S()) == SHAPE_ERR
            assert lib.sifsrr_tiles_prepare(p_(lst_c), p_(ndvi_c), p_(x), p_(active), p_(one), T, *args, 307.0, 5.5, 0.6, 0.2, 1, S()) == SHAPE_ERR
            assert lib.sifsrr_tiles_blend(p_(sr), None, None, p_(out), *args, 307.0, 5.5, -1.0, S()) == SHAPE_ERR
            assert lib.sifsrr_tiles_blend(p_(sr), p_(slot), p_(valid), p_(out), *args, 307.0, 5.5, -1.0, S()) == SHAPE_ERR
    g = (h, w, win, hr, ov, 1)
    for stds in ((0.0, 0.2), (5.5, 0.0)):                                # std == 0
        assert lib.sifsrr_tiles_prepare(p_(lst_c), p_(ndvi_c), p_(x), None, None, T, *g, 307.0, stds[0], 0.6, stds[1], 1, S()) == SHAPE_ERR
    for cap in (0, -3):                                                 # cap < 1
        assert lib.sifsrr_tiles_prepare(p_(lst_c), p_(ndvi_c), p_(x), p_(active), p_(one), cap, *g, 307.0, 5.5, 0.6, 0.2, 1, S()) == SHAPE_ERR
        with pytest.raises(E):
            Q.prepare_active_tiles(lst_c, ndvi_c, STATS, active, one, cap, win, hr, ov, True)
    for i in range(3):                                                  # null pointers
        a = [p_(lst_c), p_(ndvi_c), p_(x)]
        a[i] = None
        assert lib.sifsrr_tiles_prepare(*a, None, None, T, *g, 307.0, 5.5, 0.6, 0.2, 1, S()) == ARG_ERR
    assert lib.sifsrr_tiles_prepare(p_(lst_c), p_(ndvi_c), p_(x), p_(active), None, T, *g, 307.0, 5.5, 0.6, 0.2, 1, S()) == ARG_ERR
    assert lib.sifsrr_tiles_prepare(p_(lst_c), p_(ndvi_c), p_(x), None, p_(one), T, *g, 307.0, 5.5, 0.6, 0.2, 1, S()) == ARG_ERR
    assert lib.sifsrr_tiles_blend(None, None, None, p_(out), *g, 307.0, 5.5, -1.0, S()) == ARG_ERR
    assert lib.sifsrr_tiles_blend(p_(sr), None, None, None, *g, 307.0, 5.5, -1.0, S()) == ARG_ERR
    assert lib.sifsrr_tiles_blend(p_(sr), p_(slot), None, p_(out), *g, 307.0, 5.5, -1.0, S()) == ARG_ERR
    assert lib.sifsrr_tiles_blend(p_(sr), None, p_(valid), p_(out), *g, 307.0, 5.5, -1.0, S()) == ARG_ERR
    assert lib.sifsrr_upsample(None, p_(up), 2, 20, 26, 60, 78, S()) == ARG_ERR
    assert lib.sifsrr_upsample(p_(lst_c), None, 1, 20, 26, 60, 78, S()) == ARG_ERR
    for B, a, b, A_, B_ in ((0, 20, 26, 60, 78), (65536, 20, 26, 60, 78), (1, 0, 26, 60, 78), (1, 20, 0, 60, 78), (1, 20, 26, 19, 78),
                            (1, 20, 26, 60, 25), (1, 16385, 26, 16385, 78), (1, 20, 26, 32769, 78), (1, 20, 26, 60, 32769)):
        assert lib.sifsrr_upsample(p_(lst_c), p_(up), B, a, b, A_, B_, S()) == SHAPE_ERR
    torch.cuda.synchronize()
    for t in (x, out, up):
        assert (t == 77).all()
