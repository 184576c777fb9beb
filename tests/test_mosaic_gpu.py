"""GPU: seamless whole-granule prediction (include/sifsr_mosaic.h) -- tiles laid with an overlap and a last tile
flush to each raster edge, merged by a normalised feathered blend on the device.

  * the memory contract of the two writing entry points, in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is
    the table tests/test_capi_gate.py checks against the header),
  * the defaults reproduce the non-overlapping path bit for bit,
  * every tile's network input is bit-identical to the existing kernel's for the same block,
  * the blend alone against its formula (partition of unity, continuity, a float64 NumPy restatement, coverage),
  * the whole granule against a restatement built from the oracle, at the project's 1e-4 bar,
  * GranulePredictor (one hipGraph per granule shape) against the eager call, and the argument errors."""
import copy

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests.conftest import rel_err
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal
from tests.test_model_gpu import normalised_per_image_err

pytestmark = pytest.mark.gpu
STATS = {"mean_lst": 307.2378, "std_lst": 5.5698, "mean_ndvi": 0.6452, "std_ndvi": 0.1683}
UNIT = {"mean_lst": 0.0, "std_lst": 1.0, "mean_ndvi": 0.0, "std_ndvi": 1.0}
SHAPE_ERR = 1001


def origins(n, win, overlap, cover):
    """the layout, restated here (tests/test_mosaic_host.py pins sifsr.pipeline.tile_origins and the library against it too)"""
    o = list(range(0, n - win + 1, win - overlap))
    if cover and o[-1] + win < n:
        o.append(n - win)
    return o


def blend_ref(sr, lst_shape, win, overlap, cover, mean, std):
    """float64 restatement of the blend of include/sifsr_mosaic.h: sr (T,1,4win,4win) -> (out (4h,4w), covered mask)."""
    h, w = lst_shape
    W, R = 4 * win, 4 * overlap
    q = np.arange(W, dtype=np.float64)
    t = np.ones(W) if R == 0 else np.minimum(1.0, np.minimum((q + 0.5) / R, (W - q - 0.5) / R))
    wgt = t[:, None] * t[None, :]
    oy, ox = origins(h, win, overlap, cover), origins(w, win, overlap, cover)
    sr = np.asarray(sr, dtype=np.float64)
    assert sr.shape == (len(oy) * len(ox), 1, W, W)
    num, den = np.zeros((4 * h, 4 * w)), np.zeros((4 * h, 4 * w))
    for a, y0 in enumerate(oy):
        for b, x0 in enumerate(ox):
            num[4 * y0:4 * y0 + W, 4 * x0:4 * x0 + W] += wgt * sr[a * len(ox) + b, 0]
            den[4 * y0:4 * y0 + W, 4 * x0:4 * x0 + W] += wgt
    m = den > 0
    out = np.zeros_like(num)
    out[m] = num[m] / den[m] * std + mean
    return out, m


# (win, overlap, cover, lst_h, lst_w): cover 0 and 1, overlap 0, 8 and win/2, win 16 and 64; rasters that are not multiples of the
# stride (37 x 50, 45 x 61, 150 x 100, 100 x 70), one that is (40 x 48 at stride 8) and a single tile
LAYOUTS = [(16, 0, 0, 37, 50), (16, 0, 1, 37, 50), (16, 8, 0, 45, 61), (16, 8, 1, 45, 61), (16, 8, 1, 40, 48), (16, 8, 1, 16, 16),
           (64, 32, 1, 150, 100), (64, 32, 0, 150, 100), (64, 8, 1, 130, 64), (64, 0, 1, 100, 70)]


# ---- 1. memory contract ----------------------------------------------------------------------------------------------------
def tiles_prepare():
    def make(win, overlap, cover, h, w):
        def case(k):
            T, hr = len(origins(h, win, overlap, cover)) * len(origins(w, win, overlap, cover)), 4 * win
            lst, ndvi = k.i("lst", h, w, scale=5.0, shift=300.0), k.i("ndvi", 4 * h, 4 * w, scale=0.5)
            x = k.o("x", T, 2, hr, hr)
            call = lambda: k.L.call("sifsrx_tiles_prepare", lst, ndvi, x, h, w, win, overlap, cover, 307.2378, 5.5698, 0.3, 0.2,
                                    1, S())
            return call, {"x": x}
        return case
    return [make(*c) for c in LAYOUTS]


def tiles_blend():
    def make(win, overlap, cover, h, w):
        def case(k):
            T, hr = len(origins(h, win, overlap, cover)) * len(origins(w, win, overlap, cover)), 4 * win
            sr = k.i("sr", T, 1, hr, hr)
            out = k.o("out", 4 * h, 4 * w)              # EVERY element is the call's to write, the uncovered band included
            call = lambda: k.L.call("sifsrx_tiles_blend", sr, out, h, w, win, overlap, cover, 307.2378, 5.5698, S())
            return call, {"out": out}
        return case
    return [make(*c) for c in LAYOUTS]


CONTRACT = {"sifsrx_tiles_prepare": tiles_prepare(), "sifsrx_tiles_blend": tiles_blend()}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """x / out fully written (NaN-free under the NaN poison, bit-identical under every poison), inputs untouched, nothing outside
    the buffers written, and the same bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx)


# ---- 2. defaults unchanged -----------------------------------------------------------------------------------------------
def _granule(seed=9, h=200, w=136):
    rs = np.random.RandomState(seed)
    lst_g = torch.from_numpy((rs.standard_normal((h, w)) * 5.5 + 307).astype(np.float32))
    ndvi_g = torch.from_numpy((rs.standard_normal((4 * h, 4 * w)) * 0.6 + 0.5).astype(np.float32))
    return lst_g, ndvi_g


def _model(sifsr, sd):
    m = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def test_defaults_unchanged(sifsr):
    lst_g, ndvi_g = _granule()
    m = _model(sifsr, O.synthetic_state(3))
    a = sifsr.predict.predict_granule(m, lst_g.cuda(), ndvi_g.cuda(), STATS, batch=4)
    b = sifsr.predict.predict_granule(m, lst_g.cuda(), ndvi_g.cuda(), STATS, batch=4, overlap=0, cover_edges=False)
    assert bit_equal(a, b)
    assert a[4 * 192:, :].abs().max().item() == 0 and a[:, 4 * 128:].abs().max().item() == 0      # still the reference's zeros
    x0, t0 = sifsr.pipeline.granule_to_tiles(lst_g.cuda(), ndvi_g.cuda(), STATS)
    x1, t1 = sifsr.pipeline.granule_to_tiles(lst_g.cuda(), ndvi_g.cuda(), STATS, overlap=0, cover_edges=False)
    assert t0 == t1 == (3, 2) and bit_equal(x0, x1)
    # the defaults ARE the old entry points: what they give is what the new kernels give for the same layout
    xs = torch.empty_like(x0)
    sifsr._lib.call("sifsrx_tiles_prepare", lst_g.cuda(), ndvi_g.cuda(), xs, 200, 136, 64, 0, 0, STATS["mean_lst"], STATS["std_lst"],
                    STATS["mean_ndvi"], STATS["std_ndvi"], 1, S())
    assert bit_equal(xs, x0)


# ---- 3. prepare parity ---------------------------------------------------------------------------------------------------
def test_prepare_parity(sifsr):
    """overlap 16, covering: tile t of x is bit-equal to the existing kernel applied to the same 64 x 64 block sliced on the host,
    and within the bar of test_prepare_tiles (1e-5) of the oracle."""
    lst_g, ndvi_g = _granule()
    x, (ty, tx) = sifsr.pipeline.granule_to_tiles(lst_g.cuda(), ndvi_g.cuda(), STATS, overlap=16, cover_edges=True)
    oy, ox = origins(200, 64, 16, True), origins(136, 64, 16, True)
    assert (ty, tx) == (len(oy), len(ox)) == (4, 3) and oy[-1] == 136 and ox[-1] == 72
    lb = torch.stack([lst_g[i:i + 64, j:j + 64] for i in oy for j in ox])[:, None].contiguous()
    nb = torch.stack([ndvi_g[4 * i:4 * i + 256, 4 * j:4 * j + 256] for i in oy for j in ox])[:, None].contiguous()
    same = sifsr.pipeline.prepare_tiles(lb.cuda(), nb.cuda(), STATS, True)
    assert x.shape == same.shape == (12, 2, 256, 256)
    for t in range(12):
        assert bit_equal(x[t], same[t]), t
    ref = O.prepare_tiles(lb, nb, STATS, True)
    assert (x.cpu() - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


# ---- 4. the blend alone --------------------------------------------------------------------------------------------------
def _blend(sifsr, sr, shape, win, stats, overlap, cover):
    out = sifsr.pipeline.blend_tiles(torch.as_tensor(sr).float().contiguous().cuda(), shape, win, stats, overlap, bool(cover))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ntiles(win, overlap, cover, h, w):
    return len(origins(h, win, overlap, cover)), len(origins(w, win, overlap, cover))


@pytest.mark.parametrize("win,overlap,cover,h,w", LAYOUTS)
def test_blend_partition_of_unity(sifsr, win, overlap, cover, h, w):
    """all tiles equal c: out == c*std + mean to 1e-6 relative wherever a tile covers, whatever the weights sum to"""
    ty, tx = _ntiles(win, overlap, cover, h, w)
    for c in (0.0, 1.0, -2.75, 3.3):
        sr = np.full((ty * tx, 1, 4 * win, 4 * win), c, dtype=np.float32)
        out = _blend(sifsr, sr, (h, w), win, STATS, overlap, cover)
        _, m = blend_ref(sr, (h, w), win, overlap, cover, 0.0, 1.0)
        want = float(np.float32(c)) * STATS["std_lst"] + STATS["mean_lst"]
        err = np.abs(out[m].astype(np.float64) - want).max() / abs(want)
        print(f"partition of unity win {win} overlap {overlap} cover {cover} {h}x{w} c {c}: max rel err {err:.3e}")
        assert err <= 1e-6
        assert (out[~m] == 0).all()


# Rasters for the continuity bound.  The bound leaves 1e-5 of one weight step, Delta*std/(R*1e5), for rounding -- below the fp32
# spacing of the blended values themselves (tile constants 0..T-1 with steps of 1/R) unless the arithmetic is EXACT.  It is
# exact where every quantity is a dyadic rational of < 24 bits: mean 0, std 1, R a power of two, and weights that sum to 1 (two
# regular neighbours) or belong to one tile (num / den = (w v) / w, correctly rounded division) -- the first group: rasters of
# length win + m*stride, tiled by regular tiles alone, in two dimensions.  Where the flush tile overlaps its ONE neighbour by more
# than `overlap` the weights sum to >= 1 + 4/R and the normalised step is smaller than 1/R by that factor (>= 3 % for R <= 128,
# against ~1e-4 of fp32 rounding): the second group, one tile row / column with a flush tile.  Left to the float64 restatement
# below: zones of three tiles along an axis (the flush tile entering while two regular ones cross-fade: the formula itself steps
# by more than Delta/R there) and two-dimensional rasters with a flush tile (the quotient by a non-dyadic weight sum rounds at
# the values' own spacing, in a direction whose step has no margin).
CONTINUITY = [(16, 8, 40, 48), (64, 32, 128, 160), (64, 16, 160, 112), (16, 4, 28, 40),
              (64, 16, 64, 150), (64, 16, 150, 64), (16, 4, 16, 45), (16, 4, 45, 16)]


@pytest.mark.parametrize("cover", [0, 1])
@pytest.mark.parametrize("win,overlap,h,w", CONTINUITY)
def test_blend_continuity(sifsr, win, overlap, h, w, cover):
    """tile k holds the constant k: between adjacent output pixels the blend steps by at most |Delta| * std / R * (1 + 1e-5),
    Delta = the difference between the constants of neighbouring tiles along that axis (1 along x, tiles_x along y)."""
    ty, tx = _ntiles(win, overlap, cover, h, w)
    for axis_n in (h, w):                               # no zone of three tiles along an axis (see CONTINUITY)
        o = origins(axis_n, win, overlap, cover)
        assert all(o[i + 2] >= o[i] + win for i in range(len(o) - 2)), o
    R, std = 4 * overlap, 1.0
    assert R & (R - 1) == 0
    sr = np.broadcast_to(np.arange(ty * tx, dtype=np.float32)[:, None, None, None], (ty * tx, 1, 4 * win, 4 * win))
    out = _blend(sifsr, np.ascontiguousarray(sr), (h, w), win, UNIT, overlap, cover).astype(np.float64)
    _, m = blend_ref(sr, (h, w), win, overlap, cover, 0.0, 1.0)
    jx = np.abs(np.diff(out, axis=1))[m[:, 1:] & m[:, :-1]].max()
    jy = np.abs(np.diff(out, axis=0))[m[1:] & m[:-1]].max()
    print(f"continuity win {win} overlap {overlap} cover {cover} {h}x{w}: x step {jx * R:.9f} (bound 1), "
          f"y step {jy * R / tx:.9f} (bound 1), in units of Delta*std/R")
    assert jx <= 1 * std / R * (1 + 1e-5)
    assert jy <= tx * std / R * (1 + 1e-5)
    if tx > 1:
        assert jx >= 0.99 * std / R                     # (the tiles ARE blended: a paste would step by a whole Delta)


@pytest.mark.parametrize("win,overlap,cover,h,w", LAYOUTS + [(64, 16, 1, 200, 136), (64, 16, 0, 200, 136)])
def test_blend_restatement_and_coverage(sifsr, win, overlap, cover, h, w):
    """within 1e-5 * max|out| of the float64 restatement (fp32 rounding of a weighted sum of at most 9 terms and its quotient: the
    bar of test_prepare_tiles); the band no tile covers is exactly 0, and with cover_edges no pixel is."""
    ty, tx = _ntiles(win, overlap, cover, h, w)
    rs = np.random.RandomState(100 * win + 10 * overlap + cover)
    sr = rs.standard_normal((ty * tx, 1, 4 * win, 4 * win)).astype(np.float32) * 1.5
    out = _blend(sifsr, sr, (h, w), win, STATS, overlap, cover)
    ref, m = blend_ref(sr, (h, w), win, overlap, cover, STATS["mean_lst"], STATS["std_lst"])
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"restatement win {win} overlap {overlap} cover {cover} {h}x{w}: max|out - ref| / max|ref| = {err:.3e}")
    assert err < 1e-5
    if cover:
        assert m.all() and (out != 0).all()
    else:
        ey, ex = origins(h, win, overlap, 0)[-1] + win, origins(w, win, overlap, 0)[-1] + win
        assert m[:4 * ey, :4 * ex].all() and not m[4 * ey:].any() and not m[:, 4 * ex:].any()
        assert (out[4 * ey:] == 0).all() and (out[:, 4 * ex:] == 0).all() and (out[:4 * ey, :4 * ex] != 0).all()
    # on the network's own scale too (mean 0 / std 1), where the bar is not diluted by the 307 K offset
    out1 = _blend(sifsr, sr, (h, w), win, UNIT, overlap, cover)
    ref1, _ = blend_ref(sr, (h, w), win, overlap, cover, 0.0, 1.0)
    err1 = np.abs(out1 - ref1).max() / np.abs(ref1).max()
    print(f"  normalised scale: {err1:.3e}")
    assert err1 < 1e-5


# ---- 5. end to end -------------------------------------------------------------------------------------------------------
def _oracle_tiles(sd, lst_g, ndvi_g, dtype):
    oy, ox = origins(200, 64, 16, True), origins(136, 64, 16, True)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    ys = []
    for i in oy:
        for j in ox:
            x = O.prepare_tiles(lst_g[i:i + 64, j:j + 64][None, None].to(dtype), ndvi_g[4 * i:4 * i + 256, 4 * j:4 * j + 256][None, None].to(dtype),
                                STATS, clip_ndvi=True)
            ys.append((O.predict_tiles(sd, x[:, 0:1], x[:, 1:2], STATS["mean_lst"], STATS["std_lst"]) - STATS["mean_lst"]) / STATS["std_lst"])
    return torch.cat(ys).numpy()


def test_predict_granule_overlapped(sifsr):
    """200 x 136 granule, overlap 16, covering: 4 x 3 tiles.  Restatement: the float64 oracle per block (O.prepare_tiles,
    O.predict_tiles), blended in float64 NumPy; held at normalised_per_image_err < 1e-4 on the network's scale and rel_err < 1e-4
    de-normalised.  (The float32 oracle meets the same bar against the float64 one for these 12 tiles and their blend: on the
    CPU, 1.9e-6 per tile and 1.8e-6 for the blended raster on the network's scale, 1.4e-6 de-normalised -- the restatement's own
    precision is far inside the bar it sets.)"""
    lst_g, ndvi_g = _granule()
    sd = O.synthetic_state(3)
    y64 = _oracle_tiles(copy.deepcopy(sd), lst_g, ndvi_g, torch.float64)
    ref, m = blend_ref(y64, (200, 136), 64, 16, True, STATS["mean_lst"], STATS["std_lst"])
    ref_n, _ = blend_ref(y64, (200, 136), 64, 16, True, 0.0, 1.0)
    assert m.all()
    out = sifsr.predict.predict_granule(_model(sifsr, sd), lst_g.cuda(), ndvi_g.cuda(), STATS, batch=5, overlap=16, cover_edges=True)
    assert tuple(out.shape) == (800, 544) and (out != 0).all()
    e_abs = rel_err(out.cpu(), torch.from_numpy(ref))
    e_norm = normalised_per_image_err(out.cpu()[None], torch.from_numpy(ref_n)[None], STATS["mean_lst"], STATS["std_lst"])
    print(f"end to end: rel_err {e_abs:.3e}, normalised per-image err {float(e_norm.max()):.3e}")
    assert e_abs < 1e-4
    assert float(e_norm.max()) < 1e-4, e_norm
    # the seams are gone: across the first tile border of the non-overlapping mosaic (column 256) the overlapped raster steps no
    # more than it does one pixel further in -- not asserted as a number, the blend's continuity is pinned above


# ---- 6. GranulePredictor -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap,cover,batch", [(16, True, 5), (0, False, 4), (0, True, 256)])
def test_granule_predictor(sifsr, overlap, cover, batch):
    lst_g, ndvi_g = _granule()
    m = _model(sifsr, O.synthetic_state(3))
    eager = sifsr.predict.predict_granule(m, lst_g.cuda(), ndvi_g.cuda(), STATS, batch=batch, overlap=overlap, cover_edges=cover)
    gp = sifsr.predict.GranulePredictor(m, (200, 136), STATS, window=64, overlap=overlap, cover_edges=cover, batch=batch)
    for _ in range(2):
        assert bit_equal(gp(lst_g.cuda(), ndvi_g.cuda()), eager)
    lst2, ndvi2 = _granule(seed=31)                       # other rasters through the same graph: inputs are not baked in
    eager2 = sifsr.predict.predict_granule(m, lst2.cuda(), ndvi2.cuda(), STATS, batch=batch, overlap=overlap, cover_edges=cover)
    assert not bit_equal(eager2, eager)
    assert bit_equal(gp(lst2.cuda(), ndvi2.cuda()), eager2)
    assert bit_equal(gp(lst_g.cuda(), ndvi_g.cuda()), eager)
    with pytest.raises(ValueError):
        gp(lst_g[:, :128].contiguous().cuda(), ndvi_g[:, :512].contiguous().cuda())
    with pytest.raises(ValueError):
        gp(lst_g.cuda(), ndvi_g[:796].contiguous().cuda())


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_errors(sifsr, L):
    lst_g, ndvi_g = _granule()
    lst_c, ndvi_c = lst_g.cuda(), ndvi_g.cuda()
    m = _model(sifsr, O.synthetic_state(3))
    E = sifsr.SifsrError
    bad = [dict(overlap=-1), dict(overlap=33), dict(overlap=9, window=16), dict(window=128, overlap=8), dict(window=68, cover_edges=True),
           dict(window=64, overlap=16, lst=lst_c[:40].contiguous(), ndvi=ndvi_c[:160].contiguous()),      # raster smaller than a window
           dict(overlap=16, ndvi=ndvi_c[:, :540].contiguous()), dict(cover_edges=True, ndvi=ndvi_c[:796].contiguous())]
    for kw in bad:
        kw = dict(kw)
        a, b = kw.pop("lst", lst_c), kw.pop("ndvi", ndvi_c)
        with pytest.raises(E):
            sifsr.pipeline.granule_to_tiles(a, b, STATS, **kw)
        with pytest.raises(E):
            sifsr.predict.predict_granule(m, a, b, STATS, **kw)
        if tuple(b.shape) == (4 * a.shape[0], 4 * a.shape[1]):          # (the predictor takes the LST shape alone)
            with pytest.raises(E):
                sifsr.predict.GranulePredictor(m, tuple(a.shape), STATS, **kw)
    sr = torch.zeros((12, 1, 256, 256), device="cuda")
    for kw in (dict(overlap=-1, cover_edges=True), dict(overlap=33, cover_edges=True)):
        with pytest.raises(E):
            sifsr.pipeline.blend_tiles(sr, (200, 136), 64, STATS, **kw)
    with pytest.raises(E):
        sifsr.pipeline.blend_tiles(sr[:11], (200, 136), 64, STATS, 16, True)              # not this layout's tile count
    with pytest.raises(E):
        sifsr.pipeline.blend_tiles(sr, (40, 136), 64, STATS, 16, True)
    # the C entry points: SHAPE for the same cases, nothing launched (the poisoned outputs keep every bit)
    x = torch.full((12, 2, 256, 256), float("nan"), device="cuda")
    out = torch.full((800, 544), float("nan"), device="cuda")
    fn_p, fn_b = getattr(L.lib(), "sifsrx_tiles_prepare"), getattr(L.lib(), "sifsrx_tiles_blend")
    for h, w, win, ov in ((200, 136, 64, -1), (200, 136, 64, 33), (200, 136, 128, 8), (200, 136, 16, 9), (40, 136, 64, 16),
                          (200, 63, 64, 0), (200, 136, 62, 0), (200, 136, 0, 0)):
        for cover in (0, 1):
            assert fn_p(lst_c.data_ptr(), ndvi_c.data_ptr(), x.data_ptr(), h, w, win, ov, cover, 307.0, 5.5, 0.6, 0.2, 1, S()) == SHAPE_ERR
            assert fn_b(sr.data_ptr(), out.data_ptr(), h, w, win, ov, cover, 307.0, 5.5, S()) == SHAPE_ERR
    assert fn_p(lst_c.data_ptr(), ndvi_c.data_ptr(), x.data_ptr(), 200, 136, 64, 16, 1, 307.0, 0.0, 0.6, 0.2, 1, S()) == SHAPE_ERR
    assert fn_p(None, ndvi_c.data_ptr(), x.data_ptr(), 200, 136, 64, 16, 1, 307.0, 5.5, 0.6, 0.2, 1, S()) == 1002
    assert fn_b(sr.data_ptr(), None, 200, 136, 64, 16, 1, 307.0, 5.5, S()) == 1002
    torch.cuda.synchronize()
    assert torch.isnan(x).all() and torch.isnan(out).all()
