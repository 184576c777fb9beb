"""GPU: conservation of the observed LST at any ratio (include/sifsr_rconserve.h, sifsr/rconserve.py) against the
float64 NumPy restatement tests/rconserve_reference.py (held to the sensor model's and the resampler's own restatements by
tests/test_rconserve_host.py).

Shapes (tests/rconserve_reference.SHAPES), the smallest at which each part can go wrong: lst 12 x 16 at x3, x2.5, x2 and x4 and
12 x 15 at x8/3 (one workgroup; cells of 2 and 3 pixels; stencils of 3 and of 5 cells; the ring on both sides, on one side, on none),
2 x 2 at x3 (the smallest raster accepted: every bicubic index clamps, both reflections meet), per ratio one raster of more than one
16 x 16 tile on both axes with a ragged last tile, and 8 x 14 at x8, where the tile is 6 x 6 cells.

Bars, from the issue.  Tight: the count is exact; the residual of the pure check is the restatement's to the one fp32 rounding,
2^-23 |r| + 1e-7 K per element; row 0 of the statistics to 1e-5 K; one step at relax 1 is sr + ratio.upsample(r) bit for bit at the
pixels of valid cells; consistency(out) is the last statistics row bit for bit.  Project: rasters and later rows to TOL = 2e-4 K, the
bar of f12 / f15 (one ulp at 300 K is 3e-5 K and a step can flip it).  Against sifsr.conserve at x4: equal counts, values within
1e-3 K (f12 keeps fp32 PSF taps: neither is the other's reference).  Every test prints what it measures."""
import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import rconserve_reference as Q
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal
from tests.test_mosaic_gpu import STATS, _model

pytestmark = pytest.mark.gpu
TOL = 2e-4
SHAPE_ERR, ARG_ERR, WORKSPACE_ERR = 1001, 1002, 1003
IDS = [f"{s[0]}x{s[1]}at{p}:{q}" for s, (p, q) in Q.SHAPES]


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def run(sifsr, sr, lst, mask, n_iter, relax=1.0, in_place=False):
    """-> (out fp32 (H,W) or None, stats (n_iter+1,4) float64, r fp32 (h,w) of the last row, sr as the device holds it after)"""
    h, w = lst.shape
    s = dev(sr)
    out = s if in_place else (torch.full(sr.shape, -7.0, device="cuda") if n_iter else None)
    stats, ws = sifsr.rconserve._call(s, dev(lst), dev(mask), out, n_iter, relax, 0.1)
    torch.cuda.synchronize()
    r = ws[:4 * h * w].view(torch.float32).view(h, w).cpu().numpy()
    return (None if out is None else out.cpu().numpy()), stats.cpu().numpy(), r, s.cpu().numpy()


def compare(tag, got, ref, sr):
    """out, r and the statistics against the restatement; prints what it measures"""
    out, stats, r, _ = got
    ro, rstats, rr, c, n = ref
    d_out = 0.0
    if out is not None:
        m = Q.up(c, sr.shape)
        assert np.array_equal(bits(out)[~m], bits(np.asarray(sr, np.float32))[~m]), f"{tag}: a pixel of a cell without c moved"
        d_out = float(np.abs(out[m].astype(np.float64) - ro[m]).max()) if m.any() else 0.0
    d_r = np.abs(r.astype(np.float64) - rr)
    assert (r[~n] == 0).all() and not np.isnan(r).any()
    own = Q.stats_row(r.astype(np.float64), n)
    d_s = float(np.abs(stats[:, 1:] - rstats[:, 1:]).max()) if own[0] else 0.0
    print(f"{tag}: max|out - ref| = {d_out:.3e} K, max|r - ref| = {float(d_r.max()):.3e} K, max|stats - ref| = {d_s:.3e}, last row {stats[-1].tolist()}")
    assert stats.shape == rstats.shape and np.array_equal(stats[:, 0], rstats[:, 0])                  # the count is exact
    if stats.shape[0] == 1:
        assert np.all(d_r <= 2.0 ** -23 * np.abs(rr) + 1e-7)                                             # the one fp32 rounding
    assert d_out <= TOL and float(d_r.max()) <= TOL
    if own[0] == 0:
        assert np.isnan(stats[:, 1:]).all()
    else:
        assert np.all(np.abs(stats[-1, 1:] - own[1:]) <= 1e-12 * np.abs(own[1:])), (stats[-1], own)   # the device's own r, in float64
        assert np.abs(stats[0, 1:] - rstats[0, 1:]).max() <= 1e-5 and d_s <= TOL
    return d_out


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [0, 1, 3])
@pytest.mark.parametrize("idx", range(len(Q.SHAPES)), ids=IDS)
def test_shapes(sifsr, idx, n_iter):
    shape, pq = Q.SHAPES[idx]
    sr, lst = Q.make_case(shape, pq, seed=100 + idx)
    for relax in (1.0, 0.5):
        got = run(sifsr, sr, lst, None, n_iter, relax)
        ref = Q.conserve_ref(sr, lst, None, n_iter, relax)
        compare(f"{IDS[idx]} n_iter {n_iter} relax {relax}", got, ref, sr)
        assert np.array_equal(bits(got[3]), bits(sr))                              # the const input
        assert got[1][0, 0] == Q.counted(np.ones(shape, bool), sr.shape).sum() > 0     # all valid: everything off the ring
        if n_iter == 0:
            assert got[0] is None
            continue
        alias = run(sifsr, sr, lst, None, n_iter, relax, in_place=True)
        assert np.array_equal(bits(alias[0]), bits(got[0])) and np.array_equal(bits(alias[1]), bits(got[1]))
        assert np.array_equal(bits(alias[2]), bits(got[2])) and np.array_equal(bits(alias[3]), bits(got[0]))   # sr itself holds the result
        # consistency(out) is the last row, bit for bit
        again = run(sifsr, got[0], lst, None, 0)
        assert np.array_equal(bits(again[1][0]), bits(got[1][-1])) and np.array_equal(bits(again[2]), bits(got[2]))
    if n_iter == 1:
        # one step at relax 1 is sr + ratio.upsample(r), bit for bit (every cell is valid here)
        r0 = run(sifsr, sr, lst, None, 0)[2]
        want = dev(sr) + sifsr.ratio.upsample(dev(r0), sr.shape)
        assert np.array_equal(bits(run(sifsr, sr, lst, None, 1)[0]), bits(want))


# ---- 2. gaps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Q.HOLES)
@pytest.mark.parametrize("pq", Q.RATIOS, ids=lambda r: f"{r[0]}:{r[1]}")
def test_holes(sifsr, pq, kind):
    sr, lst, mask = Q.hole_case(kind, pq)
    for n_iter in (0, 1, 3):
        got = run(sifsr, sr, lst, mask, n_iter)
        ref = Q.conserve_ref(sr, lst, mask, n_iter)
        compare(f"{pq} {kind} n_iter {n_iter}", got, ref, sr)
        c, n = ref[3], ref[4]
        m = Q.up(c, sr.shape)
        if kind in ("nothing_valid", "checkerboard"):
            assert not n.any() and got[1][-1, 0] == 0 and np.isnan(got[1][:, 1:]).all()
            if got[0] is not None:                                                   # r = 0 everywhere: nothing moves
                assert np.array_equal(bits(got[0]), bits(sr))
        else:
            assert 0 < n.sum() < c.sum() < c.size
        if n_iter == 1 and m.any():                                                  # sr + U(r) at the pixels of valid cells
            want = dev(sr) + sifsr.ratio.upsample(dev(run(sifsr, sr, lst, mask, 0)[2]), sr.shape)
            assert np.array_equal(bits(got[0])[m], bits(want)[m])
        # what the invalid pixels hold changes no output bit
        for junk in (np.nan, 0.0, np.inf, 1e30):
            if junk == 1e30 and mask is None and kind != "sr_nan":
                continue                                                             # only a mask or a bad sr pixel makes 1e30 invalid
            psr, plst = Q.poisoned(sr, lst, mask, junk)
            other = run(sifsr, psr, plst, mask, n_iter)
            assert np.array_equal(bits(other[1]), bits(got[1])) and np.array_equal(bits(other[2]), bits(got[2])), (kind, junk)
            if got[0] is not None:
                assert np.array_equal(bits(other[0])[m], bits(got[0])[m]), (kind, junk)
                assert np.array_equal(bits(other[0])[~m], bits(psr)[~m])
        again = run(sifsr, sr, lst, mask, n_iter)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:3], again[:3]) if a is not None)


@pytest.mark.parametrize("pq", Q.RATIOS, ids=lambda r: f"{r[0]}:{r[1]}")
def test_convergence(sifsr, pq):
    """what the restatement shows on the CPU (tests/test_rconserve_host.py): the RMSE falls with every one of three steps"""
    shape = (12, 15) if pq == (8, 3) else (12, 16)
    sr, lst = Q.make_case(shape, pq, seed=5, noise=0.5)
    _, stats, _, _ = run(sifsr, sr, lst, None, 3)
    print(f"{pq}: counted {int(stats[0, 0])}, RMSE {stats[:, 2].tolist()}")
    assert np.all(np.diff(stats[:, 2]) < 0) and np.all(stats[:, 0] == stats[0, 0])


def test_cross_check_at_x4(sifsr):
    """beside sifsr.conserve on the same rasters: the counted set is the same; the values differ by the fp32 PSF taps and the fp32
    sums of f12 (neither is the other's reference)"""
    from tests import conserve_reference as R
    worst_r = worst_o = 0.0
    for sr, lst, mask in (R.hole_case("mask_block"), R.hole_case("sr_only"), R.hole_case("corner"), R.make_case(33, 41, 9) + (None,)):
        for n_iter in (0, 2):
            got = run(sifsr, sr, lst, mask, n_iter)
            o4, s4 = sifsr.conserve.conserve(dev(sr), dev(lst), dev(mask), n_iter=n_iter, return_stats=True)
            r4 = sifsr.conserve.consistency(o4, dev(lst), dev(mask), return_residual=True)[1].cpu().numpy()
            s4 = s4.cpu().numpy()
            assert np.array_equal(got[1][:, 0], s4[:, 0]) and np.array_equal(got[2] != 0, r4 != 0) and s4[0, 0] > 0
            worst_r = max(worst_r, float(np.abs(got[2] - r4).max()), float(np.abs(got[1][:, 1:] - s4[:, 1:]).max()))
            if n_iter:
                m = R.up(R.cell_valid(sr, lst, mask))
                worst_o = max(worst_o, float(np.abs(got[0][m] - o4.cpu().numpy()[m]).max()))
    print(f"x4 beside sifsr.conserve: max|r - r_f12| = {worst_r:.3e} K, max|out - out_f12| = {worst_o:.3e} K")
    assert worst_r <= 1e-3 and worst_o <= 1e-3


def test_public_calls(sifsr):
    C = sifsr.rconserve
    sr, lst, mask = Q.hole_case("block", (5, 2))
    s, l, m = dev(sr), dev(lst), dev(mask)
    row, r = C.consistency(s, l, m, return_residual=True)
    assert row.dtype == torch.float64 and tuple(row.shape) == (4,) and r.dtype == torch.float32 and tuple(r.shape) == lst.shape
    assert bit_equal(row, C.consistency(s, l, m)) and bit_equal(row, C.consistency(s, l, m.bool()))
    want = run(sifsr, sr, lst, mask, 0)
    assert np.array_equal(bits(row), bits(want[1][0])) and np.array_equal(bits(r), bits(want[2]))
    out, stats = C.conserve(s, l, m, n_iter=2, relax=0.75, return_stats=True)
    want = run(sifsr, sr, lst, mask, 2, relax=0.75)
    assert np.array_equal(bits(out), bits(want[0])) and np.array_equal(bits(stats), bits(want[1])) and np.array_equal(bits(s), bits(sr))
    assert bit_equal(stats[0], row) and bit_equal(C.consistency(out, l, m), stats[2])
    buf = torch.zeros_like(s)
    assert C.conserve(s, l, m, n_iter=2, relax=0.75, out=buf) is buf and bit_equal(buf, out)
    same = C.conserve(s, l, m, n_iter=0)                                             # the pure check copies
    assert same is not s and bit_equal(same, s)
    inp = s.clone()
    assert C.conserve(inp, l, m, n_iter=2, relax=0.75, out=inp) is inp and bit_equal(inp, out)
    E = sifsr.SifsrError
    for bad in (lambda: C.conserve(s, l[:10].contiguous()), lambda: C.conserve(s.cpu(), l), lambda: C.conserve(s, l, m.float()),
                lambda: C.conserve(s, l, n_iter=-1), lambda: C.conserve(s, l, n_iter=65), lambda: C.conserve(s, l, out=buf[:, :30]),
                lambda: C.consistency(torch.zeros((20, 25), device="cuda"), torch.zeros((16, 20), device="cuda")),
                lambda: C.consistency(l, l), lambda: C.consistency(s, l, mtf=1.0), lambda: C.consistency(s.double(), l)):
        with pytest.raises(E):
            bad()


# ---- 3. prediction ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(sifsr):
    return _model(sifsr, O.synthetic_state(3))


def _rasters(seed, h, w, p, q):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((h, w)) * 5.5 + 307).astype(np.float32), (rs.standard_normal((h * p // q, w * p // q)) * 0.6 + 0.5).astype(np.float32)


@pytest.mark.parametrize("win,hr,h,w,p,q", [(8, 24, 21, 27, 3, 1), (16, 40, 38, 46, 5, 2)])
def test_predict_granule_conserve(sifsr, model, win, hr, h, w, p, q):
    lst_np, ndvi_np = _rasters(hr, h, w, p, q)
    lst, ndvi = dev(lst_np), dev(ndvi_np)
    P, C = sifsr.ratio.predict_granule, sifsr.rconserve
    for kw in (dict(batch=4), dict(batch=5, overlap=2, cover_edges=True), dict(batch=7, overlap=2)):
        kw = dict(window=win, hr=hr, **kw)
        base = P(model, lst, ndvi, STATS, **kw)
        assert bit_equal(P(model, lst, ndvi, STATS, conserve=0, **kw), base)
        two = P(model, lst, ndvi, STATS, conserve=2, **kw)
        want, stats = C.conserve(base, lst, n_iter=2, return_stats=True)
        assert bit_equal(two, want) and not bit_equal(two, base)
        s = stats.cpu().numpy()
        print(f"ratio.predict_granule ({win},{hr}) {kw}: counted {int(s[0, 0])}, RMSE {s[:, 2].tolist()} K")
        assert s[0, 0] > 0 and s[2, 2] < s[1, 2] < s[0, 2]
        if not kw.get("cover_edges"):                                                # the uncovered edge does not move
            Hc, Wc = (h - (h - win) % (win - kw.get("overlap", 0))) * p // q, (w - (w - win) % (win - kw.get("overlap", 0))) * p // q
            assert Hc < h * p // q and Wc < w * p // q
            assert two[Hc:, :].abs().max().item() == 0 and two[:, Wc:].abs().max().item() == 0 and base[:Hc, :Wc].abs().min().item() > 0
    with pytest.raises(sifsr.SifsrError):
        P(model, lst, ndvi, STATS, window=win, hr=hr, conserve=-1)


@pytest.mark.parametrize("win,hr,h,w,p,q", [(8, 24, 21, 27, 3, 1), (16, 40, 38, 46, 5, 2)])
def test_predict_granule_gaps_conserve(sifsr, model, win, hr, h, w, p, q):
    lst_np, ndvi_np = _rasters(hr + 1, h, w, p, q)
    lst_np[:win, :win] = 0.0                                                         # an all-gap tile
    lst_np[h // 2, w // 2] = np.nan
    lst_np[h - 3, 2] = 0.0
    mask_np = np.ones((h, w), np.uint8)
    mask_np[h // 2 + 3:h // 2 + 5, 3:7] = 0
    lst, ndvi, mask = dev(lst_np), dev(ndvi_np), dev(mask_np)
    G, C = sifsr.ratio.predict_granule_gaps, sifsr.rconserve
    for kw in (dict(batch=5, overlap=2, cover_edges=True), dict(batch=4, overlap=0, cover_edges=False)):
        kw = dict(window=win, hr=hr, **kw)
        base, info0 = G(model, lst, ndvi, STATS, mask=mask, return_info=True, **kw)
        assert "conserve_stats" not in info0
        assert bit_equal(G(model, lst, ndvi, STATS, mask=mask, conserve=0, **kw), base)
        two, info = G(model, lst, ndvi, STATS, mask=mask, conserve=2, return_info=True, **kw)
        want, stats = C.conserve(base, lst, mask, n_iter=2, return_stats=True)
        assert bit_equal(two, want) and bit_equal(info["conserve_stats"], stats) and info["n_active"] == info0["n_active"]
        assert bit_equal(G(model, lst, ndvi, STATS, mask=mask, conserve=2, **kw), two)
        valid = info["valid"].cpu().numpy()
        up = Q.up(valid, two.shape)
        o = two.cpu().numpy()
        assert np.isnan(o[~up]).all() and not np.isnan(o[up]).any() and (~up).any()
        s = stats.cpu().numpy()
        n_ref = int(Q.counted(Q.cell_valid(base.cpu().numpy(), lst_np, mask_np), two.shape).sum())
        print(f"ratio.predict_granule_gaps ({win},{hr}) {kw}: counted {int(s[0, 0])} of {int(valid.sum())} valid cells, RMSE {s[:, 2].tolist()} K")
        assert s[0, 0] == s[2, 0] == n_ref and 0 < n_ref < valid.sum() and s[2, 2] < s[0, 2]
    with pytest.raises(sifsr.SifsrError):
        G(model, lst, ndvi, STATS, window=win, hr=hr, overlap=2, conserve=-2)


# ---- 4. the C entry point: a captured call, errors, memory contract ----------------------------------------------------------------
def _buffers(L, idx, n_iter, mask):
    shape, pq = Q.SHAPES[idx]
    sr_np, lst_np = Q.make_case(shape, pq, seed=40 + idx)
    (h, w), (H, W) = shape, sr_np.shape
    need = L.call("sifsrc_workspace_bytes", h, w, H, W, n_iter)
    assert need > 0
    m = None
    if mask:
        m = np.ones(shape, np.uint8)
        m[h // 2, w // 3] = 0
    return (dev(sr_np), dev(lst_np), dev(m), torch.empty((H, W), device="cuda"), torch.empty((n_iter + 1, 4), dtype=torch.float64, device="cuda"),
            torch.empty((need,), dtype=torch.uint8, device="cuda"), need, h, w, H, W)


def test_captured_call_replays_the_eager_bits(L):
    sr, lst, mask, out, stats, ws, need, h, w, H, W = _buffers(L, 7, 2, True)      # 20 x 34 at x2.5: four tiles
    call = lambda: L.call("sifsrc_conserve", sr, lst, mask, out, stats, ws, need, h, w, H, W, 0.1, 0.75, 2, S())
    call()
    torch.cuda.synchronize()
    want = (out.clone(), stats.clone(), ws[:4 * h * w].clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in (out, stats, ws):
        t.view(torch.uint8).fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    assert bit_equal(out, want[0]) and bit_equal(stats, want[1]) and bit_equal(ws[:4 * h * w], want[2])
    sr.add_(0.25)                                                                    # other inputs, the same graph
    graph.replay()
    torch.cuda.synchronize()
    got = (out.clone(), stats.clone())
    call()
    torch.cuda.synchronize()
    assert bit_equal(out, got[0]) and bit_equal(stats, got[1]) and not bit_equal(out, want[0])


def test_errors_launch_nothing(L):
    h, w, H, W = 12, 16, 30, 40
    fn, size = L.lib().sifsrc_conserve, L.lib().sifsrc_workspace_bytes
    need = size(h, w, H, W, 2)
    sr, out = torch.full((H, W), 77.0, device="cuda"), torch.full((H, W), 77.0, device="cuda")
    lst, mask = torch.full((h, w), 77.0, device="cuda"), torch.full((h, w), 77, dtype=torch.uint8, device="cuda")
    stats = torch.full((3, 4), 77.0, dtype=torch.float64, device="cuda")
    ws = torch.full((need + 16,), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    args = lambda **kw: [kw.get("sr", p(sr)), kw.get("lst", p(lst)), kw.get("mask", p(mask)), kw.get("out", p(out)), kw.get("stats", p(stats)),
                         kw.get("ws", p(ws)), kw.get("nbytes", need), kw.get("h", h), kw.get("w", w), kw.get("H", H), kw.get("W", W),
                         kw.get("mtf", 0.1), kw.get("relax", 1.0), kw.get("n_iter", 2), S()]
    for bad in (dict(h=11), dict(w=15), dict(H=31), dict(h=0), dict(w=-1), dict(h=16, w=20, H=20, W=25), dict(H=12, W=16), dict(H=108, W=144),
                dict(n_iter=-1), dict(n_iter=65), dict(mtf=0.0), dict(mtf=1.0), dict(mtf=float("nan"))):
        assert fn(*args(**bad)) == SHAPE_ERR, bad
    for bad in (dict(sr=None), dict(lst=None), dict(out=None), dict(stats=None), dict(ws=None), dict(ws=p(ws) + 8), dict(sr=p(sr) + 2),
                dict(out=p(out) + 1), dict(stats=p(stats) + 4), dict(relax=float("nan")), dict(relax=float("inf"))):
        assert fn(*args(**bad)) == ARG_ERR, bad
    for bad in (dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=size(h, w, H, W, 1))):
        assert fn(*args(**bad)) == WORKSPACE_ERR, bad
    torch.cuda.synchronize()
    for t in (sr, out, lst, mask, stats, ws):
        assert (t == 77).all()
    assert fn(*args(out=None, n_iter=0, nbytes=size(h, w, H, W, 0))) == 0           # the pure check needs no out
    assert fn(*args(mask=None)) == 0
    torch.cuda.synchronize()
    assert (sr == 77).all() and (lst == 77).all() and (ws[need:] == 77).all()


# (index into Q.SHAPES, n_iter, mask, in place): mask NULL / given, the pure check with out NULL, out aliasing sr, ragged multi-tile
CONTRACT_SHAPES = [(5, 1, False, False), (1, 0, True, False), (7, 2, True, False), (4, 3, False, True), (2, 1, True, True), (11, 2, True, False),
                   (6, 1, False, True)]


def contract_inputs(i):
    idx, n_iter, with_mask, in_place = CONTRACT_SHAPES[i]
    shape, pq = Q.SHAPES[idx]
    sr_np, lst_np = Q.make_case(shape, pq, seed=500 + i)
    (h, w), (H, W) = shape, sr_np.shape
    if h >= 8:
        lst_np[h // 2, w // 2] = 0.0
        sr_np[-(-2 * H // h), -(-2 * W // w) + 1] = np.nan          # a pixel of cell (2, 2)
    mask_np = None
    if with_mask:
        mask_np = np.ones((h, w), np.uint8)
        mask_np[h - 2, w - 3] = 0
    return sr_np, lst_np, mask_np


def conserve_case(i):
    def make(k):
        idx, n_iter, with_mask, in_place = CONTRACT_SHAPES[i]
        sr_np, lst_np, mask_np = contract_inputs(i)
        (h, w), (H, W) = lst_np.shape, sr_np.shape
        lst = k.t("lst", torch.from_numpy(lst_np))
        mask = k.t("mask", torch.from_numpy(mask_np)) if with_mask else None
        if in_place:
            sr = out = k.A.inout(torch.from_numpy(sr_np), "sr")
        else:
            sr = k.t("sr", torch.from_numpy(sr_np))
            out = k.o("out", H, W) if n_iter else None
        stats = k.o("stats", n_iter + 1, 4, dtype=torch.float64)
        need = k.L.call("sifsrc_workspace_bytes", h, w, H, W, n_iter)
        ws = k.A.scratch(need, "workspace")                       # poisoned scratch: nothing of it may reach the outputs
        call = lambda: k.L.call("sifsrc_conserve", sr, lst, mask, out, stats, ws, need, h, w, H, W, 0.1, 0.75, n_iter, S())
        outs = {"stats": stats, "r": ws[:4 * h * w].view(torch.float32)}
        if out is not None:
            outs["out"] = out
        return call, outs
    return make


CONTRACT = {"sifsrc_conserve": [conserve_case(i) for i in range(len(CONTRACT_SHAPES))]}


def _as_bits(res):
    # NaN is data here (a NaN sr pixel keeps its bits; statistics of nothing are NaN): compare those by bits, keep the NaN check for r
    res["stats"] = res["stats"].view(torch.int64)
    if "out" in res:
        res["out"] = res["out"].view(torch.int32)
    return res


@pytest.mark.parametrize("idx", range(len(CONTRACT_SHAPES)))
def test_memory_contract(L, idx):
    """out, stats and r written in full and nowhere else -- bit-identical under every poison of the outputs and of the workspace, r
    NaN-free under the NaN poison --, const inputs untouched, nothing outside the buffers written, the same bits on ordinary
    allocations, and the result is the restatement's."""
    first = run_contract(L, CONTRACT["sifsrc_conserve"][idx], seed=977 + idx, capacity=64 << 20, view=_as_bits)
    n_iter = CONTRACT_SHAPES[idx][1]
    sr, lst, mask = contract_inputs(idx)
    ro, rstats, rr, c, n = Q.conserve_ref(sr, lst, mask, n_iter, relax=0.75)
    stats = first["stats"].view(torch.float64).cpu().numpy()
    assert np.array_equal(stats[:, 0], rstats[:, 0])
    if n.any():
        assert np.abs(stats[:, 1:] - rstats[:, 1:]).max() <= TOL
    assert np.abs(first["r"].view(lst.shape).cpu().numpy() - rr).max() <= TOL
    if n_iter:
        out = first["out"].view(torch.float32).cpu().numpy()
        m = Q.up(c, sr.shape)
        assert np.abs(out[m] - ro[m]).max() <= TOL and np.array_equal(bits(out)[~m], bits(sr)[~m])
