"""GPU: conservation of the observed LST (include/sifsr_conserve.h, sifsr/conserve.py) against the float64 NumPy
restatement tests/conserve_reference.py (pinned to the reference by tests/golden/make_golden_conserve.py, held to itself by
tests/test_conserve_host.py).

Shapes (LR; the HR raster is 4x), the smallest at which each part can go wrong:

    3x3        the minimum: both reflect zones meet in one tile, every bicubic index is clamped
    5x7, 9x8   ragged, non-square; 9x8 has a second, one-row workgroup
    8x8        exactly one workgroup
    33x41      partial workgroup tiles on both axes, residual stencils and the x4 resampler across tile seams
    16x16      with the planted gaps of conserve_reference.HOLES

TOL.  The correction is some tenths of a kelvin on values near 300 K, so the bar is absolute.  Measured on an MI355X over every
case of this file (printed by each test): the largest |out - restatement| is 4.6e-5 K (n_iter = 3; 1.7e-5 K at n_iter = 1 --
half an fp32 ulp at 300 K, 1.5e-5 K, per step is its floor) and the largest |r - restatement| 5.7e-6 K.  The bar is the larger
of the two with a margin of x4, rounded up to one significant digit: 2e-4 K, below the 1e-3 K the feature may not exceed.  The statistics are held to the
restatement computed from the device's own r at 1e-12 relative, and to the full restatement at TOL."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import conserve_reference as R
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal
from tests.test_mosaic_gpu import STATS, _granule, _model

pytestmark = pytest.mark.gpu
TOL = 2e-4
SHAPE_ERR, ARG_ERR, WORKSPACE_ERR = 1001, 1002, 1003
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_conserve_v1.npz")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def run(sifsr, sr, lst, mask, n_iter, relax=1.0, in_place=False):
    """-> (out fp32 (4h,4w) or None, stats (n_iter+1,4) float64, r fp32 (h,w) of the last row, sr as the device holds it after)"""
    h, w = lst.shape
    s = dev(sr)
    out = s if in_place else (torch.full((4 * h, 4 * w), -7.0, device="cuda") if n_iter else None)
    stats, ws = sifsr.conserve._call(s, dev(lst), dev(mask), out, n_iter, relax, 0.1)
    torch.cuda.synchronize()
    r = ws[:4 * h * w].view(torch.float32).view(h, w).cpu().numpy()
    return (None if out is None else out.cpu().numpy()), stats.cpu().numpy(), r, s.cpu().numpy()


def compare(tag, got, ref, sr, lst, mask):
    """out, r and both forms of the statistics against the restatement; prints what it measures -> (dev_out, dev_r)"""
    out, stats, r, _ = got
    ro, rstats, rr, c, n = ref
    d_out = 0.0
    if out is not None:
        m = R.up(c)
        assert np.array_equal(bits(out)[~m], bits(np.asarray(sr, np.float32))[~m]), f"{tag}: a pixel of a cell without c moved"
        d_out = float(np.abs(out[m].astype(np.float64) - ro[m]).max()) if m.any() else 0.0
    d_r = float(np.abs(r.astype(np.float64) - rr).max())
    assert (r[~n] == 0).all() and not np.isnan(r).any()
    own = R.stats_row(r.astype(np.float64), n)
    last = stats[-1]
    print(f"{tag}: max|out - ref| = {d_out:.3e} K, max|r - ref| = {d_r:.3e} K, stats {last.tolist()} vs own r {own.tolist()} vs ref {rstats[-1].tolist()}")
    assert d_out <= TOL and d_r <= TOL
    assert stats.shape == rstats.shape and np.array_equal(stats[:, 0], rstats[:, 0])
    if own[0] == 0:
        assert np.isnan(stats[:, 1:]).all()
    else:
        assert np.all(np.abs(last[1:] - own[1:]) <= 1e-12 * np.abs(own[1:])), (last, own)
        assert np.all(np.abs(stats[:, 1:] - rstats[:, 1:]) <= TOL), (stats, rstats)
    return d_out, d_r


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [0, 1, 3])
@pytest.mark.parametrize("hw", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(sifsr, hw, n_iter):
    sr, lst = R.make_case(*hw, seed=100 + hw[0])
    got = run(sifsr, sr, lst, None, n_iter)
    ref = R.conserve_ref(sr, lst, None, n_iter)
    compare(f"{hw} n_iter {n_iter}", got, ref, sr, lst, None)
    assert np.array_equal(bits(got[3]), bits(sr))                                  # the const input
    assert got[1][0, 0] == hw[0] * hw[1]                                           # all valid: every cell is counted
    if n_iter == 0:
        assert got[0] is None
    again = run(sifsr, sr, lst, None, n_iter)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:3], again[:3]) if a is not None)


@pytest.mark.parametrize("hw", [(9, 8), (33, 41)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_relax_and_in_place(sifsr, hw):
    sr, lst = R.make_case(*hw, seed=300 + hw[0])
    mask = (np.random.RandomState(1).uniform(size=hw) > 0.08).astype(np.uint8)
    for n_iter in (1, 3):
        got = run(sifsr, sr, lst, mask, n_iter, relax=0.5)
        compare(f"{hw} relax 0.5 n_iter {n_iter}", got, R.conserve_ref(sr, lst, mask, n_iter, relax=0.5), sr, lst, mask)
        alias = run(sifsr, sr, lst, mask, n_iter, relax=0.5, in_place=True)
        assert np.array_equal(bits(alias[0]), bits(got[0])) and np.array_equal(bits(alias[1]), bits(got[1]))
        assert np.array_equal(bits(alias[3]), bits(got[0]))                         # sr itself now holds the result


# ---- 2. gaps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.HOLES)
def test_holes(sifsr, kind):
    sr, lst, mask = R.hole_case(kind)
    for n_iter in (0, 1, 3):
        got = run(sifsr, sr, lst, mask, n_iter)
        ref = R.conserve_ref(sr, lst, mask, n_iter)
        compare(f"{kind} n_iter {n_iter}", got, ref, sr, lst, mask)
        c, n = ref[3], ref[4]
        if kind in ("nothing_valid", "checkerboard"):
            assert not n.any() and got[1][-1, 0] == 0 and np.isnan(got[1][:, 1:]).all()
            if got[0] is not None:                                                   # r = 0 everywhere: nothing moves
                assert np.array_equal(got[0][R.up(c)], sr[R.up(c)])
        else:
            assert 0 < n.sum() < c.sum() < c.size
        # what the invalid pixels hold changes no output bit
        for junk in (np.nan, 0.0, np.inf, 1e30):
            if junk == 1e30 and mask is None and kind != "sr_only":
                continue                                                             # only a mask or a bad sr pixel makes 1e30 invalid
            psr, plst = R.poisoned(sr, lst, mask, junk)
            other = run(sifsr, psr, plst, mask, n_iter)
            assert np.array_equal(bits(other[1]), bits(got[1])) and np.array_equal(bits(other[2]), bits(got[2])), (kind, junk)
            if got[0] is not None:
                m = R.up(c)
                assert np.array_equal(bits(other[0])[m], bits(got[0])[m]), (kind, junk)
                assert np.array_equal(bits(other[0])[~m], bits(psr)[~m])
        again = run(sifsr, sr, lst, mask, n_iter)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:3], again[:3]) if a is not None)


def test_golden_cases_and_convergence(sifsr):
    """the pinned cases: the device reproduces the recorded r, out and statistics; and what the restatement shows over three steps
    (tests/test_conserve_host.py): the RMSE falls with every step"""
    gold = np.load(GOLDEN)
    for i, name in enumerate(gold["names"]):
        sr, lst, mask, relax = gold[f"c{i}_sr"], gold[f"c{i}_lst"], gold[f"c{i}_mask"], float(gold[f"c{i}_relax"])
        mask = None if mask.size == 0 else mask
        out, stats, _, _ = run(sifsr, sr, lst, mask, 3, relax)
        _, _, r0, _ = run(sifsr, sr, lst, mask, 0)
        c = R.up(R.cell_valid(sr, lst, mask))
        d_out, d_r = np.abs(out[c] - gold[f"c{i}_out3"][c]).max(), np.abs(r0 - gold[f"c{i}_r0"]).max()
        print(f"{name}: max|out - golden| = {d_out:.3e} K, max|r0 - golden| = {d_r:.3e} K, RMSE {stats[:, 2].tolist()}")
        assert d_out <= TOL and d_r <= TOL
        assert np.array_equal(stats[:, 0], gold[f"c{i}_stats"][:, 0]) and np.abs(stats[:, 1:] - gold[f"c{i}_stats"][:, 1:]).max() <= TOL
        assert np.all(np.diff(stats[:, 2]) < 0)


def test_public_calls(sifsr):
    sr, lst, mask = R.hole_case("mask_block")
    s, l, m = dev(sr), dev(lst), dev(mask)
    row, r = sifsr.conserve.consistency(s, l, m, return_residual=True)
    assert row.dtype == torch.float64 and tuple(row.shape) == (4,) and r.dtype == torch.float32 and tuple(r.shape) == lst.shape
    assert bit_equal(row, sifsr.conserve.consistency(s, l, m)) and bit_equal(row, sifsr.conserve.consistency(s, l, m.bool()))
    want = run(sifsr, sr, lst, mask, 0)
    assert np.array_equal(bits(row), bits(want[1][0])) and np.array_equal(bits(r), bits(want[2]))
    out, stats = sifsr.conserve.conserve(s, l, m, n_iter=2, relax=0.75, return_stats=True)
    want = run(sifsr, sr, lst, mask, 2, relax=0.75)
    assert np.array_equal(bits(out), bits(want[0])) and np.array_equal(bits(stats), bits(want[1])) and np.array_equal(bits(s), bits(sr))
    assert bit_equal(stats[0], row)
    buf = torch.zeros_like(s)
    assert sifsr.conserve.conserve(s, l, m, n_iter=2, relax=0.75, out=buf) is buf and bit_equal(buf, out)
    same = sifsr.conserve.conserve(s, l, m, n_iter=0)                               # the pure check copies
    assert same is not s and bit_equal(same, s)
    E = sifsr.SifsrError
    for bad in (lambda: sifsr.conserve.conserve(s, l[:15].contiguous()), lambda: sifsr.conserve.conserve(s.cpu(), l),
                lambda: sifsr.conserve.conserve(s, l, m.float()), lambda: sifsr.conserve.conserve(s, l, n_iter=-1),
                lambda: sifsr.conserve.conserve(s, l, n_iter=65), lambda: sifsr.conserve.conserve(s, l, out=buf[:, :60]),
                lambda: sifsr.conserve.consistency(s[:8, :8].contiguous(), l[:2, :2].contiguous()),
                lambda: sifsr.conserve.consistency(s.double(), l)):
        with pytest.raises(E):
            bad()


# ---- 3. prediction ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(sifsr):
    return _model(sifsr, O.synthetic_state(3))


def test_predict_granule_conserve(sifsr, model):
    lst_g, ndvi_g = _granule()
    lst, ndvi = lst_g.cuda(), ndvi_g.cuda()
    P = sifsr.predict
    for kw in (dict(batch=4), dict(batch=5, overlap=16, cover_edges=True)):
        base = P.predict_granule(model, lst, ndvi, STATS, **kw)
        assert bit_equal(P.predict_granule(model, lst, ndvi, STATS, conserve=0, **kw), base)
        one = P.predict_granule(model, lst, ndvi, STATS, conserve=1, **kw)
        want, stats = sifsr.conserve.conserve(base, lst, n_iter=1, return_stats=True)
        assert bit_equal(one, want) and not bit_equal(one, base)
        s = stats.cpu().numpy()
        print(f"predict_granule {kw}: counted {int(s[0, 0])}, RMSE {s[0, 2]:.4f} -> {s[1, 2]:.4f} K, bias {s[0, 1]:+.4f} -> {s[1, 1]:+.4f} K")
        assert s[0, 0] > 0 and s[1, 2] < s[0, 2]
        if "overlap" not in kw:                                                      # the reference's zero band stays zero
            assert one[4 * 192:, :].abs().max().item() == 0 and one[:, 4 * 128:].abs().max().item() == 0
    gp = P.GranulePredictor(model, (200, 136), STATS, overlap=16, cover_edges=True, batch=5, conserve=1)
    eager = P.predict_granule(model, lst, ndvi, STATS, batch=5, overlap=16, cover_edges=True, conserve=1)
    assert bit_equal(gp(lst, ndvi), eager)
    assert bit_equal(gp(lst, ndvi), eager)                                           # and after another replay
    gp0 = P.GranulePredictor(model, (200, 136), STATS, overlap=16, cover_edges=True, batch=5)
    assert bit_equal(gp0(lst, ndvi), P.predict_granule(model, lst, ndvi, STATS, batch=5, overlap=16, cover_edges=True))
    with pytest.raises(sifsr.SifsrError):
        P.predict_granule(model, lst, ndvi, STATS, conserve=-1)


def test_predict_granule_gaps_conserve(sifsr, model):
    lst_g, ndvi_g = _granule()
    lst_np = lst_g.numpy().copy()
    lst_np[:64, :] = 0.0
    lst_np[120:131, 70:90] = 0.0
    lst_np[150, 100] = np.nan
    mask_np = np.ones(lst_np.shape, np.uint8)
    mask_np[170:180, 20:40] = 0
    lst, ndvi, mask = dev(lst_np), ndvi_g.cuda(), dev(mask_np)
    G = sifsr.predict.predict_granule_gaps
    kw = dict(window=64, overlap=16, cover_edges=True, batch=5)
    base, info0 = G(model, lst, ndvi, STATS, mask=mask, return_info=True, **kw)
    assert "conserve_stats" not in info0
    assert bit_equal(G(model, lst, ndvi, STATS, mask=mask, conserve=0, **kw), base)
    one, info = G(model, lst, ndvi, STATS, mask=mask, conserve=1, return_info=True, **kw)
    want, stats = sifsr.conserve.conserve(base, lst, mask, n_iter=1, return_stats=True)
    assert bit_equal(one, want) and bit_equal(info["conserve_stats"], stats) and info["n_active"] == info0["n_active"]
    valid = info["valid"].cpu().numpy()
    up = R.up(valid)
    o = one.cpu().numpy()
    assert np.isnan(o[~up]).all() and not np.isnan(o[up]).any()
    s = stats.cpu().numpy()
    n_ref = int(R.counted(valid).sum())
    print(f"predict_granule_gaps: counted {int(s[0, 0])} of {int(valid.sum())} valid cells, RMSE {s[0, 2]:.4f} -> {s[1, 2]:.4f} K")
    assert s[0, 0] == s[1, 0] == n_ref and 0 < n_ref < valid.sum() and s[1, 2] < s[0, 2]
    with pytest.raises(sifsr.SifsrError):
        G(model, lst, ndvi, STATS, conserve=-2, **kw)


# ---- 4. the C entry point: errors, memory contract -----------------------------------------------------------------------------------
def test_errors_launch_nothing(L):
    h, w = 9, 8
    fn, size = L.lib().sifsrk_conserve, L.lib().sifsrk_workspace_bytes
    need = size(h, w, 2)
    sr, out = torch.full((4 * h, 4 * w), 77.0, device="cuda"), torch.full((4 * h, 4 * w), 77.0, device="cuda")
    lst, mask = torch.full((h, w), 77.0, device="cuda"), torch.full((h, w), 77, dtype=torch.uint8, device="cuda")
    stats = torch.full((3, 4), 77.0, dtype=torch.float64, device="cuda")
    ws = torch.full((need + 16,), 77, dtype=torch.uint8, device="cuda")
    taps = (ctypes.c_float * 9)(*[float(v) for v in R.taps32()])
    p = lambda t: t.data_ptr()
    args = lambda **kw: [kw.get("sr", p(sr)), kw.get("lst", p(lst)), kw.get("mask", p(mask)), kw.get("out", p(out)), kw.get("stats", p(stats)),
                         kw.get("ws", p(ws)), kw.get("nbytes", need), kw.get("h", h), kw.get("w", w), kw.get("taps", taps),
                         kw.get("relax", 1.0), kw.get("n_iter", 2), S()]
    for bad in (dict(h=2), dict(w=2), dict(h=0), dict(w=-1), dict(h=16385), dict(w=16385), dict(n_iter=-1), dict(n_iter=65)):
        assert fn(*args(**bad)) == SHAPE_ERR, bad
    for bad in (dict(sr=None), dict(lst=None), dict(out=None), dict(stats=None), dict(ws=None), dict(taps=None), dict(ws=p(ws) + 4),
                dict(sr=p(sr) + 4), dict(out=p(out) + 8), dict(relax=float("nan")), dict(relax=float("inf"))):
        assert fn(*args(**bad)) == ARG_ERR, bad
    for bad in (dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=size(h, w, 1))):
        assert fn(*args(**bad)) == WORKSPACE_ERR, bad
    torch.cuda.synchronize()
    for t in (sr, out, lst, mask, stats, ws):
        assert (t == 77).all()
    assert fn(*args(out=None, n_iter=0, nbytes=size(h, w, 0))) == 0                 # the pure check needs no out
    assert fn(*args(mask=None)) == 0
    torch.cuda.synchronize()
    assert (sr == 77).all() and (lst == 77).all() and (ws[need:] == 77).all()


# (h, w, n_iter, mask, in place)
CONTRACT_SHAPES = [(3, 3, 1, False, False), (9, 8, 0, True, False), (33, 41, 2, True, False), (16, 16, 3, False, True), (5, 7, 1, True, True)]


def contract_inputs(i):
    h, w, n_iter, with_mask, in_place = CONTRACT_SHAPES[i]
    sr_np, lst_np = R.make_case(h, w, seed=500 + i)
    if h >= 9:
        lst_np[h // 2, w // 2] = 0.0
        sr_np[5, 6] = np.nan                                        # cell (1, 1)
    mask_np = None
    if with_mask:
        mask_np = np.ones((h, w), np.uint8)
        mask_np[h - 1, w - 2] = 0
    return sr_np, lst_np, mask_np


def conserve_case(i):
    def make(k):
        h, w, n_iter, with_mask, in_place = CONTRACT_SHAPES[i]
        sr_np, lst_np, mask_np = contract_inputs(i)
        lst = k.t("lst", torch.from_numpy(lst_np))
        mask = k.t("mask", torch.from_numpy(mask_np)) if with_mask else None
        if in_place:
            sr = out = k.A.inout(torch.from_numpy(sr_np), "sr")
        else:
            sr = k.t("sr", torch.from_numpy(sr_np))
            out = k.o("out", 4 * h, 4 * w) if n_iter else None
        stats = k.o("stats", n_iter + 1, 4, dtype=torch.float64)
        need = k.L.call("sifsrk_workspace_bytes", h, w, n_iter)
        ws = k.A.scratch(need, "workspace")                       # poisoned scratch: nothing of it may reach the outputs
        taps = (ctypes.c_float * 9)(*[float(v) for v in R.taps32()])
        call = lambda: k.L.call("sifsrk_conserve", sr, lst, mask, out, stats, ws, need, h, w, taps, 0.75, n_iter, S())
        outs = {"stats": stats, "r": ws[:4 * h * w].view(torch.float32)}
        if out is not None:
            outs["out"] = out
        return call, outs
    return make


CONTRACT = {"sifsrk_conserve": [conserve_case(i) for i in range(len(CONTRACT_SHAPES))]}


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
    first = run_contract(L, CONTRACT["sifsrk_conserve"][idx], seed=977 + idx, capacity=64 << 20, view=_as_bits)
    h, w, n_iter, _, _ = CONTRACT_SHAPES[idx]
    sr, lst, mask = contract_inputs(idx)
    ro, rstats, rr, c, n = R.conserve_ref(sr, lst, mask, n_iter, relax=0.75)
    stats = first["stats"].view(torch.float64).cpu().numpy()
    assert n.any() and np.array_equal(stats[:, 0], rstats[:, 0]) and np.abs(stats[:, 1:] - rstats[:, 1:]).max() <= TOL
    assert np.abs(first["r"].view(h, w).cpu().numpy() - rr).max() <= TOL
    if n_iter:
        out = first["out"].view(torch.float32).cpu().numpy()
        m = R.up(c)
        assert np.abs(out[m] - ro[m]).max() <= TOL and np.array_equal(bits(out)[~m], bits(sr)[~m])
