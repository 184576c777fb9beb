"""GPU: the sharpening baselines at any ratio (csrc/rbaselines_api.h, sifsr/rbaselines.py).

  * against the reference's own outputs at scales 2 and 3 (tests/golden/golden_rbaselines_v1.npz, made by
    tests/golden/make_golden_rbaselines.py): tsharp and the kriging methods with the variogram fit taken out (`variogram=` the
    reference's fit 2) at 1e-4 K; the kriging methods with their own fit at the project's parity bar, 1e-4 of the image's maximum,
    and the semivariogram they fitted at 1e-9 -- the justification of tests/test_baselines_gpu.py: the reference's own image moves
    by less than 1e-4 K when its fit starts elsewhere (asserted by the generator), so the image, not the fitted parameters, is held,
  * all four methods against the float64 restatement tests/rbaselines_reference.py (pinned to that golden and to the x4
    restatements by tests/test_rbaselines_host.py) at the smallest shapes at which a kernel can go wrong (CASES below),
  * the three access widths of the fine raster give the same bits; the rows of a batch are their single-image results; two runs
    give the same bits; at H == 4h the functions agree with sifsr.baselines (the difference is printed),
  * the memory contract of every writing entry point in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is the
    table tests/test_rbaselines_host.py checks against the header), and the argument errors.

Bounds, the families' own (tests/test_baselines_gpu.py, tests/test_dms_gpu.py).  TOL_K = 1e-4 K: float64 arithmetic before the
store, one rounding to float32, whose spacing at 256..512 K is 3.05e-5 K.  TOL_REL = 1e-9 relative on float64 intermediates: sums
of at most a few thousand terms.  Tree structure: exact; every fit of the restatement is far from a tie (asserted: proxy gap
>= 1e-10, frontier gap >= 1e-6).  No pixel is left out but the NaN positions, which must be the restatement's exactly.  Scales 5
and 8 and the rational ratios have no counterpart in the reference: the restatement is their only yardstick."""
import os

import numpy as np
import pytest
import torch

from tests import rbaselines_reference as R
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_rbaselines_v1.npz")
F64 = torch.float64
TOL_K, TOL_REL = 1e-4, 1e-9
PROXY_GAP, HEAP_GAP = 1e-10, 1e-6
SHAPE_ERR, ARG_ERR = 1001, 1002
VARIO = (15.5, 4450.0)          # a fine-scale (sill, range) of the size the reference's fits give for these fields
E = 10


@pytest.fixture(scope="module")
def RB(sifsr):
    from sifsr import rbaselines
    rbaselines.bound()
    return rbaselines


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def dev(a, offset=0):
    """(h,w) or (B,h,w) numpy -> (B,1,h,w) float32 device tensor; offset: the tensor starts that many floats into a 16-byte
    aligned buffer, so its base is off by 4 * offset bytes"""
    a = np.array(a, dtype=np.float32)
    a = a if a.ndim == 3 else a[None]
    if not offset:
        return torch.from_numpy(np.ascontiguousarray(a))[:, None].contiguous().cuda()
    buf = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:].view(a.shape[0], 1, a.shape[1], a.shape[2])
    t.copy_(torch.from_numpy(a)[:, None])
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset
    return t


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def fine_shape(h, w, p, q):
    assert h % q == 0 and w % q == 0
    return h // q * p, w // q * p


def make_inputs(h, w, p, q, seed, zeros=True, nan_cell=True):
    """seeded float32 (lst (h,w), ndvi_coarse (h,w), ndvi_fine (H,W)): a smooth index in [-1, 1], its norm-L4 pooling over the cells,
    lst = 310 - 12 ndvi_coarse + a smooth residual + noise.  zeros: lst == 0 on the raster's edge, rows 0..1 of the last 3 columns
    and the bottom-left corner; nan_cell: every fine pixel of cell (3, 1) is NaN (the coarse index stays finite)."""
    H, W = fine_shape(h, w, p, q)
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64) * (4.0 * q / p)
    ph = rs.uniform(0, 1, 6)
    nf = 0.4 + 0.35 * np.sin(2 * np.pi * (yy / 37 + ph[0])) * np.cos(2 * np.pi * (xx / 29 + ph[1])) \
        + 0.15 * np.sin(2 * np.pi * (yy / 11 + xx / 13 + ph[2])) + 0.03 * rs.standard_normal((H, W))
    nf = np.clip(nf, -1, 1).astype(np.float32)
    m4, _ = R.aggregate(nf, (h, w), pow4=True)
    nc = (m4 ** 0.25).astype(np.float32)
    cy, cx = np.mgrid[0:h, 0:w].astype(np.float64)
    lst = 310 - 12 * nc.astype(np.float64) + 2.0 * np.sin(2 * np.pi * (cy / 7 + ph[3])) * np.cos(2 * np.pi * (cx / 9 + ph[4])) \
        + 0.5 * rs.standard_normal((h, w))
    lst = lst.astype(np.float32)
    if zeros:
        lst[0:2, w - 3:w] = 0.0
        lst[h - 1, 0] = 0.0
    if nan_cell:
        nf[np.ix_(R.cells(h, H) == 3, R.cells(w, W) == 1)] = np.nan
    return lst, nc, nf


# coarse (h, w) and ratio p / q.  5 x 5: a single interior cell; 5 x 9 and 7 x 6; the sharpening pass owns 256 fine columns of
# one coarse row per workgroup and the correction 16 x 256 fine pixels, the prediction 4096: widths past 256 fine columns
# (6 x 130 at x2, 6 x 35 at x8, 6 x 104 at 5/2, 6 x 99 at 8/3) and heights past 16 fine rows (every shape but 5 x 5 at x2 and x3).
# Fine pitches: odd (15, 21, 27, 45), 2 mod 4 (10, 18, 30), multiples of 4 (20, 40, 48, 260, 264, 280).
INT_CASES = [(5, 5, 2), (5, 5, 3), (5, 5, 5), (5, 5, 8), (5, 9, 3), (7, 6, 5), (7, 6, 2), (6, 130, 2), (6, 35, 8), (20, 6, 3), (9, 7, 3)]
RAT_CASES = [(6, 8, 5, 2), (6, 9, 8, 3), (6, 104, 5, 2), (6, 99, 8, 3), (12, 6, 5, 2)]
CASES = [(h, w, s, 1) for h, w, s in INT_CASES] + RAT_CASES
IDS = [f"{h}x{w}-{p}over{q}" for h, w, p, q in CASES]

_REF = {}


def reference(key, fn):
    """the restatement's result for `key`, computed once and shared (read-only)"""
    if key not in _REF:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def check_raster(got, ref, what, tol=TOL_K):
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what               # NaN exactly where the restatement has NaN
    err = float(np.nanmax(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) if (~np.isnan(ref)).any() else 0.0
    print(f"{what}: max |out - ref| = {err:.3e} K, {int(np.isnan(ref).sum())} NaN pixels")
    assert err <= tol, what
    return err


def rel(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max()) if a.size else 0.0


# ---- 1. against the reference's own outputs at scales 2 and 3 ----------------------------------------------------------------------
def gcase(golden, s, i):
    return golden[f"s{s}_c{i}_lst"], golden[f"s{s}_c{i}_ndvi_coarse"], golden[f"s{s}_c{i}_ndvi_fine"]


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_tsharp_vs_golden(RB, golden, s, i):
    lst, nc, nf = gcase(golden, s, i)
    out = host(RB.tsharp(dev(lst), dev(nc), dev(nf), min_T=float(golden["min_T"])))[0, 0]
    ref = golden[f"s{s}_c{i}_tsharp"]
    check_raster(out, ref, f"tsharp x{s} case {i}")
    if i == 2:
        assert np.isnan(ref).sum() == 2 * s * s                               # the NaN fine block and the cell of the NaN coarse index


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("method", ["atprk", "aatprk"])
def test_kriging_vs_golden_with_the_reference_fit(RB, golden, method, i, s):
    """`variogram=` the reference's fit 2: everything but the fit, against the reference's image"""
    lst, nc, nf = gcase(golden, s, i)
    pre = f"s{s}_c{i}_{method}"
    out, info = getattr(RB, method)(dev(lst), dev(nc), dev(nf), scc=float(golden["scc"]), min_T=float(golden["min_T"]),
                                    variogram=golden[pre + "_fit2"], return_variogram=True)
    lam = np.abs(info["lambdas"][0] - golden[pre + "_lambdas"]).max()
    print(f"{method} x{s} case {i}: max |lambda - ref| = {lam:.3e}")
    assert info["gamma_coarse"] is None and info["fit1"] is None and info["lambdas"].shape == (1, s * s, 25) and lam <= TOL_REL
    check_raster(host(out)[0, 0], golden[pre], f"{method} x{s} case {i}, reference fit")


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("method", ["atprk", "aatprk"])
def test_kriging_vs_golden_with_its_own_fit(RB, golden, method, i, s):
    """the package's own fits at scale s: the image at the project's parity bar (1e-4 of its maximum), the empirical semivariogram
    it fitted at 1e-9.  The fitted parameters are printed, not compared."""
    lst, nc, nf = gcase(golden, s, i)
    pre = f"s{s}_c{i}_{method}"
    out, info = getattr(RB, method)(dev(lst), dev(nc), dev(nf), scc=float(golden["scc"]), min_T=float(golden["min_T"]),
                                    return_variogram=True)
    ref = golden[pre]
    err = np.abs(host(out)[0, 0] - ref).max()
    print(f"{method} x{s} case {i}, own fit: fit1 {info['fit1'][0]} fit2 {info['fit2'][0]} (reference {golden[pre + '_fit1']} "
          f"{golden[pre + '_fit2']}); max |out - ref| = {err:.3e} K = {err / np.abs(ref).max():.3e} of the maximum")
    g, gref = info["gamma_coarse"][0], golden[pre + "_gamma"]
    assert info["gamma_coarse"].shape == (1, 15) and info["fit1"].shape == (1, 2) and info["fit2"].shape == (1, 2)
    assert np.abs(g - gref)[1:].max() <= 1e-9 * np.abs(gref[1:]).min() and g[0] == 0
    assert err <= 1e-4 * np.abs(ref).max()


# ---- 2. the regression / kriging methods against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("h,w,p,q", CASES, ids=IDS)
def test_sharpen_vs_restatement(RB, h, w, p, q):
    lst, nc, nf = make_inputs(h, w, p, q, 1000 * h + 10 * w + p)
    l64, c64, f64 = (a.astype(np.float64) for a in (lst, nc, nf))
    a, b, c = dev(lst), dev(nc), dev(nf)
    H, W = fine_shape(h, w, p, q)
    ts = reference(("ts", h, w, p, q), lambda: R.tsharp(l64, c64, f64, 285.0))
    assert np.isnan(ts).sum() == (nf != nf).sum() > 0 and (ts == 0).sum() > 0
    check_raster(host(RB.tsharp(a, b, c))[0, 0], ts, f"tsharp {h}x{w} {p}/{q}")
    if q != 1:
        for fn in (RB.atprk, RB.aatprk):
            with pytest.raises(NotImplementedError, match="integer scales"):
                fn(a, b, c, variogram=VARIO)
        return
    at, _ = reference(("at", h, w, p), lambda: R.atprk(l64, c64, f64, VARIO, 926.0, 285.0))
    aa, _ = reference(("aa", h, w, p), lambda: R.aatprk(l64, c64, f64, VARIO, 926.0, 285.0))
    assert np.isfinite(aa).all() and np.isnan(at).sum() == (nf != nf).sum()
    out, info = RB.atprk(a, b, c, variogram=VARIO, return_variogram=True)
    assert out.shape == (1, 1, H, W) and info["lambdas"].shape == (1, p * p, 25)
    check_raster(host(out)[0, 0], at, f"atprk {h}x{w} x{p}")
    check_raster(host(RB.aatprk(a, b, c, variogram=np.array([VARIO])))[0, 0], aa, f"aatprk {h}x{w} x{p}")
    # the outer two coarse rows and columns hold the plain unmixed value: the result of a zero residual
    plain = torch.empty_like(out)
    fit = torch.empty((1, 2), dtype=F64, device="cuda")
    RB._lib.call("sifsrb_linfit", a, b, fit, 1, h, w, 285.0, S())
    RB._lib.call("sifsrh_sharpen", a, c, fit, torch.zeros((1, h, w), dtype=F64, device="cuda"),
                 torch.from_numpy(info["lambdas"]).cuda(), plain, 1, h, w, H, W, 1, S())
    inner = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    inner[2 * p:H - 2 * p, 2 * p:W - 2 * p] = True
    assert bit_equal(out[0, 0][~inner], plain[0, 0][~inner])
    live = inner & (plain[0, 0] != 0) & ~torch.isnan(plain[0, 0])
    assert live.sum() >= p * p // 2 and (out[0, 0][live] != plain[0, 0][live]).float().mean().item() > 0.9


# ---- 3. DMS against the restatement -------------------------------------------------------------------------------------------------
DMS_CASES = [(5, 5, 2, 1), (5, 9, 3, 1), (7, 6, 5, 1), (5, 5, 8, 1), (6, 130, 2, 1), (20, 6, 3, 1), (6, 8, 5, 2), (6, 9, 8, 3), (6, 104, 5, 2)]
DMS_IDS = [f"{h}x{w}-{p}over{q}" for h, w, p, q in DMS_CASES]


def make_counts(lst, nf, seed, n_est):
    """(E, h*w) bootstrap multiplicities in cell order: n_train draws among the good cells per estimator"""
    mean, std = R.aggregate(nf, lst.shape)
    ts = R.D4.training_set(lst, mean, std)
    idx = np.flatnonzero(ts["good"].ravel())
    rs = np.random.RandomState(seed)
    counts = np.zeros((n_est, lst.size), dtype=np.int64)
    for e in range(n_est):
        counts[e, idx] = np.bincount(rs.randint(0, idx.size, idx.size), minlength=idx.size)
    return counts


def dms_reference(h, w, p, q, n_est=E):
    """(lst, nf, counts, restatement's corrected image, info), computed once and shared; every fit far from a tie"""
    def build():
        lst, _, nf = make_inputs(h, w, p, q, 77 * h + w + p)
        counts = make_counts(lst, nf, 5, n_est)
        out, info = R.dms(lst, nf, counts)
        for t in info["trees"]:
            assert t["proxy_gap"] >= PROXY_GAP and t["heap_gap"] >= HEAP_GAP, (h, w, p, q, t["proxy_gap"], t["heap_gap"])
        return lst, nf, counts, out, info
    return reference(("dms", h, w, p, q, n_est), build)


def tables(trees):
    thr = np.full((len(trees), 29), np.inf)
    nl = np.zeros(len(trees), dtype=np.int32)
    lf = np.zeros((len(trees), 30, 4))
    for e, t in enumerate(trees):
        n = t["leaves"].shape[0]
        thr[e, :n - 1], nl[e], lf[e, :n] = t["thresholds"], n, t["leaves"]
    return thr, nl, lf


def check_model(model, b, trees, what):
    thr, nl, lf = tables(trees)
    assert np.array_equal(model["nleaf"][b].cpu().numpy(), nl), what                      # exact
    assert np.array_equal(model["thresholds"][b].cpu().numpy(), thr), what                # exact, padding included
    got = model["leaves"][b].cpu().numpy()
    err = max(rel(got[e, :nl[e]], lf[e, :nl[e]]) for e in range(len(trees)))
    print(f"{what}: leaves {nl.tolist()}, leaf parameters {err:.2e} relative")
    assert err <= TOL_REL, what


@pytest.mark.parametrize("h,w,p,q", DMS_CASES, ids=DMS_IDS)
def test_dms_stages_vs_restatement(RB, L, h, w, p, q):
    lst, nf, counts, out, info = dms_reference(h, w, p, q)
    H, W = fine_shape(h, w, p, q)
    a, c = dev(lst), dev(nf)
    # stage 1: mean and std, and the fourth power without the std
    mean, std = RB.dms_aggregate(c, coarse=(h, w))
    m, s_ = mean[0].cpu().numpy(), std[0].cpu().numpy()
    assert np.isnan(info["mean"]).sum() == 1                                               # the all-NaN cell
    assert np.array_equal(np.isnan(m), np.isnan(info["mean"])) and np.array_equal(np.isnan(s_), np.isnan(info["std"]))
    ok = ~np.isnan(m)
    assert rel(m[ok], info["mean"][ok]) <= TOL_REL and rel(s_[ok], info["std"][ok]) <= TOL_REL
    srr = dev(info["sr"])
    m4 = torch.empty((1, h, w), dtype=F64, device="cuda")
    L.call("sifsrh_aggregate", srr, m4, None, 1, h, w, H, W, 1, S())
    r4 = R.aggregate(info["sr"], (h, w), pow4=True)[0]
    assert np.array_equal(np.isnan(m4[0].cpu().numpy()), np.isnan(r4)) and rel(m4[0].cpu().numpy()[ok], r4[ok]) <= TOL_REL
    # stage 4 on the restatement's trees, stage 5 on the restatement's image
    thr, nl, lf = (torch.from_numpy(t)[None].cuda() for t in tables(info["trees"]))
    sr = torch.empty((1, 1, H, W), device="cuda")
    L.call("sifsrh_predict", c, thr, nl, lf, sr, 1, E, H, W, S())
    check_raster(sr[0, 0].cpu().numpy(), info["sr"], f"predict {h}x{w} {p}/{q}")
    got = torch.empty_like(srr)
    L.call("sifsrh_correct", a, srr, m4, got, 1, h, w, H, W, S())
    check_raster(got[0, 0].cpu().numpy(), out, f"correct {h}x{w} {p}/{q}")
    assert np.isnan(out).sum() > np.isnan(info["sr"]).sum()                                # the NaN cell spreads over its cubic footprint


@pytest.mark.parametrize("h,w,p,q", DMS_CASES, ids=DMS_IDS)
def test_dms_end_to_end_vs_restatement(RB, h, w, p, q):
    lst, nf, counts, out, info = dms_reference(h, w, p, q)
    H, W = fine_shape(h, w, p, q)
    cnt = torch.from_numpy(counts.copy())[None].cuda()
    got, model = RB.dms(dev(lst), dev(nf), counts=cnt, return_model=True)
    assert got.shape == (1, 1, H, W) and got.dtype == torch.float32
    check_model(model, 0, info["trees"], f"dms {h}x{w} {p}/{q}")
    check_raster(got[0, 0].cpu().numpy(), out, f"dms {h}x{w} {p}/{q}")
    plain = RB.dms(dev(lst), dev(nf), counts=cnt, correct=False)
    check_raster(plain[0, 0].cpu().numpy(), info["sr"], f"dms uncorrected {h}x{w} {p}/{q}")


def test_dms_one_estimator_and_too_few_cells(RB):
    """n_estimators = 1 with given counts; an image with fewer than 10 usable cells comes out all NaN, and the image beside it in
    the batch is its single-image result"""
    h, w, p, q = 6, 8, 5, 2
    lst, nf, counts, out, info = dms_reference(h, w, p, q, n_est=1)
    got, model = RB.dms(dev(lst), dev(nf), n_estimators=1, counts=torch.from_numpy(counts.copy())[None].cuda(), return_model=True)
    check_model(model, 0, info["trees"], "dms one estimator")
    check_raster(got[0, 0].cpu().numpy(), out, "dms one estimator")
    few = lst.copy()
    few.ravel()[9:] = 0.0                                                                  # 9 cells left
    ref, rinfo = R.dms(few, nf, counts)
    assert rinfo["ts"]["n_train"] == 0 and np.isnan(ref).all()
    both = RB.dms(dev(np.stack([few, lst])), dev(np.stack([nf, nf])), n_estimators=1, seed=3)
    one = RB.dms(dev(lst), dev(nf), n_estimators=1, seed=3)
    assert torch.isnan(both[0]).all() and bit_equal(both[1:2].contiguous(), one)


# ---- 4. the access widths ----------------------------------------------------------------------------------------------------------
def test_every_access_width_gives_the_same_bits(RB):
    """W = 40 with the bases aligned takes the 16-byte path; the same rasters one float into an aligned buffer take the scalar
    path and two floats in the 8-byte path; W = 30 takes the 8-byte path and W = 15, 21 the scalar one by their pitch"""
    h, w, s = 5, 5, 8
    lst, nc, nf = make_inputs(h, w, s, 1, 9)
    a, b = dev(lst), dev(nc)
    counts = torch.from_numpy(make_counts(lst, nf, 4, 2))[None].cuda()
    model = RB.dms_model(a, dev(nf), n_estimators=2, counts=counts)
    runs = {"tsharp": lambda c: RB.tsharp(a, b, c), "atprk": lambda c: RB.atprk(a, b, c, variogram=VARIO),
            "aatprk": lambda c: RB.aatprk(a, b, c, variogram=VARIO), "dms": lambda c: RB.dms_apply(model, a, c),
            "dms uncorrected": lambda c: RB.dms_apply(model, a, c, correct=False)}
    for name, fn in runs.items():
        wide = fn(dev(nf))
        assert wide.data_ptr() % 16 == 0
        for off in (1, 2, 3):
            assert bit_equal(wide, fn(dev(nf, offset=off))), (name, off)
    # and an output that is off its alignment, through the entry point itself
    fit = torch.empty((1, 2), dtype=F64, device="cuda")
    RB._lib.call("sifsrb_linfit", a, b, fit, 1, h, w, 285.0, S())
    delta = torch.from_numpy(np.random.RandomState(2).standard_normal((1, h, w))).cuda()
    lam = torch.from_numpy(RB.kriging_weights(*VARIO, 926.0, s)[None].copy()).cuda()
    outs = []
    for off in (0, 1, 2):
        c, o = dev(nf, offset=off), dev(np.zeros_like(nf), offset=off)
        RB._lib.call("sifsrh_sharpen", a, c, fit, delta, lam, o, 1, h, w, 8 * h, 8 * w, 1, S())
        outs.append(o.clone())
    assert bit_equal(outs[0], outs[1]) and bit_equal(outs[0], outs[2])
    for (hh, ww, p) in ((5, 5, 3), (7, 6, 5), (5, 7, 3)):                                  # pitches 15, 30, 21
        lst, nc, nf = make_inputs(hh, ww, p, 1, 3)
        ref, _ = R.atprk(*(x.astype(np.float64) for x in (lst, nc, nf)), VARIO, 926.0, 285.0)
        check_raster(host(RB.atprk(dev(lst), dev(nc), dev(nf), variogram=VARIO))[0, 0], ref, f"atprk pitch {ww * p}")


# ---- 5. batches, repeats, and x4 beside sifsr.baselines ----------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,p,q", [(7, 6, 3, 1), (6, 8, 5, 2)], ids=["x3", "5over2"])
def test_batch_rows_are_their_single_image_results(RB, h, w, p, q):
    trip = [make_inputs(h, w, p, q, s, zeros=z) for s, z in ((1, False), (2, True), (3, False))]
    a, b, c = (dev(np.stack([t[k] for t in trip])) for k in range(3))
    H, W = fine_shape(h, w, p, q)
    runs = [("tsharp", lambda x, y, z: RB.tsharp(x, y, z, min_T=273.0)), ("dms", lambda x, y, z: RB.dms(x, z, seed=11))]
    if q == 1:
        runs += [("atprk", lambda x, y, z: RB.atprk(x, y, z, min_T=273.0)), ("aatprk", lambda x, y, z: RB.aatprk(x, y, z, min_T=273.0)),
                 ("atprk given", lambda x, y, z: RB.atprk(x, y, z, variogram=VARIO))]
    for name, fn in runs:
        whole = fn(a, b, c)
        assert whole.shape == (3, 1, H, W) and whole.dtype == torch.float32
        assert bit_equal(whole, fn(a, b, c)), name                                        # two runs, the same bits
        for r in range(3):
            one = fn(a[r:r + 1].contiguous(), b[r:r + 1].contiguous(), c[r:r + 1].contiguous())
            assert bit_equal(whole[r:r + 1].contiguous(), one), (name, r)
        assert not bit_equal(whole[0], whole[2])


def test_at_four_times_the_functions_agree_with_baselines(RB, sifsr):
    """H == 4h: the same inputs through sifsr.baselines; bit-equality is not required (the x4 kernels contract products into sums
    and the x4 DMS correction uses the exact x4 bicubic coefficients), the families' bar is"""
    BL = sifsr.baselines
    lst, nc, nf = make_inputs(9, 12, 4, 1, 21)
    a, b, c = dev(lst), dev(nc), dev(nf)
    counts = torch.from_numpy(make_counts(lst, nf, 6, E))[None].cuda()
    pairs = {"tsharp": (RB.tsharp(a, b, c), BL.tsharp(a, b, c)),
             "atprk": (RB.atprk(a, b, c), BL.atprk(a, b, c)),
             "aatprk": (RB.aatprk(a, b, c), BL.aatprk(a, b, c)),
             "dms": (RB.dms(a, c, counts=counts), BL.dms(a, c, counts=counts)),
             "dms uncorrected": (RB.dms(a, c, counts=counts, correct=False), BL.dms(a, c, counts=counts, correct=False))}
    for name, (new, old) in pairs.items():
        err = check_raster(new[0, 0].cpu().numpy(), old[0, 0].cpu().numpy(), f"x4 {name}: rbaselines against baselines")
        print(f"x4 {name}: {'bit-equal' if bit_equal(new, old) else 'not bit-equal'}, max difference {err:.3e} K")
    m_new, s_new = RB.dms_aggregate(c, coarse=(9, 12))
    m_old, s_old = BL.dms_aggregate(c)
    assert bit_equal(m_new, m_old) and bit_equal(s_new, s_old)                             # the same sums in the same order


# ---- 6. memory contract ---------------------------------------------------------------------------------------------------------
# (B, h, w, p, q): an odd pitch, a 2-mod-4 pitch with a rational ratio, more than one 256-column workgroup with pitch 260
CONTRACT_SHAPES = [(2, 5, 7, 3, 1), (1, 6, 8, 5, 2), (2, 6, 130, 2, 1)]


def _f64(k, name, *shape, scale=1.0, shift=0.0):
    return k.t(name, torch.from_numpy(k.rs.standard_normal(shape) * scale + shift))


def _fit(k, B):
    return k.t("fit", torch.from_numpy(np.stack([k.rs.uniform(305, 315, B), k.rs.uniform(-15, -9, B)], 1)))


def aggregate(pow4, with_std):
    def make(B, h, w, p, q):
        H, W = fine_shape(h, w, p, q)

        def case(k):
            fine = k.i("fine", B, H, W, scale=0.3, shift=0.4)
            mean = k.o("mean", B, h, w, dtype=F64)
            std = k.o("std", B, h, w, dtype=F64) if with_std else None
            outs = {"mean": mean, "std": std} if with_std else {"mean": mean}
            return (lambda: k.L.call("sifsrh_aggregate", fine, mean, std, B, h, w, H, W, pow4, S())), outs
        return case
    return make


def sharpen(mode):
    def make(B, h, w, p, q):
        H, W = fine_shape(h, w, p, q)

        def case(k):
            lst = k.i("lst", B, h, w, scale=5.0, shift=300.0)
            nf = k.i("ndvi_f", B, H, W, scale=0.3, shift=0.4)
            coef = _f64(k, "coef", B, 2, h, w, shift=5.0) if mode == 2 else _fit(k, B)
            delta = _f64(k, "delta", B, h, w)
            lam = _f64(k, "lambdas", B, p * p, 25, scale=0.1) if mode else None
            out = k.o("out", B, H, W)
            return (lambda: k.L.call("sifsrh_sharpen", lst, nf, coef, delta, lam, out, B, h, w, H, W, mode, S())), {"out": out}
        return case
    return make


def predict(B, h, w, p, q):
    H, W = fine_shape(h, w, p, q)

    def case(k):
        nf = k.i("ndvi_f", B, H, W, scale=0.3, shift=0.4)
        thr = k.t("thresholds", torch.from_numpy(np.sort(k.rs.uniform(-0.5, 1.2, (B, 3, 29)), axis=2)))
        nleaf = k.t("nleaf", torch.from_numpy(k.rs.randint(1, 31, (B, 3)).astype(np.int32)))
        leaves = _f64(k, "leaves", B, 3, 30, 4, scale=3.0, shift=300.0)
        sr = k.o("sr", B, H, W)
        return (lambda: k.L.call("sifsrh_predict", nf, thr, nleaf, leaves, sr, B, 3, H, W, S())), {"sr": sr}
    return case


def correct(B, h, w, p, q):
    H, W = fine_shape(h, w, p, q)

    def case(k):
        lst = k.i("lst", B, h, w, scale=5.0, shift=300.0)
        sr = k.i("sr", B, H, W, scale=5.0, shift=300.0)
        m4 = _f64(k, "m4", B, h, w, scale=1e8, shift=8.1e9)
        out = k.o("out", B, H, W)
        return (lambda: k.L.call("sifsrh_correct", lst, sr, m4, out, B, h, w, H, W, S())), {"out": out}
    return case


CONTRACT = {
    "sifsrh_aggregate": [aggregate(p4, sd)(*s) for p4, sd in ((0, True), (1, False)) for s in CONTRACT_SHAPES],
    "sifsrh_sharpen": [sharpen(m)(*s) for m in (0, 1, 2) for s in CONTRACT_SHAPES if m == 0 or s[4] == 1],
    "sifsrh_predict": [predict(*s) for s in CONTRACT_SHAPES],
    "sifsrh_correct": [correct(*s) for s in CONTRACT_SHAPES],
}
CONTRACT_CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CONTRACT_CASES, ids=[f"{n[7:]}-{i}" for n, i in CONTRACT_CASES])
def test_memory_contract(RB, L, name, idx):
    """every output fully written -- NaN-free under the NaN poison, bit-identical under every poison --, inputs untouched, nothing
    outside the buffers written, and the same bits on ordinary allocations"""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=64 << 20)


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_errors(sifsr, RB, L):
    lst, nc, nf = make_inputs(8, 8, 3, 1, 3)
    a, b, c = dev(lst), dev(nc), dev(nf)
    Err = sifsr.SifsrError
    for fn in (RB.tsharp, RB.atprk, RB.aatprk):
        with pytest.raises(Err):
            fn(a.cpu(), b, c)                                                  # no CPU path
        with pytest.raises(Err):
            fn(a, b, c.cpu())
        with pytest.raises(ValueError, match="per-axis"):
            fn(a, b, c[:, :, :16].contiguous())
        with pytest.raises(ValueError):
            fn(a, b[:, :, :, :7].contiguous(), c)
        with pytest.raises(ValueError, match="at least 5 x 5"):
            fn(a[:, :, :4].contiguous(), b[:, :, :4].contiguous(), c[:, :, :12].contiguous())
    with pytest.raises(ValueError, match="at most 8"):
        RB.tsharp(a[:, :, :5, :5].contiguous(), b[:, :, :5, :5].contiguous(), torch.zeros((1, 1, 45, 45), device="cuda"))
    with pytest.raises(ValueError):
        RB.atprk(a, b, c, variogram=np.ones((2, 2)))
    with pytest.raises(Err, match="image 0"):
        RB.atprk(a, b, c, variogram=(float("nan"), 1000.0))
    with pytest.raises(ValueError, match="b_radius"):
        RB.aatprk(a, b, c, b_radius=0)
    with pytest.raises(ValueError, match="n_estimators"):
        RB.dms(a, c, n_estimators=33)
    with pytest.raises(sifsr.SifsrError):                                      # sifsr.baselines keeps refusing x3
        sifsr.baselines.tsharp(a.cpu(), b, c)
    with pytest.raises(ValueError, match="exactly 4x"):
        sifsr.baselines.tsharp(a, b, c)
    # the C entry points: nothing launched for a bad shape / null pointer (the poisoned output keeps every bit)
    out = torch.full((1, 1, 24, 24), float("nan"), device="cuda")
    f64 = torch.full((1, 2, 8, 8), float("nan"), dtype=F64, device="cuda")
    h = L.lib()
    p = lambda t: t.data_ptr()
    assert h.sifsrh_sharpen(p(a), p(c), p(f64), p(f64), None, p(out), 1, 8, 8, 24, 24, 1, S()) == ARG_ERR
    assert h.sifsrh_sharpen(p(a), p(c), p(f64), p(f64), None, p(out), 1, 8, 8, 24, 24, 3, S()) == ARG_ERR
    assert h.sifsrh_sharpen(p(a), p(c), p(f64), p(f64), None, p(out), 1, 8, 8, 24, 16, 0, S()) == SHAPE_ERR     # per-axis
    assert h.sifsrh_sharpen(p(a), p(c), p(f64), p(f64), None, p(out), 1, 8, 8, 8, 8, 0, S()) == SHAPE_ERR       # ratio 1
    assert h.sifsrh_sharpen(p(a), p(c), p(f64), p(f64), None, p(out), 1, 2, 2, 18, 18, 0, S()) == SHAPE_ERR     # ratio 9
    assert h.sifsrh_sharpen(p(a), p(c), p(f64), p(f64), p(f64), p(out), 1, 8, 8, 20, 20, 1, S()) == SHAPE_ERR   # kriging at 5 / 2
    assert h.sifsrh_sharpen(p(a), p(c), p(f64), p(f64), p(f64), p(out), 1, 4, 8, 12, 24, 1, S()) == SHAPE_ERR   # h < 5
    assert h.sifsrh_aggregate(p(c), None, None, 1, 8, 8, 24, 24, 0, S()) == ARG_ERR
    assert h.sifsrh_aggregate(p(c), p(f64), None, 1, 8, 7, 20, 18, 0, S()) == SHAPE_ERR                         # 5 / 2, odd width
    assert h.sifsrh_predict(p(c), p(f64), p(f64), p(f64), p(out), 1, 33, 24, 24, S()) == SHAPE_ERR
    assert h.sifsrh_predict(p(c), p(f64), None, p(f64), p(out), 1, 3, 24, 24, S()) == ARG_ERR
    assert h.sifsrh_correct(p(a), p(c), p(f64), p(out), 1, 8, 8, 24, 32, S()) == SHAPE_ERR
    assert h.sifsrh_correct(p(a), p(c), None, p(out), 1, 8, 8, 24, 24, S()) == ARG_ERR
    assert h.sifsrh_correct(p(a) + 2, p(c), p(f64), p(out), 1, 8, 8, 24, 24, S()) == ARG_ERR                    # lst off its alignment
    assert h.sifsrh_sharpen(p(a) + 2, p(c), p(f64), p(f64), None, p(out), 1, 8, 8, 24, 24, 0, S()) == ARG_ERR
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(f64).all()
