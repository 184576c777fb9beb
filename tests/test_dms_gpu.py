"""GPU: the DMS sharpener (include/sifsr_dms.h, sifsr/baselines.py) on the device.

  * every stage against the float64 restatement tests/dms_reference.py (pinned by tests/test_dms_host.py to a live scikit-learn and
    to the reference's own tree class) at the coarse shapes where a path changes: (4,4) the root is a leaf, (5,7) one split is
    possible, (16,16), (17,23) no multiple of a wavefront, (64,64) the golden pairs,
  * end to end against tests/golden/golden_dms_v1.npz (the reference's tree class inside BaggingRegressor),
  * batch rows bit-equal to single-image calls, the same seed the same bits, an image with fewer than 10 good cells all NaN,
  * the memory contract of every writing entry point in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is the
    table tests/test_capi_gate.py checks against the header), the argument errors and the drop-in name.

Bounds.  Tree structure (thresholds, leaf counts): exact.  Rasters: 1e-4 K, the bar tests/test_baselines_gpu.py applies to TsHARP
against its restatement (float64 arithmetic, one float32 rounding, spacing 3.05e-5 K at 256..512 K).  float64 stage outputs:
1e-9 relative (sums of at most a few thousand terms; the weights, a ratio of differences in [0, 1], 1e-9 absolute).  None was
taken from what the kernels give.  Every fit is far from a tie in the restatement (asserted: proxy gap >= 1e-10, frontier gap
>= 1e-6), so a different float64 summation order cannot change a tree."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import dms_reference as R
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_dms_v1.npz")
F64 = torch.float64
TOL_K, TOL_REL = 1e-4, 1e-9
PROXY_GAP, HEAP_GAP = 1e-10, 1e-6
SHAPE_ERR, ARG_ERR = 1001, 1002
E = 10
# coarse shape -> (input seed, bootstrap seed), screened on the CPU so that the restatement's fits are far from a tie
SHAPES = {(4, 4): (1, 1), (5, 7): (1, 1), (16, 16): (1, 1), (17, 23): (1, 1)}


@pytest.fixture(scope="module")
def BL(sifsr):
    from sifsr import baselines
    return baselines


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def dev(a):
    """(h,w) or (B,h,w) numpy -> (B,1,h,w) float32 device tensor"""
    a = np.array(a, dtype=np.float32)                               # a copy: the shared references are read-only
    return torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a[None]))[:, None].contiguous().cuda()


def make_case(h, w, seed):
    """seeded float32 (lst (h,w), ndvi_fine (4h,4w)): a smooth index, lst = 312 - 14 mean + a smooth residual + noise; one NaN and
    one 0 K cell, one NaN fine pixel, cell (2,1) of negative mean NDVI, cell (0,1) a copy of cell (0,0) (duplicate feature)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:4 * h, 0:4 * w].astype(np.float64)
    p = rs.uniform(0, 1, 4)
    nf = 0.4 + 0.3 * np.sin(2 * np.pi * (yy / 37 + p[0])) * np.cos(2 * np.pi * (xx / 29 + p[1])) \
        + 0.12 * np.sin(2 * np.pi * (yy / 11 + xx / 13 + p[2])) + 0.03 * rs.standard_normal((4 * h, 4 * w))
    nf = np.clip(nf, -1, 1)
    nf[8:12, 4:8] = -0.3 + 0.05 * rs.standard_normal((4, 4))
    nf[0:4, 4:8] = nf[0:4, 0:4]
    nf = nf.astype(np.float32)
    mean, _ = R.aggregate(nf)
    lst = 312 - 14 * mean + 1.5 * np.sin(2 * np.pi * (np.mgrid[0:h, 0:w][0] / 7 + p[3])) + 0.4 * rs.standard_normal((h, w))
    lst = lst.astype(np.float32)
    lst[1, 2], lst[3, 0] = np.nan, 0.0
    nf[13, 9] = np.nan
    return lst, nf


def make_counts(lst, nf, seed, n_est=E):
    """(E, h*w) bootstrap multiplicities in cell order: n_train draws among the good cells per estimator"""
    mean, std = R.aggregate(nf)
    ts = R.training_set(lst, mean, std)
    idx = np.flatnonzero(ts["good"].ravel())
    rs = np.random.RandomState(seed)
    counts = np.zeros((n_est, lst.size), dtype=np.int64)
    for e in range(n_est):
        counts[e, idx] = np.bincount(rs.randint(0, idx.size, idx.size), minlength=idx.size)
    return counts


_REF = {}


def reference(h, w):
    """(lst, nf, counts, restatement's corrected image, info) for a shape, computed once and shared (read-only)"""
    if (h, w) not in _REF:
        s_in, s_boot = SHAPES[(h, w)]
        lst, nf = make_case(h, w, s_in)
        counts = make_counts(lst, nf, s_boot)
        out, info = R.dms(lst, nf, counts)
        for t in info["trees"]:
            assert t["proxy_gap"] >= PROXY_GAP and t["heap_gap"] >= HEAP_GAP, (h, w, t["proxy_gap"], t["heap_gap"])
            assert np.unique(t["values"]).size == t["values"].size
        for a in (lst, nf, counts, out):
            a.setflags(write=False)
        _REF[(h, w)] = lst, nf, counts, out, info
    return _REF[(h, w)]


def tables(trees):
    """restatement trees -> (thresholds (E,29), nleaf (E,), leaves (E,30,4)) as sifsrd_fit lays them out"""
    thr = np.full((len(trees), 29), np.inf)
    nl = np.zeros(len(trees), dtype=np.int32)
    lf = np.zeros((len(trees), 30, 4))
    for e, t in enumerate(trees):
        n = t["leaves"].shape[0]
        thr[e, :n - 1], nl[e], lf[e, :n] = t["thresholds"], n, t["leaves"]
    return thr, nl, lf


def rel(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max()) if a.size else 0.0


def check_model(model, b, trees, what):
    thr, nl, lf = tables(trees)
    assert np.array_equal(model["nleaf"][b].cpu().numpy(), nl), what                      # exact
    assert np.array_equal(model["thresholds"][b].cpu().numpy(), thr), what                # exact, padding included
    got = model["leaves"][b].cpu().numpy()
    err = max(rel(got[e, :nl[e]], lf[e, :nl[e]]) for e in range(len(trees)))
    print(f"{what}: leaves {nl.tolist()}, leaf parameters {err:.2e} relative")
    assert err <= TOL_REL, what
    assert all((got[e, nl[e]:] == 0).all() for e in range(len(trees)))


def check_raster(got, ref, what):
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = float(np.nanmax(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) if (~np.isnan(ref)).any() else 0.0
    print(f"{what}: max |out - ref| = {err:.3e} K, {int(np.isnan(ref).sum())} NaN pixels")
    assert err <= TOL_K, what


# ---- 1. the stages against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", list(SHAPES))
def test_aggregate_and_training_set(BL, h, w):
    lst, nf, _, _, info = reference(h, w)
    ts = info["ts"]
    mean, std = BL.dms_aggregate(dev(nf))
    rm, rs_ = R.aggregate(nf)
    m, s = mean[0].cpu().numpy(), std[0].cpu().numpy()
    assert np.array_equal(np.isnan(m), np.isnan(rm)) and rel(m, rm) <= TOL_REL and rel(s, rs_) <= TOL_REL
    got = BL.dms_training_set(dev(lst), dev(nf))
    good = got["good"][0].cpu().numpy().reshape(h, w)
    assert np.array_equal(good, ts["good"]) and int(got["n_train"][0]) == ts["n_train"] == h * w - 3
    x = got["x"][0].cpu().numpy().reshape(h, w)
    assert np.array_equal(x.astype(np.float32)[good], ts["x"].astype(np.float32)[good])   # the feature the trees sort by: exact
    assert rel(x[good], ts["x"][good]) <= TOL_REL
    assert rel(got["cv"][0].cpu().numpy().reshape(h, w)[good], ts["cv"][good]) <= TOL_REL
    assert abs(float(got["threshold"][0]) - ts["thr"]) <= TOL_REL * ts["thr"]
    wgt = got["weight"][0].cpu().numpy().reshape(h, w)
    assert np.abs(wgt - ts["w"]).max() <= TOL_REL and (wgt[~good] == 0).all()
    assert (wgt[good] == 0).sum() == 1 and wgt[good].max() <= 1.0                          # the least homogeneous cell gets 0
    # fine^4, without the std
    m4 = torch.empty((1, h, w), dtype=F64, device="cuda")
    BL._lib.call("sifsrd_aggregate", dev(info["sr"]), m4, None, 1, h, w, 1, S())
    assert rel(m4[0].cpu().numpy(), R.aggregate(info["sr"], pow4=True)[0]) <= TOL_REL


@pytest.mark.parametrize("h,w", list(SHAPES))
def test_fit(BL, h, w):
    lst, nf, counts, _, info = reference(h, w)
    model = BL.dms_model(dev(lst), dev(nf), counts=torch.from_numpy(counts.copy())[None].cuda())
    check_model(model, 0, info["trees"], f"fit {h}x{w}")
    nl = model["nleaf"][0].cpu().numpy()
    if (h, w) == (4, 4):
        assert (nl == 1).all()                                                             # fewer than 20 samples: one ridge
    if (h, w) == (5, 7):
        assert nl.max() == 2 and nl.min() >= 1                                             # one split possible
    if (h, w) == (17, 23):
        assert nl.max() > 8


@pytest.mark.parametrize("h,w", list(SHAPES))
def test_predict_and_correct(L, h, w):
    lst, nf, _, out, info = reference(h, w)
    thr, nl, lf = (torch.from_numpy(a)[None].cuda() for a in tables(info["trees"]))
    a, c = dev(lst), dev(nf)
    sr = torch.empty((1, 1, 4 * h, 4 * w), device="cuda")
    L.call("sifsrd_predict", c, thr, nl, lf, sr, 1, E, h, w, S())
    check_raster(sr[0, 0].cpu().numpy(), info["sr"], f"predict {h}x{w}")
    assert np.isnan(info["sr"]).sum() == 1
    srr = dev(info["sr"])                                                                 # stage 5 on the restatement's image
    m4 = torch.empty((1, h, w), dtype=F64, device="cuda")
    L.call("sifsrd_aggregate", srr, m4, None, 1, h, w, 1, S())
    got = torch.empty_like(srr)
    L.call("sifsrd_correct", a, srr, m4, got, 1, h, w, S())
    check_raster(got[0, 0].cpu().numpy(), out, f"correct {h}x{w}")
    assert np.isnan(out).sum() > 16                                                       # the NaN cell spreads over its cubic footprint


@pytest.mark.parametrize("h,w", list(SHAPES))
def test_end_to_end_vs_restatement(BL, h, w):
    lst, nf, counts, out, info = reference(h, w)
    got, model = BL.dms(dev(lst), dev(nf), counts=torch.from_numpy(counts.copy())[None].cuda(), return_model=True)
    assert got.shape == (1, 1, 4 * h, 4 * w) and got.dtype == torch.float32
    check_model(model, 0, info["trees"], f"dms {h}x{w}")
    check_raster(got[0, 0].cpu().numpy(), out, f"dms {h}x{w}")
    plain = BL.dms(dev(lst), dev(nf), counts=torch.from_numpy(counts.copy())[None].cuda(), correct=False)
    check_raster(plain[0, 0].cpu().numpy(), info["sr"], f"dms uncorrected {h}x{w}")


# ---- 2. against the reference's own trees -----------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_vs_golden(BL, golden, i):
    lst, nf, counts = golden[f"c{i}_lst"], golden[f"c{i}_ndvi_fine"], golden[f"c{i}_counts"].astype(np.int64)
    sr, model = BL.dms(dev(lst), dev(nf), counts=torch.from_numpy(counts.copy())[None].cuda(), correct=False, return_model=True)
    nl = golden[f"c{i}_nleaf"]
    assert np.array_equal(model["nleaf"][0].cpu().numpy(), nl)
    assert np.array_equal(model["thresholds"][0].cpu().numpy(), golden[f"c{i}_thresholds"])
    got, err = model["leaves"][0].cpu().numpy(), 0.0
    for e in range(E):
        g = golden[f"c{i}_leaves"][e, :nl[e]].copy()
        r = g[:, 3] - g[:, 2]
        g[:, 2], g[:, 3] = g[:, 2] - 0.25 * r, g[:, 3] + 0.25 * r
        err = max(err, rel(got[e, :nl[e]], g))
    print(f"golden case {i}: leaf parameters {err:.2e} relative")
    assert err <= TOL_REL
    ref = golden[f"c{i}_pred"]
    img = sr[0, 0].cpu().numpy()
    check_raster(img if ref.shape == img.shape else img[1::4, 2::4], ref, f"golden case {i}")
    if i < 2:                                                                              # and the corrected image, the golden pairs
        out = BL.dms(dev(lst), dev(nf), counts=torch.from_numpy(counts.copy())[None].cuda())
        check_raster(out[0, 0].cpu().numpy(), R.correct(lst, R.dms(lst, nf, counts, do_correct=False)[0]), f"golden case {i} corrected")


# ---- 3. batches, determinism, no model ----------------------------------------------------------------------------------------
def test_batch_rows_are_their_single_image_results(BL):
    trip = [make_case(16, 16, s) for s in (1, 2, 3)]
    trip[1][0][:] = np.nan
    trip[1][0].ravel()[5:14] = 301.5                                                       # 9 good cells: no model
    a, c = (dev(np.stack([t[k] for t in trip])) for k in range(2))
    for kw in ({"seed": 7}, {"seed": 7, "correct": False}, {"seed": 8, "n_estimators": 3}):
        whole, model = BL.dms(a, c, return_model=True, **kw)
        assert whole.shape == (3, 1, 64, 64) and whole.dtype == torch.float32
        again = BL.dms(a, c, **kw)
        assert bit_equal(whole, again), kw                                                 # the same seed: the same bits
        assert model["n_train"].tolist() == [253, 0, 253] and (model["nleaf"][1] == 0).all()
        assert torch.isnan(whole[1]).all()                                                 # fewer than 10 good cells: all NaN
        assert torch.isinf(model["thresholds"][1]).all() and (model["leaves"][1] == 0).all()
        assert (model["counts"][1] == 0).all() and (model["counts"][0].sum(1) == 253).all()
        for r in range(3):
            one, m1 = BL.dms(a[r:r + 1].contiguous(), c[r:r + 1].contiguous(), return_model=True, **kw)
            assert bit_equal(whole[r:r + 1].contiguous(), one), (kw, r)
            for k in ("thresholds", "nleaf", "leaves", "counts"):
                assert bit_equal(model[k][r:r + 1].contiguous(), m1[k]), (kw, r, k)
        assert not bit_equal(whole[0], whole[2])
    assert not bit_equal(BL.dms(a, c, seed=7), BL.dms(a, c, seed=9))


def test_model_then_apply_is_dms(BL):
    lst, nf, counts, _, _ = reference(17, 23)
    a, c, k = dev(lst), dev(nf), torch.from_numpy(counts.copy())[None].cuda()
    model = BL.dms_model(a, c, counts=k)
    assert bit_equal(BL.dms_apply(model, a, c), BL.dms(a, c, counts=k))
    assert bit_equal(BL.dms_apply(model, a, c, correct=False), BL.dms(a, c, counts=k, correct=False))


# ---- 4. memory contract -------------------------------------------------------------------------------------------------------
CONTRACT_SHAPES = [(2, 5, 7), (1, 17, 23), (2, 4, 70)]


def _f64(k, name, *shape, scale=1.0, shift=0.0):
    return k.t(name, torch.from_numpy(k.rs.standard_normal(shape) * scale + shift))


def aggregate(pow4):
    def make(B, h, w):
        def case(k):
            fine = k.i("fine", B, 4 * h, 4 * w, scale=0.2, shift=0.5)
            mean, std = k.o("mean", B, h, w, dtype=F64), k.o("std", B, h, w, dtype=F64)
            return (lambda: k.L.call("sifsrd_aggregate", fine, mean, std, B, h, w, pow4, S())), {"mean": mean, "std": std}
        return case
    return make


def trainset(B, h, w):
    def case(k):
        lst = k.i("lst", B, h, w, scale=5.0, shift=300.0)
        mean, std = _f64(k, "mean", B, h, w, scale=0.2, shift=0.5), _f64(k, "std", B, h, w, scale=0.01, shift=0.05)
        x, cv = k.o("x", B, h, w, dtype=F64), k.o("cv", B, h, w, dtype=F64)
        good = k.o("good", B, h, w, dtype=torch.uint8)
        return (lambda: k.L.call("sifsrd_trainset", lst, mean, std, x, cv, good, B, h, w, S())), {"x": x, "cv": cv, "good": good}
    return case


def weights(B, h, w):
    def case(k):
        N = h * w
        cv = k.t("cv", torch.from_numpy(k.rs.uniform(0.05, 0.5, (B, N))))
        good = k.t("good", torch.from_numpy((k.rs.uniform(0, 1, (B, N)) < 0.9).astype(np.uint8)))
        stats = k.t("stats", torch.from_numpy(np.tile(np.array([0.4, 0.05, 0.5]), (B, 1))))
        wgt = k.o("weight", B, N, dtype=F64)
        return (lambda: k.L.call("sifsrd_weights", cv, good, stats, wgt, B, N, S())), {"weight": wgt}
    return case


def fit(B, h, w):
    def case(k):
        N, n_est = h * w, 3
        n = np.array([N - 2, N][:B] if B > 1 else [N - 1], dtype=np.int32)
        xs = k.t("xs", torch.from_numpy(np.sort(k.rs.uniform(-0.1, 0.9, (B, N)), axis=1)))
        ys = _f64(k, "ys", B, N, scale=4.0, shift=300.0)
        ws = k.t("ws", torch.from_numpy(k.rs.uniform(0.0, 1.0, (B, N))))
        cs = k.t("cs", torch.from_numpy(k.rs.poisson(1.0, (B, n_est, N)).astype(np.int32)))
        nt = k.t("n_train", torch.from_numpy(n))
        nbytes = k.L.call("sifsrd_fit_scratch_bytes", B, n_est, N)
        assert nbytes == B * n_est * ((N * 4 + 7) // 8 * 8 + 3 * (N + 1) * 8)
        scratch = k.A.scratch(nbytes, "scratch")                       # exactly the size the query states
        thr, nl = k.o("thresholds", B, n_est, 29, dtype=F64), k.o("nleaf", B, n_est, dtype=torch.int32)
        lf = k.o("leaves", B, n_est, 30, 4, dtype=F64)
        call = lambda: k.L.call("sifsrd_fit", xs, ys, ws, cs, nt, scratch, thr, nl, lf, B, n_est, N, S())
        return call, {"thresholds": thr, "nleaf": nl, "leaves": lf}
    return case


def _tables(k, B, n_est):
    thr = np.full((B, n_est, 29), np.inf)
    nl = k.rs.randint(1, 31, (B, n_est)).astype(np.int32)
    lf = np.zeros((B, n_est, 30, 4))
    for b in range(B):
        for e in range(n_est):
            n = nl[b, e]
            thr[b, e, :n - 1] = np.sort(k.rs.uniform(0.0, 0.9, n - 1))
            lf[b, e, :n] = np.stack([k.rs.uniform(-20, -5, n), k.rs.uniform(305, 315, n), np.full(n, 290.0), np.full(n, 320.0)], 1)
    return k.t("thresholds", torch.from_numpy(thr)), k.t("nleaf", torch.from_numpy(nl)), k.t("leaves", torch.from_numpy(lf))


def predict(B, h, w):
    def case(k):
        nf = k.i("ndvi_f", B, 4 * h, 4 * w, scale=0.3, shift=0.4)
        thr, nl, lf = _tables(k, B, 5)
        sr = k.o("sr", B, 4 * h, 4 * w)
        return (lambda: k.L.call("sifsrd_predict", nf, thr, nl, lf, sr, B, 5, h, w, S())), {"sr": sr}
    return case


def correct(B, h, w):
    def case(k):
        lst = k.i("lst", B, h, w, scale=3.0, shift=300.0)
        sr = k.i("sr", B, 4 * h, 4 * w, scale=3.0, shift=300.0)
        m4 = k.t("m4", torch.from_numpy(k.rs.uniform(295.0, 305.0, (B, h, w)) ** 4))
        out = k.o("out", B, 4 * h, 4 * w)
        return (lambda: k.L.call("sifsrd_correct", lst, sr, m4, out, B, h, w, S())), {"out": out}
    return case


CONTRACT = {
    "sifsrd_aggregate": [aggregate(p)(*s) for p in (0, 1) for s in CONTRACT_SHAPES],
    "sifsrd_trainset": [trainset(*s) for s in CONTRACT_SHAPES],
    "sifsrd_weights": [weights(*s) for s in CONTRACT_SHAPES],
    "sifsrd_fit": [fit(*s) for s in CONTRACT_SHAPES],
    "sifsrd_predict": [predict(*s) for s in CONTRACT_SHAPES],
    "sifsrd_correct": [correct(*s) for s in CONTRACT_SHAPES],
}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output fully written -- NaN-free under the NaN poison, bit-identical under every poison --, inputs untouched, nothing
    outside the buffers written (the fit's scratch included), and the same bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=64 << 20)


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------
def test_errors(sifsr, BL, L):
    lst, nf = make_case(8, 8, 3)
    a, c = dev(lst), dev(nf)
    Err = sifsr.SifsrError
    with pytest.raises(Err):
        BL.dms(a.cpu(), c)                                                     # no CPU path
    with pytest.raises(Err):
        BL.dms(a, c.cpu())
    with pytest.raises(Err):
        BL.dms(a, c, counts=torch.ones((1, 10, 64), dtype=torch.int32))
    with pytest.raises(ValueError):
        BL.dms(a, c[:, :, :28].contiguous())                                   # fine shape not 4x the coarse one
    with pytest.raises(ValueError):
        BL.dms(a, c, counts=torch.ones((1, 10, 63), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        BL.dms(a, c, counts=torch.ones((1, 10, 64), device="cuda"))            # not an integer tensor
    with pytest.raises(ValueError):
        BL.dms(a, c, n_estimators=33)
    for kw in ({"moving_window_size": 30}, {"predictors": 2}, {"quality": "q.tif"}):
        with pytest.raises(NotImplementedError):
            BL.dms(a, c, **kw)
    with pytest.raises(NotImplementedError):
        BL.dms(a, torch.cat([c, c], 1).contiguous())                           # two predictors
    # the C entry points: nothing launched for a bad shape / null pointer (the poisoned outputs keep every bit)
    out = torch.full((1, 1, 32, 32), float("nan"), device="cuda")
    d = torch.full((1, 30 * 4 * 10), float("nan"), dtype=F64, device="cuda")
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    h = L.lib()
    P = lambda t: t.data_ptr()
    assert h.sifsrd_aggregate(P(c), P(d), None, 1, 0, 8, 0, S()) == SHAPE_ERR
    assert h.sifsrd_aggregate(None, P(d), None, 1, 8, 8, 0, S()) == ARG_ERR
    assert h.sifsrd_trainset(P(a), P(d), None, P(d), P(d), P(i32), 1, 8, 8, S()) == ARG_ERR
    assert h.sifsrd_weights(P(d), P(i32), P(d), P(d), 1, 0, S()) == SHAPE_ERR
    assert h.sifsrd_fit_scratch_bytes(1, 33, 64) == 0 and h.sifsrd_fit_scratch_bytes(1, 10, 0) == 0
    assert h.sifsrd_fit(P(d), P(d), P(d), P(i32), P(i32), None, P(d), P(i32), P(d), 1, 10, 64, S()) == ARG_ERR
    assert h.sifsrd_fit(P(d), P(d), P(d), P(i32), P(i32), P(d), P(d), P(i32), P(d), 1, 0, 64, S()) == SHAPE_ERR
    assert h.sifsrd_predict(P(c), P(d), P(i32), P(d), P(out), 1, 33, 8, 8, S()) == SHAPE_ERR
    assert h.sifsrd_predict(P(c), P(d), None, P(d), P(out), 1, 10, 8, 8, S()) == ARG_ERR
    assert h.sifsrd_correct(P(a), P(c), P(d), None, 1, 8, 8, S()) == ARG_ERR
    assert h.sifsrd_correct(P(a), P(c), P(d), P(out), 1, 8, 0, S()) == SHAPE_ERR
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(d).all() and (i32 == 0).all()


# ---- 6. drop-in --------------------------------------------------------------------------------------------------------------
def test_dropin(sifsr, BL):
    saved = {k: sys.modules.pop(k, None) for k in ("model", "dataset", "utils")}
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        us = importlib.import_module("utils")
        lst, nf, _, _, _ = reference(16, 16)
        out = us.DMS(lst.copy(), nf.copy(), 4, seed=5)
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (64, 64)
        ref = BL.dms(dev(lst), dev(nf), seed=5)[0, 0].cpu().numpy()
        assert np.array_equal(out.astype(np.float32), ref, equal_nan=True)
        with pytest.raises(NotImplementedError, match="scale"):
            us.DMS(lst, nf, 2)
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v
