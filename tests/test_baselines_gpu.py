"""GPU: the classical sharpening baselines (include/sifsr_baselines.h, sifsr/baselines.py) -- TsHARP, ATPRK and
AATPRK of the reference's utils.py:854-1606 on the device.

  * against the reference's own outputs (tests/golden/golden_baselines_v1.npz, made by tests/golden/make_golden_baselines.py):
    tsharp, the empirical semivariogram, and the kriging methods with the variogram fit taken out (`variogram=` the reference's
    fit 2) at 1e-4 K / 1e-9 relative; the kriging methods with their own fit at the project's parity bar, 1e-4 of the image's max,
  * against the float64 restatement tests/baselines_reference.py (pinned to the same golden by tests/test_baselines_host.py) at
    the shapes where the tiling can go wrong,
  * batch rows bit-equal to single-image calls, the window fallback of AATPRK, the uncorrected border of the kriging methods,
  * the memory contract of every writing entry point in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is the
    table tests/test_capi_gate.py checks against the header), and the argument errors.

Bounds.  1e-4 K: the arithmetic before the store is float64, the store rounds once to float32, whose spacing at 256..512 K is
3.05e-5 K -- three of them.  1e-9 relative on the semivariogram: float64 sums of at most a few thousand terms of one sign.  Both
are the issue's and neither was taken from what the kernels give."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import baselines_reference as R
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_baselines_v1.npz")
F64 = torch.float64
TOL_K = 1e-4
SHAPE_ERR, ARG_ERR = 1001, 1002


@pytest.fixture(scope="module")
def BL(sifsr):
    from sifsr import baselines
    return baselines


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def dev(a):
    """(h,w) or (B,h,w) numpy -> (B,1,h,w) float32 device tensor"""
    a = np.asarray(a, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a[None]))[:, None].contiguous().cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def case(golden, i):
    return golden[f"c{i}_lst"], golden[f"c{i}_ndvi_coarse"], golden[f"c{i}_ndvi_fine"]


def make_inputs(h, w, seed, zeros=None):
    """seeded float32 (lst (h,w), ndvi_coarse (h,w), ndvi_fine (4h,4w)): a smooth index in [-1, 1], its norm-L4 pooling, and
    lst = 310 - 12 ndvi_coarse + a smooth residual + noise; `zeros` = (r0, r1, c0, c1) block of lst == 0."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:4 * h, 0:4 * w].astype(np.float64)
    p = rs.uniform(0, 1, 6)
    nf = 0.4 + 0.35 * np.sin(2 * np.pi * (yy / 37 + p[0])) * np.cos(2 * np.pi * (xx / 29 + p[1])) \
        + 0.15 * np.sin(2 * np.pi * (yy / 11 + xx / 13 + p[2])) + 0.03 * rs.standard_normal((4 * h, 4 * w))
    nf = np.clip(nf, -1, 1).astype(np.float32)
    nc = (((nf.astype(np.float64).reshape(h, 4, w, 4) ** 4).sum((1, 3)) / 16) ** 0.25).astype(np.float32)
    cy, cx = np.mgrid[0:h, 0:w].astype(np.float64)
    lst = 310 - 12 * nc.astype(np.float64) + 2.0 * np.sin(2 * np.pi * (cy / 7 + p[3])) * np.cos(2 * np.pi * (cx / 9 + p[4])) \
        + 0.5 * rs.standard_normal((h, w))
    lst = lst.astype(np.float32)
    if zeros:
        lst[zeros[0]:zeros[1], zeros[2]:zeros[3]] = 0.0
    return lst, nc, nf


_REF = {}


def reference(key, fn):
    """the restatement's result for `key`, computed once and shared (read-only)"""
    if key not in _REF:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
        _REF[key] = v
    return _REF[key]


VARIO = (15.5, 4450.0)          # a fine-scale (sill, range) of the size the reference's fits give for these fields


# ---- 1. against the reference's own outputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2])
def test_tsharp_vs_golden(BL, golden, i):
    lst, nc, nf = case(golden, i)
    out = host(BL.tsharp(dev(lst), dev(nc), dev(nf), min_T=float(golden["min_T"])))[0, 0]
    ref = golden[f"c{i}_tsharp"]
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan)                       # NaN exactly where the reference has NaN
    err = np.abs(out - ref)[~nan].max()
    print(f"tsharp case {i}: max |out - ref| = {err:.3e} K, {int(nan.sum())} NaN pixels")
    assert err <= TOL_K
    if i == 2:
        # the case holds what it should: 16 + 16 NaN pixels, and the 96 pixels of the lst == 0 block less the 8 where the NaN
        # block of the fine index overlaps it (NaN * 0 is NaN: the unmixing multiplies by the mask)
        assert nan.sum() == 32 and (ref[~nan] == 0).sum() == 88 and nan[21:25, 42:44].all()


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("method", ["atprk", "aatprk"])
def test_semivariogram_vs_golden(BL, golden, method, i):
    lst, nc, nf = (a.astype(np.float64) for a in case(golden, i))
    a0, a1 = R.linear_fit(lst, nc, float(golden["min_T"])) if method == "atprk" else R.linear_fit_window(lst, nc, float(golden["min_T"]))
    delta = R.residual(lst, nc, a0, a1)
    g = BL.semivariogram(torch.from_numpy(delta)[None, None].cuda()).cpu().numpy()[0]
    ref = golden[f"c{i}_{method}_gamma"]
    assert g.shape == (15,) and g.dtype == np.float64
    assert np.array_equal(g == 0, ref == 0) and ref[0] == 0
    err = np.abs(g - ref)[ref != 0] / np.abs(ref[ref != 0])
    print(f"semivariogram {method} case {i}: max rel err {err.max():.3e}")
    assert err.max() <= 1e-9


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("method", ["atprk", "aatprk"])
def test_kriging_vs_golden_with_the_reference_fit(BL, golden, method, i):
    """`variogram=` the reference's fit 2: everything but the fit, against the reference's image"""
    lst, nc, nf = case(golden, i)
    out, info = getattr(BL, method)(dev(lst), dev(nc), dev(nf), scc=float(golden["scc"]), min_T=float(golden["min_T"]),
                                    variogram=golden[f"c{i}_{method}_fit2"], return_variogram=True)
    ref = golden[f"c{i}_{method}"]
    err = np.abs(host(out)[0, 0] - ref).max()
    lam = np.abs(info["lambdas"][0] - golden[f"c{i}_{method}_lambdas"]).max()
    print(f"{method} case {i}, reference fit: max |out - ref| = {err:.3e} K; max |lambda - ref| = {lam:.3e}")
    assert info["gamma_coarse"] is None and info["fit1"] is None and info["lambdas"].shape == (1, 16, 25)
    assert err <= TOL_K


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("method", ["atprk", "aatprk"])
def test_kriging_vs_golden_with_its_own_fit(BL, golden, method, i):
    """the package's own fits: the image at the project's parity bar (1e-4 of its maximum); the empirical semivariogram it fitted
    at 1e-9.  The fitted parameters are printed, not compared (the image does not depend on the fit path: the reference's own
    image moves by < 1e-4 K when its fit starts elsewhere, asserted by the generator)."""
    lst, nc, nf = case(golden, i)
    out, info = getattr(BL, method)(dev(lst), dev(nc), dev(nf), scc=float(golden["scc"]), min_T=float(golden["min_T"]),
                                    return_variogram=True)
    ref = golden[f"c{i}_{method}"]
    err = np.abs(host(out)[0, 0] - ref).max()
    print(f"{method} case {i}, own fit: fit1 {info['fit1'][0]} fit2 {info['fit2'][0]} (reference {golden[f'c{i}_{method}_fit1']} "
          f"{golden[f'c{i}_{method}_fit2']}); max |out - ref| = {err:.3e} K = {err / np.abs(ref).max():.3e} of the maximum")
    g, gref = info["gamma_coarse"][0], golden[f"c{i}_{method}_gamma"]
    assert info["gamma_coarse"].shape == (1, 15) and info["fit1"].shape == (1, 2) and info["fit2"].shape == (1, 2)
    assert np.abs(g - gref)[1:].max() <= 1e-9 * np.abs(gref[1:]).min() and g[0] == 0
    assert err <= 1e-4 * np.abs(ref).max()


# ---- 2. shapes where the tiling can go wrong, against the restatement -------------------------------------------------------
# coarse (h, w): one interior window; non-square; odd; more than one 64-column block of the sharpening pass (70); more than one
# 16 x 16 tile of windows in both directions of the semivariogram (22 x 37 -> 2 x 3 tiles, the last ones partial)
SHAPES = [(5, 5), (8, 12), (16, 24), (9, 7), (6, 70), (22, 37)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_shapes_vs_restatement(BL, h, w):
    lst, nc, nf = make_inputs(h, w, 100 * h + w, zeros=(1, 3, 2, 4))
    l64, c64, f64 = (a.astype(np.float64) for a in (lst, nc, nf))
    ts = reference(("ts", h, w), lambda: R.tsharp(l64, c64, f64, 285.0))
    at, g_at = reference(("at", h, w), lambda: R.atprk(l64, c64, f64, VARIO, 926.0, 285.0))
    aa, g_aa = reference(("aa", h, w), lambda: R.aatprk(l64, c64, f64, VARIO, 926.0, 285.0))
    a, b, c = dev(lst), dev(nc), dev(nf)
    got = {"tsharp": (host(BL.tsharp(a, b, c))[0, 0], ts),
           "atprk": (host(BL.atprk(a, b, c, variogram=VARIO))[0, 0], at),
           "aatprk": (host(BL.aatprk(a, b, c, variogram=np.array([VARIO])))[0, 0], aa)}
    for name, (out, ref) in got.items():
        assert out.shape == (4 * h, 4 * w) and np.isfinite(ref).all()
        err = np.abs(out - ref).max()
        print(f"{name} {h}x{w}: max |out - restatement| = {err:.3e} K")
        assert err <= TOL_K, name
    d = R.residual(l64, c64, *R.linear_fit(l64, c64, 285.0))
    g = BL.semivariogram(torch.from_numpy(d)[None, None].cuda()).cpu().numpy()[0]
    assert np.array_equal(g == 0, g_at == 0)
    nz = g_at != 0
    assert (np.abs(g - g_at)[nz] / g_at[nz]).max() <= 1e-9
    if (h, w) == (5, 5):
        assert nz[1:].all()                                          # the single window feeds every class


# ---- 3. batches ------------------------------------------------------------------------------------------------------------
def test_batch_rows_are_their_single_image_results(BL):
    trip = [make_inputs(16, 16, s, zeros=z) for s, z in ((1, None), (2, (4, 6, 9, 12)), (3, None))]
    a, b, c = (dev(np.stack([t[k] for t in trip])) for k in range(3))
    for name, kw in (("tsharp", {}), ("atprk", {}), ("aatprk", {}), ("atprk", {"variogram": VARIO})):
        fn = getattr(BL, name)
        whole = fn(a, b, c, min_T=273.0, **kw)
        assert whole.shape == (3, 1, 64, 64) and whole.dtype == torch.float32
        assert bit_equal(whole, fn(a, b, c, min_T=273.0, **kw)), name               # two identical calls
        for r in range(3):
            one = fn(a[r:r + 1].contiguous(), b[r:r + 1].contiguous(), c[r:r + 1].contiguous(), min_T=273.0, **kw)
            assert bit_equal(whole[r:r + 1].contiguous(), one), (name, r)
        assert not bit_equal(whole[0], whole[2])


# ---- 4. AATPRK's fallback ----------------------------------------------------------------------------------------------------
def test_aatprk_window_fallback(BL, L):
    """a 3 x 3 block of lst == 0 centred on (7, 8): every window centred within one pixel of (7, 8) holds the whole block, 16
    valid pixels (<= 2/3 of 25), and takes the global fit; the centres two pixels away see 6 zeros (19 valid) and keep their own."""
    lst, nc, nf = make_inputs(16, 16, 77, zeros=(6, 9, 7, 10))
    l64, c64, f64 = (x.astype(np.float64) for x in (lst, nc, nf))
    a, b, c = dev(lst), dev(nc), dev(nf)
    fit = torch.empty((1, 2), dtype=F64, device="cuda")
    coef = torch.empty((1, 2, 16, 16), dtype=F64, device="cuda")
    L.call("sifsrb_linfit", a, b, fit, 1, 16, 16, 285.0, S())
    L.call("sifsrb_linfit_window", a, b, fit, coef, 1, 16, 16, 2, 285.0, S())
    fit, coef = fit.cpu().numpy()[0], coef.cpu().numpy()[0]
    g0, g1 = R.linear_fit(l64, c64, 285.0)
    w0, w1 = R.linear_fit_window(l64, c64, 285.0, 2)
    assert abs(fit[0] - g0) <= 1e-9 * abs(g0) and abs(fit[1] - g1) <= 1e-9 * abs(g1)
    for y in (6, 7, 8):
        for x in (7, 8, 9):
            assert coef[0, y, x] == fit[0] and coef[1, y, x] == fit[1] and w0[y, x] == g0
    for y, x in ((5, 8), (9, 8), (7, 6), (7, 10)):
        assert coef[0, y, x] != fit[0] and w0[y, x] != g0
    border = np.ones((16, 16), dtype=bool)
    border[2:-2, 2:-2] = False
    assert (coef[0][border] == fit[0]).all() and (coef[1][border] == fit[1]).all()
    assert np.abs(coef[0] - w0).max() <= 1e-7 * np.abs(w0).max() and np.abs(coef[1] - w1).max() <= 1e-7 * np.abs(w1).max()
    ref, _ = R.aatprk(l64, c64, f64, VARIO, 926.0, 285.0)
    err = np.abs(host(BL.aatprk(a, b, c, variogram=VARIO))[0, 0] - ref).max()
    print(f"aatprk with a fallback window: max |out - restatement| = {err:.3e} K")
    assert err <= TOL_K


# ---- 5. the uncorrected border ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,mode", [("atprk", 1), ("aatprk", 2)])
def test_kriging_border_is_the_plain_unmixed_value(BL, L, method, mode):
    lst, nc, nf = make_inputs(9, 12, 5)
    a, b, c = dev(lst), dev(nc), dev(nf)
    out, info = getattr(BL, method)(a, b, c, variogram=VARIO, return_variogram=True)
    fit = torch.empty((1, 2), dtype=F64, device="cuda")
    L.call("sifsrb_linfit", a, b, fit, 1, 9, 12, 285.0, S())
    coef = fit
    if mode == 2:
        coef = torch.empty((1, 2, 9, 12), dtype=F64, device="cuda")
        L.call("sifsrb_linfit_window", a, b, fit, coef, 1, 9, 12, 2, 285.0, S())
    plain = torch.empty_like(out)                                     # residual 0: u + sum(lambda * 0) = u, every pixel
    L.call("sifsrb_sharpen", a, c, coef, torch.zeros((1, 9, 12), dtype=F64, device="cuda"),
           torch.from_numpy(info["lambdas"]).cuda(), plain, 1, 9, 12, mode, S())
    o, p = out[0, 0], plain[0, 0]
    inner = torch.zeros((36, 48), dtype=torch.bool, device="cuda")
    inner[8:-8, 8:-8] = True
    assert bit_equal(o[~inner], p[~inner])
    assert (o[inner] != p[inner]).float().mean().item() > 0.99


# ---- 6. memory contract -------------------------------------------------------------------------------------------------------
CONTRACT_SHAPES = [(2, 9, 7), (1, 22, 37), (2, 6, 70)]


def _f64(k, name, *shape, scale=1.0, shift=0.0):
    return k.t(name, torch.from_numpy(k.rs.standard_normal(shape) * scale + shift))


def _images(k, B, h, w):
    return k.i("lst", B, h, w, scale=5.0, shift=300.0), k.i("ndvi_c", B, h, w, scale=0.3, shift=0.4)


def _fit(k, B):
    return k.t("fit", torch.from_numpy(np.stack([k.rs.uniform(305, 315, B), k.rs.uniform(-15, -9, B)], 1)))


def linfit(B, h, w):
    def case(k):
        lst, nc = _images(k, B, h, w)
        fit = k.o("fit", B, 2, dtype=F64)
        return (lambda: k.L.call("sifsrb_linfit", lst, nc, fit, B, h, w, 285.0, S())), {"fit": fit}
    return case


def linfit_window(B, h, w):
    def case(k):
        lst, nc = _images(k, B, h, w)
        fit = _fit(k, B)
        coef = k.o("coef", B, 2, h, w, dtype=F64)
        return (lambda: k.L.call("sifsrb_linfit_window", lst, nc, fit, coef, B, h, w, 2, 285.0, S())), {"coef": coef}
    return case


def residual(per_pixel):
    def make(B, h, w):
        def case(k):
            lst, nc = _images(k, B, h, w)
            coef = _f64(k, "coef", B, 2, h, w, shift=5.0) if per_pixel else _fit(k, B)
            delta = k.o("delta", B, h, w, dtype=F64)
            return (lambda: k.L.call("sifsrb_residual", lst, nc, coef, per_pixel, delta, B, h, w, S())), {"delta": delta}
        return case
    return make


def semivar(B, h, w):
    def case(k):
        delta = _f64(k, "delta", B, h, w)
        nbytes = k.L.call("sifsrb_semivariogram_scratch_bytes", B, h, w)
        assert nbytes == B * ((h - 4 + 15) // 16) * ((w - 4 + 15) // 16) * 28 * 8
        scratch = k.A.scratch(nbytes, "scratch")                     # exactly the size the query states
        gamma = k.o("gamma", B, 15, dtype=F64)
        call = lambda: k.L.call("sifsrb_semivariogram", delta, scratch, gamma, B, h, w, S())
        return call, {"gamma": gamma, "scratch": scratch.view(F64)}  # the scratch is written in full: NaN-free under every poison
    return case


def sharpen(mode):
    def make(B, h, w):
        def case(k):
            lst = k.i("lst", B, h, w, scale=5.0, shift=300.0)
            nf = k.i("ndvi_f", B, 4 * h, 4 * w, scale=0.3, shift=0.4)
            coef = _f64(k, "coef", B, 2, h, w, shift=5.0) if mode == 2 else _fit(k, B)
            delta = _f64(k, "delta", B, h, w)
            lam = _f64(k, "lambdas", B, 16, 25, scale=0.1) if mode else None
            out = k.o("out", B, 4 * h, 4 * w)
            return (lambda: k.L.call("sifsrb_sharpen", lst, nf, coef, delta, lam, out, B, h, w, mode, S())), {"out": out}
        return case
    return make


CONTRACT = {
    "sifsrb_linfit": [linfit(*s) for s in CONTRACT_SHAPES],
    "sifsrb_linfit_window": [linfit_window(*s) for s in CONTRACT_SHAPES],
    "sifsrb_residual": [residual(p)(*s) for p in (0, 1) for s in CONTRACT_SHAPES],
    "sifsrb_semivariogram": [semivar(*s) for s in CONTRACT_SHAPES + [(1, 5, 5)]],
    "sifsrb_sharpen": [sharpen(m)(*s) for m in (0, 1, 2) for s in CONTRACT_SHAPES],
}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output (and the semivariogram's scratch) fully written -- NaN-free under the NaN poison, bit-identical under every
    poison --, inputs untouched, nothing outside the buffers written, and the same bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=64 << 20)


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------
def test_errors(sifsr, BL, L):
    lst, nc, nf = make_inputs(8, 8, 3)
    a, b, c = dev(lst), dev(nc), dev(nf)
    E = sifsr.SifsrError
    for fn in (BL.tsharp, BL.atprk, BL.aatprk):
        with pytest.raises(E):
            fn(a.cpu(), b, c)                                                  # no CPU path
        with pytest.raises(E):
            fn(a, b, c.cpu())
        with pytest.raises(ValueError):
            fn(a, b, c[:, :, :28].contiguous())                                # fine shape not 4x the coarse one
        with pytest.raises(ValueError):
            fn(a, b[:, :, :, :7].contiguous(), c)
        with pytest.raises(ValueError):
            fn(a[:, :, :4].contiguous(), b[:, :, :4].contiguous(), c[:, :, :16].contiguous())      # h < 5
    with pytest.raises(E):
        BL.semivariogram(torch.zeros((1, 1, 8, 8), dtype=F64))
    with pytest.raises(ValueError):
        BL.semivariogram(torch.zeros((1, 1, 4, 8), dtype=F64, device="cuda"))
    with pytest.raises(ValueError):
        BL.atprk(a, b, c, variogram=np.ones((2, 2)))
    with pytest.raises(E, match="image 0"):
        BL.atprk(a, b, c, variogram=(float("nan"), 1000.0))
    with pytest.raises(E, match="image 0"):
        BL.aatprk(a, b, c, variogram=(7.0, -1.0))
    # the C entry points: nothing launched for a bad shape / null pointer (the poisoned output keeps every bit)
    out = torch.full((1, 1, 32, 32), float("nan"), device="cuda")
    fit = torch.full((1, 2), float("nan"), dtype=F64, device="cuda")
    h = L.lib()
    assert h.sifsrb_linfit(a.data_ptr(), b.data_ptr(), fit.data_ptr(), 1, 4, 8, 285.0, S()) == SHAPE_ERR
    assert h.sifsrb_linfit(a.data_ptr(), None, fit.data_ptr(), 1, 8, 8, 285.0, S()) == ARG_ERR
    assert h.sifsrb_linfit_window(a.data_ptr(), b.data_ptr(), fit.data_ptr(), fit.data_ptr(), 1, 8, 8, 0, 285.0, S()) == SHAPE_ERR
    assert h.sifsrb_sharpen(a.data_ptr(), c.data_ptr(), fit.data_ptr(), fit.data_ptr(), None, out.data_ptr(), 1, 8, 8, 1, S()) == ARG_ERR
    assert h.sifsrb_sharpen(a.data_ptr(), c.data_ptr(), fit.data_ptr(), fit.data_ptr(), None, out.data_ptr(), 1, 8, 8, 3, S()) == ARG_ERR
    assert h.sifsrb_sharpen(a.data_ptr(), c.data_ptr(), fit.data_ptr(), fit.data_ptr(), None, out.data_ptr(), 1, 8, 4, 0, S()) == SHAPE_ERR
    assert h.sifsrb_semivariogram_scratch_bytes(1, 4, 8) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(fit).all()


# ---- 8. drop-in --------------------------------------------------------------------------------------------------------------
def test_dropin(sifsr, golden):
    saved = {k: sys.modules.pop(k, None) for k in ("model", "dataset", "utils")}
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        us = importlib.import_module("utils")
        lst, nd, nf = case(golden, 2)
        out = us.TsHARP(lst, nd, nf, 4, min_T=273)
        ref = golden["c2_tsharp"]
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (64, 64)
        assert np.array_equal(np.isnan(out), np.isnan(ref)) and np.nanmax(np.abs(out - ref)) <= TOL_K
        lst, nd, nf = case(golden, 0)
        for name, extra in (("ATPRK", {}), ("AATPRK", {"b_radius": 2})):
            out = getattr(us, name)(lst, nd, nf, 4, 926, min_T=273, path_image="ignored.tif", **extra)
            ref = golden[f"c0_{name.lower()}"]
            assert out.dtype == np.float64 and np.abs(out - ref).max() <= 1e-4 * np.abs(ref).max()
        with pytest.raises(NotImplementedError, match="block_size"):
            us.ATPRK(lst, nd, nf, 4, 926, block_size=3)
        with pytest.raises(NotImplementedError, match="block_size"):
            us.AATPRK(lst, nd, nf, 4, 926, block_size=3)
        for fn, args in ((us.TsHARP, ()), (us.ATPRK, (926,)), (us.AATPRK, (926,))):
            with pytest.raises(NotImplementedError, match="scale"):
                fn(lst, nd, nf, 2, *args)
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v
