"""The classical sharpening baselines at any ratio: `sifsr.baselines` for a fine raster that is not x4.

    tsharp, dms, dms_model, dms_apply, dms_aggregate      any ratio H / h == W / w == p / q in lowest terms, 1 < p / q <= 8
    atprk, aatprk                                         integer scales s = 2 .. 8 (the reference's `iscale`, utils.py:944-1606)

The functions, their signatures, defaults, NaN and 0 K conventions and error types are those of `sifsr.baselines`; the ratio is read
from the two shapes.  (`dms_aggregate` alone needs the coarse shape beside the raster: `coarse=(h, w)`.)  The cell of fine pixel
(Y, X) is (floor(Y h / H), floor(X w / W)) formed in integers -- the rule of ratio.predict_granule_gaps, rloss.valid_counts and
rconserve -- so at x2.5 a cell holds 2 or 3 pixels per axis.

What reads coarse rasters alone has no ratio in it and is `sifsr.baselines`' own: the regressions, the residual, the empirical
semivariogram, the damped least squares of the two variogram fits, the DMS training set, weights and tree fit.  New are the passes
over the fine raster (csrc/rbaselines.hip, declared in csrc/rbaselines_api.h and bound here, once, on the handle of _lib.lib()) and
the host's kriging geometry, which is a function of the scale s: the fine spacing scc / s, the s^2 x s^2 fine pairs of every pair of
block pixels, the s^2 weight rows.  It is built once per scale and cached; at s = 4 it is `sifsr.baselines`' to the bit.

Area-to-point kriging over cells of unequal size is a different method: atprk and aatprk raise NotImplementedError at a rational
ratio.  Scales 2 and 3 are pinned to the reference's own outputs; scales 5..8 and the rational ratios have no counterpart in the
reference and are held to the float64 restatement tests/rbaselines_reference.py alone.
Transfers per call are `sifsr.baselines`'; CPU tensors raise SifsrError: there is no fallback.
"""
from __future__ import annotations

import functools
import math
import os

import numpy as np
import torch

from . import _lib
from . import baselines as _b4
from .baselines import DMS_MAX_LEAVES, DMS_MIN_TRAIN, KS, LM_MAX_ITER  # noqa: F401

API_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "rbaselines_api.h")
MAX_RATIO, MAX_SCALE = 8, 8
_bound = None


def bound():
    """The `sifsrh_` entry points as bound on the library's handle: {name: (restype, [Arg])} (bound on first use, once)."""
    global _bound
    if _bound is None:
        _bound = _lib.bind_header(API_HEADER)
    return _bound


def _call(name, *args):
    bound()
    return _lib.call(name, *args)


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def geometry(coarse, fine):
    """(h, w), (H, W) -> (p, q): H / h == W / w == p / q in lowest terms.  Raises ValueError naming the rule that fails."""
    (h, w), (H, W) = (int(v) for v in coarse), (int(v) for v in fine)
    if h < 1 or w < 1 or H < 1 or W < 1:
        raise ValueError(f"empty raster: coarse {h} x {w}, fine {H} x {W}")
    g = math.gcd(H, h)
    p, q = H // g, h // g
    if not q < p <= MAX_RATIO * q:
        raise ValueError(f"the ratio H / h = {H} / {h} = {p} / {q} must be above 1 and at most {MAX_RATIO}")
    if w % q:
        raise ValueError(f"at ratio {p} / {q} both coarse sides must be multiples of {q}, got {h} x {w}")
    if W != w // q * p:
        raise ValueError(f"per-axis ratios are not built: H / h = {p} / {q} asks for a fine raster of {H} x {w // q * p}, got {H} x {W}")
    return p, q


def _check(lst, ndvi_coarse, ndvi_fine, kriging):
    for t, what in ((lst, "lst"), (ndvi_coarse, "ndvi_coarse"), (ndvi_fine, "ndvi_fine")):
        if not isinstance(t, torch.Tensor):
            raise _lib.SifsrError(f"{what} must be a device tensor, got {type(t).__name__}")
        _lib.require_gpu(t, what)
        if t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"{what}: expected (B,1,H,W), got {tuple(t.shape)}")
    B, _, h, w = lst.shape
    if tuple(ndvi_coarse.shape) != (B, 1, h, w):
        raise ValueError(f"ndvi_coarse {tuple(ndvi_coarse.shape)} does not match lst {tuple(lst.shape)}")
    if ndvi_fine.shape[0] != B:
        raise ValueError(f"ndvi_fine {tuple(ndvi_fine.shape)} does not match the batch of lst {tuple(lst.shape)}")
    H, W = ndvi_fine.shape[2:]
    p, q = geometry((h, w), (H, W))
    if h < 5 or w < 5:
        raise ValueError(f"the coarse image must be at least 5 x 5 (one kriging block), got {h} x {w}")
    if kriging and q != 1:
        raise NotImplementedError(f"area-to-point kriging is built for integer scales 2..{MAX_SCALE} only, not for the rational "
                                  f"ratio {p} / {q}: over cells of unequal size it is a different method")
    return B, h, w, H, W, p, q


# ---- host kriging geometry, a function of the scale ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _geometry(s):
    """-> (mult ((2s-1)^2,), d_cc (5, 5, (2s-1)^2), d_fc (s^2, 25, s^2)) in units of the fine pixel: the multiplicities and
    distances of the fine offsets inside a pair of coarse pixels, and the distances from the fine pixels of the centre pixel."""
    if not 2 <= s <= MAX_SCALE:
        raise ValueError(f"the scale must be in [2, {MAX_SCALE}], got {s}")
    e = np.arange(-(s - 1), s)
    mult = ((s - np.abs(e))[:, None] * (s - np.abs(e))[None, :] / float(s ** 4)).ravel()
    d_cc = np.sqrt((s * np.arange(5)[:, None, None, None] + e[None, None, :, None]) ** 2
                   + (s * np.arange(5)[None, :, None, None] + e[None, None, None, :]) ** 2).reshape(5, 5, (2 * s - 1) ** 2)
    a = np.stack(np.divmod(np.arange(s * s), s), 1)
    rc = _b4._RC
    d_fc = np.sqrt((s * (rc[None, :, None, 0] - 2) + a[None, None, :, 0] - a[:, None, None, 0]) ** 2
                   + (s * (rc[None, :, None, 1] - 2) + a[None, None, :, 1] - a[:, None, None, 1]) ** 2)
    for v in (mult, d_cc, d_fc):
        v.setflags(write=False)
    return mult, d_cc, d_fc


def _gamma_cc(sill, ran, scc, s):
    mult, d_cc, _ = _geometry(s)
    tab = (_b4._expo(scc / s * d_cc, sill, ran) * mult).sum(-1)
    return tab[_b4._DR, _b4._DC]


def regularised_model(sill, ran, scc=926.0, s=4):
    """Gamma_ff of utils.py:944-975 at the 15 distance classes for scale s; the running division is the reference's."""
    rows = np.einsum("kij,ij->ki", _b4._MEMBER, _gamma_cc(sill, ran, scc, s))
    m = np.zeros(15)
    for i in range(25):
        m = (m + rows[:, i]) / _b4._COUNT[:, i]
    return m - m[0]


def kriging_weights(sill, ran, scc=926.0, s=4):
    """utils.py:1118-1182 at scale s: the (s^2, 25) weights of the 5 x 5 coarse residuals for the s^2 fine pixels of the centre."""
    _, _, d_fc = _geometry(s)
    A = np.zeros((26, 26))
    A[:25, :25] = _gamma_cc(sill, ran, scc, s)
    A[:25, 25] = A[25, :25] = 1.0
    rhs = np.concatenate([_b4._expo(scc / s * d_fc, sill, ran).mean(-1), np.ones((s * s, 1))], 1)
    return np.linalg.solve(A, rhs.T).T[:, :25]


def fit_variogram(gamma_coarse, scc=926.0, sill=7.0, ran=1000.0, s=4):
    """The two fits for ONE image at scale s: gamma_coarse (15,) -> (fit1 (2,), fit2 (2,)), each (sill, range)."""
    y = np.asarray(gamma_coarse, dtype=np.float64)
    d = scc * np.sqrt(np.array(KS, dtype=np.float64))
    fit1, _ = _b4._damped_least_squares(lambda p: _b4._expo(d, p[0], p[1]), y, (sill, ran))
    fit2, _ = _b4._damped_least_squares(lambda p: regularised_model(p[0], p[1], scc, s), y, fit1)
    return fit1, fit2


# ---- device side ---------------------------------------------------------------------------------------------------------------
def _sharpen(lst, ndvi_fine, coef, delta, lambdas, B, h, w, H, W, mode, s):
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=lst.device)
    _call("sifsrh_sharpen", lst, ndvi_fine, coef, delta, lambdas, out, B, h, w, H, W, mode, s)
    return out


def tsharp(lst, ndvi_coarse, ndvi_fine, min_T=285.0):
    """us.TsHARP at any ratio: the global regression and the coarse residual of `sifsr.baselines`, the unmixing of the fine index
    and the residual of the pixel's cell added back.  -> (B,1,H,W) float32."""
    B, h, w, H, W, _, _ = _check(lst, ndvi_coarse, ndvi_fine, False)
    s = _lib.stream_ptr(lst.device)
    fit = _b4._global_fit(lst, ndvi_coarse, B, h, w, min_T, s)
    delta = _b4._residual(lst, ndvi_coarse, fit, False, B, h, w, s)
    return _sharpen(lst, ndvi_fine, fit, delta, None, B, h, w, H, W, 0, s)


def _kriging(lst, ndvi_coarse, ndvi_fine, coef, per_pixel, mode, B, h, w, H, W, scale, scc, sill, ran, variogram, return_variogram,
             s):
    delta = _b4._residual(lst, ndvi_coarse, coef, per_pixel, B, h, w, s)
    info = {"gamma_coarse": None, "fit1": None}
    if variogram is None:
        gamma = _b4._semivariogram(delta, B, h, w, s).cpu().numpy()            # the call's one D2H
        fits = [fit_variogram(gamma[b], scc, sill, ran, scale) for b in range(B)]
        fit2 = np.stack([f[1] for f in fits])
        info.update(gamma_coarse=gamma, fit1=np.stack([f[0] for f in fits]))
    else:
        fit2 = np.asarray(variogram.detach().cpu() if isinstance(variogram, torch.Tensor) else variogram, dtype=np.float64)
        if fit2.shape == (2,):
            fit2 = np.broadcast_to(fit2, (B, 2))
        if fit2.shape != (B, 2):
            raise ValueError(f"variogram: expected (sill, range) as a (2,) or ({B}, 2) array, got {fit2.shape}")
    for b in range(B):
        if not (np.isfinite(fit2[b]).all() and (fit2[b] > 0).all()):
            raise _lib.SifsrError(f"image {b}: the fine-scale variogram (sill, range) = {tuple(fit2[b])} is not finite and positive")
    lam = np.stack([kriging_weights(fit2[b, 0], fit2[b, 1], scc, scale) for b in range(B)])
    lam_d = torch.from_numpy(np.ascontiguousarray(lam)).to(lst.device)         # the call's one H2D
    out = _sharpen(lst, ndvi_fine, coef, delta, lam_d, B, h, w, H, W, mode, s)
    if return_variogram:
        info.update(fit2=np.array(fit2), lambdas=lam)
        return out, info
    return out


def atprk(lst, ndvi_coarse, ndvi_fine, scc=926.0, sill=7.0, ran=1000.0, min_T=285.0, variogram=None, return_variogram=False):
    """us.ATPRK at the integer scale s = H / h in 2..8: as `sifsr.baselines.atprk`, the fine spacing scc / s, lambdas (B, s^2, 25)."""
    B, h, w, H, W, p, _ = _check(lst, ndvi_coarse, ndvi_fine, True)
    s = _lib.stream_ptr(lst.device)
    fit = _b4._global_fit(lst, ndvi_coarse, B, h, w, min_T, s)
    return _kriging(lst, ndvi_coarse, ndvi_fine, fit, False, 1, B, h, w, H, W, p, float(scc), float(sill), float(ran), variogram,
                    return_variogram, s)


def aatprk(lst, ndvi_coarse, ndvi_fine, scc=926.0, b_radius=2, sill=7.0, ran=1000.0, min_T=285.0, variogram=None,
           return_variogram=False):
    """us.AATPRK at the integer scale s = H / h in 2..8: as `sifsr.baselines.aatprk`."""
    B, h, w, H, W, p, _ = _check(lst, ndvi_coarse, ndvi_fine, True)
    if not 1 <= int(b_radius) <= 8:
        raise ValueError(f"b_radius must be in [1, 8], got {b_radius}")
    s = _lib.stream_ptr(lst.device)
    fit = _b4._global_fit(lst, ndvi_coarse, B, h, w, min_T, s)
    coef = _b4._f64((B, 2, h, w), lst)
    _lib.call("sifsrb_linfit_window", lst, ndvi_coarse, fit, coef, B, h, w, int(b_radius), float(min_T), s)
    return _kriging(lst, ndvi_coarse, ndvi_fine, coef, True, 2, B, h, w, H, W, p, float(scc), float(sill), float(ran), variogram,
                    return_variogram, s)


# ---- DMS -------------------------------------------------------------------------------------------------------------------------
def _check_dms(lst, ndvi_fine):
    for t, what in ((lst, "lst"), (ndvi_fine, "ndvi_fine")):
        if not isinstance(t, torch.Tensor):
            raise _lib.SifsrError(f"{what} must be a device tensor, got {type(t).__name__}")
        _lib.require_gpu(t, what)
        if what == "ndvi_fine" and t.dim() == 4 and t.shape[1] > 1:
            raise NotImplementedError(f"dms: only one predictor (NDVI) is built, got {t.shape[1]} channels")
        if t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"{what}: expected (B,1,H,W), got {tuple(t.shape)}")
    B, _, h, w = lst.shape
    if ndvi_fine.shape[0] != B:
        raise ValueError(f"ndvi_fine {tuple(ndvi_fine.shape)} does not match the batch of lst {tuple(lst.shape)}")
    if B < 1 or h < 1 or w < 1:
        raise ValueError(f"empty input {tuple(lst.shape)}")
    H, W = ndvi_fine.shape[2:]
    geometry((h, w), (H, W))
    return B, h, w, H, W


def dms_aggregate(fine, pow4=False, *, coarse=None):
    """Stage 1 at any ratio: (B,1,H,W) float32 -> (mean, std) (B,h,w) float64, NaN-ignoring, of the fine pixels of every cell (of
    fine^4 when pow4), added in row-major order.  coarse = (h, w): the ratio is read from the two shapes."""
    if not isinstance(fine, torch.Tensor):
        raise _lib.SifsrError(f"fine must be a device tensor, got {type(fine).__name__}")
    _lib.require_gpu(fine, "fine")
    if fine.dim() != 4 or fine.shape[1] != 1:
        raise ValueError(f"fine: expected (B,1,H,W), got {tuple(fine.shape)}")
    if coarse is None:
        raise ValueError("dms_aggregate: give coarse=(h, w); the ratio is read from the two shapes")
    B, _, H, W = fine.shape
    h, w = (int(v) for v in coarse)
    geometry((h, w), (H, W))
    mean, std = _b4._f64((B, h, w), fine), _b4._f64((B, h, w), fine)
    _call("sifsrh_aggregate", fine, mean, std, B, h, w, H, W, int(bool(pow4)), _lib.stream_ptr(fine.device))
    return mean, std


def dms_training_set(lst, ndvi_fine):
    """Stages 1 and 2 as `sifsr.baselines.dms_training_set`, on the cell statistics at the pair's ratio."""
    B, h, w, H, W = _check_dms(lst, ndvi_fine)
    mean, std = dms_aggregate(ndvi_fine, coarse=(h, w))
    return _b4._training_set(lst, mean, std, B, h, w)


def dms_model(lst, ndvi_fine, *, n_estimators=10, counts=None, seed=0):
    """Stages 1-3 as `sifsr.baselines.dms_model`: the trees are fitted on coarse cells, the ratio enters through stage 1 alone."""
    B, h, w, H, W = _check_dms(lst, ndvi_fine)
    E = _b4._estimators(n_estimators)
    return _b4._fit_model(lst, dms_training_set(lst, ndvi_fine), B, h, w, E, counts, seed)


def dms_apply(model, lst, ndvi_fine, correct=True):
    """Stages 4 and 5 at any ratio.  -> (B,1,H,W) float32; an image without a model (n_train == 0) is all NaN."""
    B, h, w, H, W = _check_dms(lst, ndvi_fine)
    s = _lib.stream_ptr(lst.device)
    thr, nleaf, leaves = model["thresholds"], model["nleaf"], model["leaves"]
    E = nleaf.shape[1]
    if tuple(thr.shape) != (B, E, DMS_MAX_LEAVES - 1) or tuple(leaves.shape) != (B, E, DMS_MAX_LEAVES, 4) or nleaf.shape[0] != B:
        raise ValueError("the model does not belong to this batch")
    sr = torch.empty((B, 1, H, W), dtype=torch.float32, device=lst.device)
    _call("sifsrh_predict", ndvi_fine, thr.contiguous(), nleaf.contiguous(), leaves.contiguous(), sr, B, E, H, W, s)
    if not correct:
        return sr
    m4 = _b4._f64((B, h, w), lst)
    _call("sifsrh_aggregate", sr, m4, None, B, h, w, H, W, 1, s)
    out = torch.empty_like(sr)
    _call("sifsrh_correct", lst, sr, m4, out, B, h, w, H, W, s)
    return out


def dms(lst, ndvi_fine, *, n_estimators=10, counts=None, seed=0, correct=True, return_model=False, moving_window_size=0,
        predictors=1, quality=None):
    """DMS as `sifsr.baselines.dms`, for a fine index at any ratio H / h <= 8.  Local windows, several predictors and quality files
    are the reference's and not built here."""
    if moving_window_size:
        raise NotImplementedError("dms: local (moving window) regressions are not built; only movingWindowSize=0")
    if predictors != 1:
        raise NotImplementedError("dms: only one predictor (NDVI) is built")
    if quality is not None:
        raise NotImplementedError("dms: low-resolution quality files are not built")
    model = dms_model(lst, ndvi_fine, n_estimators=n_estimators, counts=counts, seed=seed)
    out = dms_apply(model, lst, ndvi_fine, correct=correct)
    return (out, model) if return_model else out
