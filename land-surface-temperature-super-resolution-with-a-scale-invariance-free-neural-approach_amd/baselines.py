"""The classical sharpening baselines the paper compares the network with, on the device:

    us.TsHARP / us.ATPRK / us.AATPRK                                      utils.py:1213-1253, :1588-1606
    scored per (lst 64x64, ndvi_down 64x64, ndvi 256x256) triple           model_perf_aster_formatds.py:205-218
    DMS (`dms`, `dms_model`, `dms_apply`; the end of this file)            data_mining_sharpener_modified.py, :220-250

The data-sized parts -- the NDVI/LST regressions, the coarse residual, the empirical semivariogram and the fused unmix +
correction pass over the fine raster -- are hand-written HIP kernels in float64 (include/sifsr_baselines.h, csrc/baselines.hip);
the result is rounded once, at the float32 store.  What is left of ATPRK / AATPRK is small and stays on the HOST in float64
NumPy: two fits of (sill, range) to 15 points and one 26 x 26 linear system per image.

  fit 1   sill (1 - exp(-3 d / ran)) to the 15 points (d_k, Gamma_k), started from the `sill`, `ran` arguments
  fit 2   the regularised model Gamma_ff of utils.py:944-975 -- the fine-scale exponential variogram averaged over the 16 x 16
          fine-pixel pairs of every pair of coarse pixels of the 5 x 5 block, then accumulated per distance class, less class 0 --
          started from fit 1's result.  (The reference divides the running class sum by the running class count after EVERY row
          of the 25 x 25 matrix, not once at the end; the fit it runs is a fit of that model, so `regularised_model` has it.)
  weights utils.py:1118-1182: Gamma_cc (25 x 25), Gamma_fc (16 x 25, from the centre pixel), the bordered 26 x 26 system.

The reference fits with scipy.optimize.curve_fit(method='lm'); here the fits run the package's own damped least squares
(`_damped_least_squares`, at most LM_MAX_ITER iterations; no scipy import).  Fit 1 is degenerate on residuals whose range exceeds
the block (a valley of constant sill / ran) and where it stops depends on the optimiser, but the image does not: parity is held on
the image and on the empirical semivariogram, never on the fitted parameters, and `variogram=` takes the fit out altogether.

Transfers per call: one D2H of (B, 15) doubles (the semivariogram) and one H2D of (B, 16, 25) doubles (the weights).  With
`variogram=` there is no D2H.  `tsharp` has neither.  CPU tensors raise SifsrError: there is no fallback.
Index NaNs: pinned for `tsharp` (a NaN fine index stays NaN, a NaN coarse index is left out of the regression and makes its
4 x 4 pixels NaN); in the kriging methods they are not pinned against the reference.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

# At any other ratio H / h <= 8 (kriging: integer scales 2..8) the same seven functions are sifsr.rbaselines.
KS = (0, 1, 2, 4, 5, 8, 9, 10, 13, 16, 17, 18, 20, 25, 32)       # squared coarse distances inside a 5 x 5 block
LM_MAX_ITER = 200

# ---- host geometry (scale 4, block 5), in units of the fine pixel ----------------------------------------------------------
_RC = np.stack(np.divmod(np.arange(25), 5), 1)
_DR = np.abs(_RC[:, None, 0] - _RC[None, :, 0])                    # (25, 25) coarse row / column offsets of block pixels i, j
_DC = np.abs(_RC[:, None, 1] - _RC[None, :, 1])
_CLASS = np.searchsorted(np.array(KS), _DR ** 2 + _DC ** 2)
_MEMBER = (_CLASS[None] == np.arange(15)[:, None, None]).astype(np.float64)      # (15, 25, 25)
_COUNT = np.cumsum(_MEMBER.sum(2), 1)                              # (15, 25) running class count after row i
_E = np.arange(-3, 4)                                              # fine offset inside a coarse pixel pair, multiplicity 4 - |e|
_MULT = ((4 - np.abs(_E))[:, None] * (4 - np.abs(_E))[None, :] / 256.0).ravel()
# by translation symmetry Gamma_cc[i, j] depends on the coarse offset alone: (5, 5, 49) fine distances per offset
_D_CC = np.sqrt((4 * np.arange(5)[:, None, None, None] + _E[None, None, :, None]) ** 2
                + (4 * np.arange(5)[None, :, None, None] + _E[None, None, None, :]) ** 2).reshape(5, 5, 49)
_A = np.stack(np.divmod(np.arange(16), 4), 1)                      # fine pixel a inside a coarse pixel
_D_FC = np.sqrt((4 * (_RC[None, :, None, 0] - 2) + _A[None, None, :, 0] - _A[:, None, None, 0]) ** 2
                + (4 * (_RC[None, :, None, 1] - 2) + _A[None, None, :, 1] - _A[:, None, None, 1]) ** 2)   # (16 a, 25 j, 16 b)


def _expo(d, sill, ran):
    return sill * (1.0 - np.exp(-d / (ran / 3.0)))


def _gamma_cc(sill, ran, scc):
    tab = (_expo(scc / 4.0 * _D_CC, sill, ran) * _MULT).sum(-1)    # (5, 5)
    return tab[_DR, _DC]


def regularised_model(sill, ran, scc=926.0):
    """Gamma_ff of utils.py:944-975 at the 15 distance classes (module docstring: the running division is the reference's)."""
    rows = np.einsum("kij,ij->ki", _MEMBER, _gamma_cc(sill, ran, scc))
    m = np.zeros(15)
    for i in range(25):
        m = (m + rows[:, i]) / _COUNT[:, i]
    return m - m[0]


def kriging_weights(sill, ran, scc=926.0):
    """utils.py:1118-1182: the (16, 25) weights of the 5 x 5 coarse residuals for the 16 fine pixels of the centre coarse pixel."""
    A = np.zeros((26, 26))
    A[:25, :25] = _gamma_cc(sill, ran, scc)
    A[:25, 25] = A[25, :25] = 1.0
    rhs = np.concatenate([_expo(scc / 4.0 * _D_FC, sill, ran).mean(-1), np.ones((16, 1))], 1)      # (16, 26)
    return np.linalg.solve(A, rhs.T).T[:, :25]


def _damped_least_squares(model, y, p0, max_iter=LM_MAX_ITER):
    """Levenberg-Marquardt on the 2 parameters of `model`: forward-difference Jacobian, Marquardt's scaling by the largest
    diagonal of J^T J seen so far, damping / 10 after an accepted step and x 10 after a rejected one.  Stops when an accepted step
    lowers the cost by less than 1e-14 of it and moves the parameters by less than 1e-10 of their size, when no damping up to
    1e12 lowers the cost, or after max_iter iterations.  -> (p, iterations)"""
    p = np.asarray(p0, dtype=np.float64).copy()
    r = model(p) - y
    cost = float(r @ r)
    mu, scale = 1e-3, np.zeros(2)
    for it in range(max_iter):
        J = np.empty((y.size, 2))
        for k in range(2):
            step = 1.5e-8 * max(abs(p[k]), 1e-300)
            q = p.copy()
            q[k] += step
            J[:, k] = (model(q) - y - r) / step
        A, g = J.T @ J, J.T @ r
        scale = np.maximum(scale, np.diag(A))
        accepted = False
        while mu <= 1e12:
            try:
                dp = np.linalg.solve(A + mu * np.diag(np.where(scale > 0, scale, 1.0)), -g)
            except np.linalg.LinAlgError:
                mu *= 10.0
                continue
            with np.errstate(all="ignore"):
                rn = model(p + dp) - y
                cn = float(rn @ rn)
            if np.isfinite(cn) and cn < cost:
                accepted = True
                break
            mu *= 10.0
        if not accepted:
            return p, it
        small = (cost - cn) <= 1e-14 * cost and np.all(np.abs(dp) <= 1e-10 * np.abs(p + dp))
        p, r, cost, mu = p + dp, rn, cn, max(mu / 10.0, 1e-12)
        if small or cost == 0.0:
            return p, it + 1
    return p, max_iter


def fit_variogram(gamma_coarse, scc=926.0, sill=7.0, ran=1000.0):
    """The two fits for ONE image: gamma_coarse (15,) -> (fit1 (2,), fit2 (2,)), each (sill, range)."""
    y = np.asarray(gamma_coarse, dtype=np.float64)
    d = scc * np.sqrt(np.array(KS, dtype=np.float64))
    fit1, _ = _damped_least_squares(lambda p: _expo(d, p[0], p[1]), y, (sill, ran))
    fit2, _ = _damped_least_squares(lambda p: regularised_model(p[0], p[1], scc), y, fit1)
    return fit1, fit2


# ---- device side ----------------------------------------------------------------------------------------------------------
def _check(lst, ndvi_coarse, ndvi_fine):
    for t, what in ((lst, "lst"), (ndvi_coarse, "ndvi_coarse"), (ndvi_fine, "ndvi_fine")):
        if not isinstance(t, torch.Tensor):
            raise _lib.SifsrError(f"{what} must be a device tensor, got {type(t).__name__}")
        _lib.require_gpu(t, what)
        if t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"{what}: expected (B,1,H,W), got {tuple(t.shape)}")
    B, _, h, w = lst.shape
    if tuple(ndvi_coarse.shape) != (B, 1, h, w):
        raise ValueError(f"ndvi_coarse {tuple(ndvi_coarse.shape)} does not match lst {tuple(lst.shape)}")
    if tuple(ndvi_fine.shape) != (B, 1, 4 * h, 4 * w):
        raise ValueError(f"ndvi_fine must be exactly 4x the coarse shape ({B}, 1, {4 * h}, {4 * w}), got {tuple(ndvi_fine.shape)}")
    if h < 5 or w < 5:
        raise ValueError(f"the coarse image must be at least 5 x 5 (one kriging block), got {h} x {w}")
    return B, h, w


def _f64(shape, like):
    return torch.empty(shape, dtype=torch.float64, device=like.device)


def _global_fit(lst, ndvi_coarse, B, h, w, min_T, s):
    fit = _f64((B, 2), lst)
    _lib.call("sifsrb_linfit", lst, ndvi_coarse, fit, B, h, w, float(min_T), s)
    return fit


def _residual(lst, ndvi_coarse, coef, per_pixel, B, h, w, s):
    delta = _f64((B, h, w), lst)
    _lib.call("sifsrb_residual", lst, ndvi_coarse, coef, int(per_pixel), delta, B, h, w, s)
    return delta


def _semivariogram(delta, B, h, w, s):
    nbytes = _lib.call("sifsrb_semivariogram_scratch_bytes", B, h, w)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=delta.device)
    gamma = _f64((B, 15), delta)
    _lib.call("sifsrb_semivariogram", delta, scratch, gamma, B, h, w, s)
    return gamma


def _sharpen(lst, ndvi_fine, coef, delta, lambdas, B, h, w, mode, s):
    out = torch.empty((B, 1, 4 * h, 4 * w), dtype=torch.float32, device=lst.device)
    _lib.call("sifsrb_sharpen", lst, ndvi_fine, coef, delta, lambdas, out, B, h, w, mode, s)
    return out


def semivariogram(delta):
    """Gamma_coarse of utils.py:1008-1051: delta (B,1,h,w) float64 device tensor -> (B,15) float64 device tensor, the classes
    scc * sqrt(KS)."""
    if not isinstance(delta, torch.Tensor) or not delta.is_cuda:
        raise _lib.SifsrError("semivariogram: delta must be a device tensor; there is no CPU path")
    if delta.dtype != torch.float64 or delta.dim() != 4 or delta.shape[1] != 1:
        raise ValueError(f"semivariogram: expected a (B,1,h,w) float64 tensor, got {tuple(delta.shape)} {delta.dtype}")
    B, _, h, w = delta.shape
    if h < 5 or w < 5:
        raise ValueError(f"the coarse image must be at least 5 x 5, got {h} x {w}")
    return _semivariogram(delta.contiguous(), B, h, w, _lib.stream_ptr(delta.device))


def tsharp(lst, ndvi_coarse, ndvi_fine, min_T=285.0):
    """us.TsHARP (utils.py:1213-1231): global NDVI/LST regression over the pixels above min_T, unmixing of the fine index, and the
    coarse residual added back per coarse pixel.  -> (B,1,4h,4w) float32."""
    B, h, w = _check(lst, ndvi_coarse, ndvi_fine)
    s = _lib.stream_ptr(lst.device)
    fit = _global_fit(lst, ndvi_coarse, B, h, w, min_T, s)
    delta = _residual(lst, ndvi_coarse, fit, False, B, h, w, s)
    return _sharpen(lst, ndvi_fine, fit, delta, None, B, h, w, 0, s)


def _kriging(lst, ndvi_coarse, ndvi_fine, coef, per_pixel, mode, B, h, w, scc, sill, ran, variogram, return_variogram, s):
    delta = _residual(lst, ndvi_coarse, coef, per_pixel, B, h, w, s)
    info = {"gamma_coarse": None, "fit1": None}
    if variogram is None:
        gamma = _semivariogram(delta, B, h, w, s).cpu().numpy()               # the call's one D2H
        fits = [fit_variogram(gamma[b], scc, sill, ran) for b in range(B)]
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
    lam = np.stack([kriging_weights(fit2[b, 0], fit2[b, 1], scc) for b in range(B)])
    lam_d = torch.from_numpy(np.ascontiguousarray(lam)).to(lst.device)        # the call's one H2D
    out = _sharpen(lst, ndvi_fine, coef, delta, lam_d, B, h, w, mode, s)
    if return_variogram:
        info.update(fit2=np.array(fit2), lambdas=lam)
        return out, info
    return out


def atprk(lst, ndvi_coarse, ndvi_fine, scc=926.0, sill=7.0, ran=1000.0, min_T=285.0, variogram=None, return_variogram=False):
    """us.ATPRK (utils.py:1234-1253): TsHARP's regression and unmixing, the residual downscaled by area-to-point kriging over
    5 x 5 coarse blocks.  `scc`: coarse pixel size; `sill`, `ran`: start of fit 1; `variogram`: the FINAL fine-scale (sill, range),
    (2,) or (B,2) -- skips both fits and the D2H.  return_variogram=True: also a dict with gamma_coarse (B,15) float64, fit1 and
    fit2 (B,2), lambdas (B,16,25) (gamma_coarse and fit1 are None when `variogram` was given)."""
    B, h, w = _check(lst, ndvi_coarse, ndvi_fine)
    s = _lib.stream_ptr(lst.device)
    fit = _global_fit(lst, ndvi_coarse, B, h, w, min_T, s)
    return _kriging(lst, ndvi_coarse, ndvi_fine, fit, False, 1, B, h, w, float(scc), float(sill), float(ran), variogram,
                    return_variogram, s)


def aatprk(lst, ndvi_coarse, ndvi_fine, scc=926.0, b_radius=2, sill=7.0, ran=1000.0, min_T=285.0, variogram=None,
           return_variogram=False):
    """us.AATPRK (utils.py:1588-1606): the regression is fitted per coarse pixel over its (2 b_radius + 1)^2 window (the global
    fit where no more than 2/3 of the window is valid, and within b_radius of a border); the rest as `atprk`."""
    B, h, w = _check(lst, ndvi_coarse, ndvi_fine)
    if not 1 <= int(b_radius) <= 8:
        raise ValueError(f"b_radius must be in [1, 8], got {b_radius}")
    s = _lib.stream_ptr(lst.device)
    fit = _global_fit(lst, ndvi_coarse, B, h, w, min_T, s)
    coef = _f64((B, 2, h, w), lst)
    _lib.call("sifsrb_linfit_window", lst, ndvi_coarse, fit, coef, B, h, w, int(b_radius), float(min_T), s)
    return _kriging(lst, ndvi_coarse, ndvi_fine, coef, True, 2, B, h, w, float(scc), float(sill), float(ran), variogram,
                    return_variogram, s)


# ---- DMS, the Data Mining Sharpener (include/sifsr_dms.h, csrc/dms.hip) -----------------------------------
DMS_MAX_LEAVES, DMS_MIN_TRAIN = 30, 10


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
    if tuple(ndvi_fine.shape) != (B, 1, 4 * h, 4 * w):
        raise ValueError(f"ndvi_fine must be exactly 4x the coarse shape ({B}, 1, {4 * h}, {4 * w}), got {tuple(ndvi_fine.shape)}")
    if B < 1 or h < 1 or w < 1:
        raise ValueError(f"empty input {tuple(lst.shape)}")
    return B, h, w


def dms_aggregate(fine, pow4=False):
    """Stage 1: (B,1,4h,4w) float32 -> (mean, std) (B,h,w) float64, NaN-ignoring, of the 4 x 4 blocks (of fine^4 when pow4)."""
    _lib.require_gpu(fine, "fine")
    B, _, H, W = fine.shape
    if H % 4 or W % 4:
        raise ValueError(f"the fine raster must be a multiple of 4 on both axes, got {H} x {W}")
    mean, std = _f64((B, H // 4, W // 4), fine), _f64((B, H // 4, W // 4), fine)
    _lib.call("sifsrd_aggregate", fine, mean, std, B, H // 4, W // 4, int(bool(pow4)), _lib.stream_ptr(fine.device))
    return mean, std


def dms_training_set(lst, ndvi_fine):
    """Stages 1 and 2 -> dict(x, cv, weight (B,N) float64, good (B,N) bool, threshold (B,) float64, n_train (B,) int32: 0 where
    fewer than 10 cells are good).  The percentile's sort is torch.sort."""
    B, h, w = _check_dms(lst, ndvi_fine)
    mean, std = dms_aggregate(ndvi_fine)
    return _training_set(lst, mean, std, B, h, w)


def _training_set(lst, mean, std, B, h, w):
    """stage 2 on the cell statistics (B,h,w) of stage 1: nothing here knows the ratio (sifsr.rbaselines calls it too)"""
    N, s, dev = h * w, _lib.stream_ptr(lst.device), lst.device
    x, cv = _f64((B, N), lst), _f64((B, N), lst)
    good = torch.empty((B, N), dtype=torch.uint8, device=dev)
    _lib.call("sifsrd_trainset", lst, mean, std, x, cv, good, B, h, w, s)
    good = good.bool()
    n = good.sum(1)
    n_train = torch.where(n >= DMS_MIN_TRAIN, n, torch.zeros_like(n))
    good = good & (n_train > 0)[:, None]
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    srt = torch.sort(torch.where(good, cv, inf), dim=1).values
    last = (n_train - 1).clamp(min=0)
    v = last.double() * (80 / 100)                                      # np.percentile(., 80), linear
    lo = v.floor().long()
    hi = torch.minimum(lo + 1, last)
    t = v - lo.double()
    a, b = srt.gather(1, lo[:, None])[:, 0], srt.gather(1, hi[:, None])[:, 0]
    thr = torch.where(t >= 0.5, b - (b - a) * (1 - t), a + (b - a) * t)
    stats = torch.stack([thr, srt[:, 0], srt.gather(1, last[:, None])[:, 0]], 1).contiguous()
    weight = _f64((B, N), lst)
    _lib.call("sifsrd_weights", cv, good.to(torch.uint8), stats, weight, B, N, s)
    return dict(x=x, cv=cv, weight=weight, good=good, threshold=thr, n_train=n_train.int())


def _bootstrap_counts(good, n_train, E, seed):
    """(B,E,N) int32 multiplicities in row-major cell order: per image n_train draws with replacement among its good cells.  The
    same E x N integers serve every image (scaled to its n_train), so an image's draw does not depend on the batch around it."""
    B, N = good.shape
    g = torch.Generator(device=good.device)
    g.manual_seed(int(seed))
    r = torch.randint(0, 1 << 31, (E, N), generator=g, device=good.device, dtype=torch.int64)
    nt = n_train.long()[:, None, None]
    rank = (r[None] * nt) >> 31                                          # uniform in [0, n_train)
    valid = torch.arange(N, device=good.device)[None, None, :] < nt
    order = torch.sort((~good).to(torch.uint8), dim=1, stable=True).indices        # the good cells first, row-major
    cell = order.gather(1, rank.reshape(B, E * N)).reshape(B, E, N)
    counts = torch.zeros((B, E, N), dtype=torch.int64, device=good.device)
    counts.scatter_add_(2, cell, valid.expand(B, E, N).long())                          # integer adds: the order does not matter
    return counts.int()


def dms_model(lst, ndvi_fine, *, n_estimators=10, counts=None, seed=0):
    """Stages 1-3: fit the bagged trees of every image.  -> dict(thresholds (B,E,29) float64 ascending, +inf padded; nleaf (B,E)
    int32; leaves (B,E,30,4) float64 = coef, intercept, lo, hi; n_train (B,) int32; counts (B,E,h*w) int32)."""
    B, h, w = _check_dms(lst, ndvi_fine)
    E = _estimators(n_estimators)
    return _fit_model(lst, dms_training_set(lst, ndvi_fine), B, h, w, E, counts, seed)


def _estimators(n_estimators):
    E = int(n_estimators)
    if not 1 <= E <= 32:
        raise ValueError(f"n_estimators must be in [1, 32], got {n_estimators}")
    return E


def _fit_model(lst, ts, B, h, w, E, counts, seed):
    """stage 3 on a training set of coarse cells: nothing here knows the ratio (sifsr.rbaselines calls it too)"""
    N, s, dev = h * w, _lib.stream_ptr(lst.device), lst.device
    good, n_train = ts["good"], ts["n_train"]
    if counts is None:
        counts = _bootstrap_counts(good, n_train, E, seed)
    else:
        if not isinstance(counts, torch.Tensor) or not counts.is_cuda:
            raise _lib.SifsrError("counts must be a device tensor; there is no CPU path")
        if tuple(counts.shape) != (B, E, N) or counts.dtype.is_floating_point or counts.dtype == torch.bool:
            raise ValueError(f"counts: expected an integer ({B}, {E}, {N}) tensor, got {tuple(counts.shape)} {counts.dtype}")
        counts = counts.int()
    # the samples in ascending order of the float32 feature, the cells that are not good last
    inf32 = torch.full((), float("inf"), dtype=torch.float32, device=dev)
    perm = torch.sort(torch.where(good, ts["x"].float(), inf32), dim=1, stable=True).indices
    xs = ts["x"].gather(1, perm).contiguous()
    ys = lst.reshape(B, N).double().gather(1, perm).contiguous()
    ws = ts["weight"].gather(1, perm).contiguous()
    cs = counts.gather(2, perm[:, None, :].expand(B, E, N)).contiguous()
    nbytes = _lib.call("sifsrd_fit_scratch_bytes", B, E, N)
    if nbytes == 0:
        raise ValueError(f"unsupported shape B={B}, E={E}, N={N}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    thresholds = _f64((B, E, DMS_MAX_LEAVES - 1), lst)
    nleaf = torch.empty((B, E), dtype=torch.int32, device=dev)
    leaves = _f64((B, E, DMS_MAX_LEAVES, 4), lst)
    _lib.call("sifsrd_fit", xs, ys, ws, cs, n_train, scratch, thresholds, nleaf, leaves, B, E, N, s)
    return dict(thresholds=thresholds, nleaf=nleaf, leaves=leaves, n_train=n_train, counts=counts)


def dms_apply(model, lst, ndvi_fine, correct=True):
    """Stages 4 and 5: the ensemble's prediction of the fine index and (correct=True) the radiance residual correction against
    `lst`.  -> (B,1,4h,4w) float32; an image without a model (n_train == 0) is all NaN."""
    B, h, w = _check_dms(lst, ndvi_fine)
    s = _lib.stream_ptr(lst.device)
    thr, nleaf, leaves = model["thresholds"], model["nleaf"], model["leaves"]
    E = nleaf.shape[1]
    if tuple(thr.shape) != (B, E, DMS_MAX_LEAVES - 1) or tuple(leaves.shape) != (B, E, DMS_MAX_LEAVES, 4) or nleaf.shape[0] != B:
        raise ValueError("the model does not belong to this batch")
    sr = torch.empty((B, 1, 4 * h, 4 * w), dtype=torch.float32, device=lst.device)
    _lib.call("sifsrd_predict", ndvi_fine, thr.contiguous(), nleaf.contiguous(), leaves.contiguous(), sr, B, E, h, w, s)
    if not correct:
        return sr
    m4 = _f64((B, h, w), lst)
    _lib.call("sifsrd_aggregate", sr, m4, None, B, h, w, 1, s)
    out = torch.empty_like(sr)
    _lib.call("sifsrd_correct", lst, sr, m4, out, B, h, w, s)
    return out


def dms(lst, ndvi_fine, *, n_estimators=10, counts=None, seed=0, correct=True, return_model=False, moving_window_size=0,
        predictors=1, quality=None):
    """DMS as the reference's evaluation runs it (model_perf_aster_formatds.py:220-250): NDVI -> LST trees with per-leaf ridge,
    global regression, T^4 residual correction.  lst (B,1,h,w) float32 Kelvin (NaN or <= 0: no data), ndvi_fine (B,1,4h,4w).
    `counts`: (B,E,h*w) integer bootstrap multiplicities in row-major cell order; absent, they are drawn on the device from
    `seed`.  Deterministic: the same inputs and seed give the same bits.  Local windows, several predictors and quality files are
    the reference's and not built here."""
    if moving_window_size:
        raise NotImplementedError("dms: local (moving window) regressions are not built; only movingWindowSize=0")
    if predictors != 1:
        raise NotImplementedError("dms: only one predictor (NDVI) is built")
    if quality is not None:
        raise NotImplementedError("dms: low-resolution quality files are not built")
    model = dms_model(lst, ndvi_fine, n_estimators=n_estimators, counts=counts, seed=seed)
    out = dms_apply(model, lst, ndvi_fine, correct=correct)
    return (out, model) if return_model else out
