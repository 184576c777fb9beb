"""Fourier scores for rasters of any size (include/sifsr_spectra.h, csrc/fourier.hip) -- the last four columns of
the reference's performances.csv on the rectangles the real evaluation produces:

    fourier_dict[m] = np.fft.fftshift(np.abs(sp.fft.fft2(LST_m)))       compare_methods.py:305-324, on the l x c crop of a pair
    us.compute_2D_attenuation_spectra(fourier_dict[m])                   utils.py:598-636
    PFR, AFR, FRR, FRO, FRU, RMSE_ATT per pair and method                compare_methods.py:336-353
    mean, std, 10%, Q1, mediane, Q3, 90%                                 compare_methods.py:376-410, model_perf_aster_formatds.py:514-520

``fft2_magnitude`` and ``attenuation_spectra`` are those of ``sifsr.fourier`` for sides that need not be powers of two (a power of
two in 4..2048 or any integer in 4..1024) and for lists of rasters of mixed sizes: an axis that is no power of two runs Bluestein's
chirp-z transform over the same radix-2 butterfly, float64 throughout; rasters with two power-of-two sides get the bits of
``sifsr.fourier``.  The score algebra is a few hundred scalar operations on the 1-D spectra and stays on the host, vectorised, with
the ``get_*`` functions of ``sifsr.fourier``.  CPU-only use raises SifsrError: there is no fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, fourier

SCORES = ("PFR", "AFR", "FRR", "FRO", "FRU", "RMSE_ATT")
SUMMARY = ("mean", "std", "10%", "Q1", "mediane", "Q3", "90%")
_PERCENTILES = (10, 25, 50, 75, 90)


def _call(x, want_mag, want_spec):
    """x (B,H,W) -> (mag (B,H,W) or None, spectrum (B, min(H//2, W//2)) or None) after one ``sifsrf_fft2_attenuation``"""
    _lib.require_gpu(x, "image")
    if x.dim() != 3:
        raise _lib.SifsrError("expected an (H,W) image, a (B,H,W) stack or a list of (H,W) images")
    B, H, W = x.shape
    nbytes = _lib.call("sifsrf_fft2_attenuation_scratch_bytes", B, H, W)
    if nbytes == 0:
        raise _lib.SifsrError(f"stack {(B, H, W)}: each side must be a power of two in 4..2048 or any integer in 4..1024")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    mag = torch.empty((B, H, W), dtype=torch.float32, device=x.device) if want_mag else None
    spec = torch.empty((B, min(H // 2, W // 2)), dtype=torch.float32, device=x.device) if want_spec else None
    _lib.call("sifsrf_fft2_attenuation", x, B, H, W, scratch, nbytes, mag, spec, _lib.stream_ptr(x.device))
    return mag, spec


def _run(img, want_mag, want_spec):
    if not isinstance(img, (list, tuple)):
        if img.dim() == 2:
            mag, spec = _call(img[None], want_mag, want_spec)
            return (None if mag is None else mag[0]), (None if spec is None else spec[0])
        return _call(img, want_mag, want_spec)
    # a list of (H,W) rasters: those of equal shape go down in one call, in the order of their first appearance
    groups = {}
    for i, t in enumerate(img):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise _lib.SifsrError("a list must hold (H,W) images")
        _lib.require_gpu(t, "image")
        groups.setdefault(tuple(t.shape), []).append(i)
    mags, specs = [None] * len(img), [None] * len(img)
    for idx in groups.values():
        mag, spec = _call(torch.stack([img[i] for i in idx]), want_mag, want_spec)
        for j, i in enumerate(idx):
            mags[i] = None if mag is None else mag[j]
            specs[i] = None if spec is None else spec[j]
    return mags, specs


def fft2_magnitude(img):
    """fftshift(|fft2(img)|) of an (H,W) image, a (B,H,W) stack or a list of (H,W) images of mixed sizes (-> a list)."""
    return _run(img, True, False)[0]


def attenuation_spectra(img):
    """1-D attenuation spectrum [dB] of the image(s), min(H//2, W//2) values each: compute_2D_attenuation_spectra(fftshift(|fft2|)),
    utils.py:598-636.  An (H,W) image, a (B,H,W) stack or a list of (H,W) images of mixed sizes (-> a list)."""
    return _run(img, False, True)[1]


def scores_from_spectra(aster_dB, bicubic_dB, model_dB):
    """compare_methods.py:344-353 for one method of one pair, on the host -> float64 (6,): PFR, AFR, FRR, FRO, FRU, RMSE_ATT.
    RMSE_ATT runs over the whole spectrum, element 0 included."""
    rb, xb, pb = (np.asarray(v, dtype=np.float64) for v in (aster_dB, bicubic_dB, model_dB))
    return np.array([fourier.get_PFR(rb, xb), fourier.get_AFR(pb, rb, xb), fourier.get_FRR(pb, rb, xb), fourier.get_FRO(pb, rb, xb),
                     fourier.get_FRU(pb, rb, xb), float(np.sqrt(np.mean((pb - rb) ** 2)))], dtype=np.float64)


def _pair_stack(aster, bicubic, predictions):
    preds = list(predictions) if isinstance(predictions, (list, tuple)) else predictions
    if isinstance(preds, list):
        if not preds:
            raise _lib.SifsrError("a pair needs at least one prediction")
        preds = torch.stack(preds)
    if aster.dim() != 2 or bicubic.shape != aster.shape or preds.dim() != 3 or preds.shape[1:] != aster.shape:
        raise _lib.SifsrError(f"a pair is aster (H,W), bicubic (H,W) and K predictions (H,W): got {tuple(aster.shape)}, "
                              f"{tuple(bicubic.shape)} and {tuple(preds.shape)}")
    return torch.cat((aster[None], bicubic[None], preds))


def spectral_scores(aster, bicubic, predictions):
    """The loop of compare_methods.py:336-353.  One pair: ``aster`` (H,W), ``bicubic`` (H,W), ``predictions`` a (K,H,W) stack or a
    list of K (H,W) rasters; or three lists of those, one entry per pair, of any sizes (the same K for every pair).  All K + 2
    rasters of a pair go through one ``sifsrf_fft2_attenuation`` call; the spectra are read back once, after the last launch.
    -> float64 array (pairs, K, 6) of ``SCORES``; one pair gives (1, K, 6)."""
    if not isinstance(aster, (list, tuple)):
        aster, bicubic, predictions = [aster], [bicubic], [predictions]
    if not (len(aster) == len(bicubic) == len(predictions)):
        raise _lib.SifsrError(f"{len(aster)} aster, {len(bicubic)} bicubic and {len(predictions)} prediction entries")
    specs = [_call(_pair_stack(a, b, p), False, True)[1] for a, b, p in zip(aster, bicubic, predictions)]
    K = {s.shape[0] - 2 for s in specs}
    if len(K) > 1:
        raise _lib.SifsrError(f"every pair needs the same number of predictions, got {sorted(K)}")
    out = np.empty((len(specs), K.pop() if K else 0, 6), dtype=np.float64)
    for i, s in enumerate(specs):
        s = s.cpu().numpy().astype(np.float64)
        for k in range(out.shape[1]):
            out[i, k] = scores_from_spectra(s[0], s[1], s[2 + k])
    return out


def summary_rows(table, ddof):
    """The seven rows the reference appends to a performances table: ``SUMMARY`` over axis 0 of ``table`` (pairs, ...) -> float64
    (7, ...).  Quantiles interpolate linearly (np.percentile's default, DataFrame.quantile's too).  ``ddof = 1`` is the pandas
    ``std`` of model_perf_aster_formatds.py:514-520 (the nine per-pair columns), ``ddof = 0`` the ``np.std`` of
    compare_methods.py:376-410 (the four spectral ones).  Host only."""
    if ddof not in (0, 1):
        raise _lib.SifsrError(f"ddof must be 0 (np.std) or 1 (pandas), got {ddof}")
    t = np.asarray(table.detach().cpu() if isinstance(table, torch.Tensor) else table, dtype=np.float64)
    if t.ndim < 1 or t.shape[0] == 0:
        raise _lib.SifsrError("summary_rows needs at least one row")
    with np.errstate(invalid="ignore", divide="ignore"):            # one pair and ddof = 1: NaN, as pandas gives
        std = t.std(axis=0, ddof=ddof) if t.shape[0] > ddof else np.full(t.shape[1:], np.nan)
    return np.stack([t.mean(axis=0), std] + [np.percentile(t, q, axis=0) for q in _PERCENTILES])
