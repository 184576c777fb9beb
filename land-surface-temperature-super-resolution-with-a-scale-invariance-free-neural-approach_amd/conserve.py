"""Does the super-resolved raster conserve the observed one? (include/sifsr_conserve.h, csrc/conserve.hip)

The training signal of the scale-invariance-free loss is ``Huber(D(SR), LST)``: the super-resolved raster, seen through the sensor's
MTF and decimated by 4 (``sif_ops.downscale_LST_SR_to_LR``), should be the raster the sensor observed.  Every method the paper
compares against enforces that as its last step (TsHARP's ``correction_linreg``, the kriged residual of ATPRK / AATPRK); here, on
the device, for the network's output and for rasters with gaps:

    consistency   the residual ``r = lst - D(sr)`` over the cells whose whole 3 x 3 neighbourhood is valid, reduced to
                  (count, bias, RMSE, max |r|) in float64
    conserve      ``n_iter`` steps of ``sr += relax * U(r)`` (U: the bicubic x4 of the input pipeline, clamped at the raster edge) at
                  the pixels of valid cells; every other pixel keeps its bits

A cell is an LST pixel and the 4 x 4 sr pixels under it; it is valid iff the LST pixel is finite, not 0 K and kept by ``mask`` (the
rule of ``gaps.fill_gaps``) and its 16 sr pixels are finite and not 0 (``fill_value`` = NaN, the zeros of an uncovered edge).  What
invalid pixels hold changes no output bit.  Nothing is read back: the statistics stay on the device.  CPU-only use raises
SifsrError: there is no fallback.
"""
from __future__ import annotations

import functools
import inspect

import torch

from . import _lib, sif_ops

MAX_ITER = 64


def _call(sr, lst, mask, out, n_iter, relax, mtf):
    """-> (stats (n_iter+1, 4) float64, workspace) after one ``sifsrk_conserve``"""
    _lib.require_gpu(sr, "sr"); _lib.require_gpu(lst, "lst")
    if lst.dim() != 2 or sr.dim() != 2 or tuple(sr.shape) != (4 * lst.shape[0], 4 * lst.shape[1]):
        raise _lib.SifsrError(f"expected lst (h,w) and sr (4h,4w), got {tuple(lst.shape)} and {tuple(sr.shape)}")
    if sr.device != lst.device:
        raise _lib.SifsrError(f"sr is on {sr.device}, lst on {lst.device}")
    h, w = lst.shape
    n_iter = int(n_iter)
    if not 0 <= n_iter <= MAX_ITER:
        raise _lib.SifsrError(f"n_iter must be in 0..{MAX_ITER}, got {n_iter}")
    if mask is not None:
        from .gaps import _valid_raster
        mask = _valid_raster(mask, (h, w), lst.device, "mask")
    need = _lib.call("sifsrk_workspace_bytes", h, w, n_iter)
    if need == 0:
        raise _lib.SifsrError(f"lst raster {(h, w)}: each side must be in 3..16384")
    ws = torch.empty((need,), dtype=torch.uint8, device=lst.device)
    stats = torch.empty((n_iter + 1, 4), dtype=torch.float64, device=lst.device)
    _lib.call("sifsrk_conserve", sr, lst, mask, out, stats, ws, need, h, w, sif_ops._taps_c(mtf, 4, None), float(relax), n_iter,
              _lib.stream_ptr(lst.device))
    return stats, ws


def consistency(sr, lst, mask=None, mtf=0.1, return_residual=False):
    """sr (4h,4w) [K], lst (h,w) [K], mask (h,w) uint8 / bool or None (non-zero = keep) -> the float64 device tensor
    (count, bias, RMSE, max |r|) of ``r = lst - D(sr)`` over the counted cells (count 0: NaN in the other three).
    ``return_residual``: also r (h,w) float32, 0 where the cell is not counted."""
    stats, ws = _call(sr, lst, mask, None, 0, 1.0, mtf)
    if return_residual:
        h, w = lst.shape
        return stats[0], ws[:4 * h * w].view(torch.float32).view(h, w).clone()
    return stats[0]


def conserve(sr, lst, mask=None, n_iter=1, relax=1.0, mtf=0.1, out=None, return_stats=False):
    """``n_iter`` correction steps ``sr += relax * U(lst - D(sr))`` at the pixels of valid cells -> the corrected raster (4h,4w);
    ``out``: the buffer to write (``out=sr`` corrects in place), default a new one.  ``n_iter = 0`` copies.
    ``return_stats``: also the float64 device tensor (n_iter+1, 4) of (count, bias, RMSE, max |r|) before the first step and after
    every step."""
    if out is None:
        out = torch.empty_like(sr)
    else:
        _lib.require_gpu(out, "out")
        if out.shape != sr.shape or out.device != sr.device:
            raise _lib.SifsrError(f"out must be {tuple(sr.shape)} on {sr.device}, got {tuple(out.shape)} on {out.device}")
        if out.data_ptr() != sr.data_ptr() and out.untyped_storage().data_ptr() == sr.untyped_storage().data_ptr():
            lo, hi = sorted((out.data_ptr(), sr.data_ptr()))
            if hi < lo + sr.numel() * 4:
                raise _lib.SifsrError("out overlaps sr partly: pass sr itself or a separate buffer")
    stats, _ = _call(sr, lst, mask, out, n_iter, relax, mtf)
    if int(n_iter) == 0 and out.data_ptr() != sr.data_ptr():
        out.copy_(sr)
    return (out, stats) if return_stats else out


def granule_option(fn, correct=None):
    """Decorator that gives a whole-granule prediction call (``predict.predict_granule``, ``gaps.predict_granule_gaps``) the
    keyword-only option ``conserve=k``: k correction steps on the blended raster, in place, against the call's own ``lst_g`` (and
    ``mask``, where the call has one), on the same stream; with ``return_info`` the statistics go into the info dict as
    ``"conserve_stats"``.  ``conserve=0``, the default, is the undecorated call: the same launches, the same bits.  The option is
    added around the call and not to its parameter list: the positional signature of the two calls is part of their contract
    (tests/test_gaps_host.py pins it) and stays what it was; ``inspect.signature(f, follow_wrapped=False)`` shows the option.
    ``correct``: the step to run, with the signature of ``conserve`` (``rconserve.granule_option`` passes its own); default
    ``conserve`` of this module."""
    sig = inspect.signature(fn)
    correct = correct or globals()["conserve"]

    @functools.wraps(fn)
    def call(*args, conserve=0, **kw):
        k = int(conserve)
        if k < 0:
            raise _lib.SifsrError(f"conserve must be a step count >= 0, got {conserve}")
        res = fn(*args, **kw)
        if k == 0:
            return res
        a = sig.bind(*args, **kw)
        a.apply_defaults()
        a = a.arguments
        out, info = res if a.get("return_info") else (res, None)
        with torch.inference_mode():
            out, stats = correct(out, a["lst_g"], a.get("mask"), n_iter=k, out=out, return_stats=True)
        if info is None:
            return out
        info["conserve_stats"] = stats
        return out, info
    return call
