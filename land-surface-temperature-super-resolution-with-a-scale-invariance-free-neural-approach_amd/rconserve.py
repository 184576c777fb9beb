"""Does the super-resolved raster conserve the observed one, at any ratio? (include/sifsr_rconserve.h,
csrc/rconserve.hip)

``sifsr.conserve`` with the sensor model of ``sifsr.degrade`` in the place of the /4 one and the exact-phase bicubic of
``sifsr.ratio`` in the place of the x4 one: what a model trained with ``rloss.train_step`` at x3, x2.5 or x2 is trained on,
``Huber(D(SR), LST)``, measured and enforced on a whole raster with gaps.  The ratio is taken from the two shapes:

    consistency   the residual ``r = lst - D(sr)`` over the cells whose whole stencil is valid and away from the zero ring, reduced
                  to (count, bias, RMSE, max |r|) in float64
    conserve      ``n_iter`` steps of ``sr += relax * U(r)`` (U: ``ratio.upsample``, bit for bit) at the pixels of valid cells;
                  every other pixel keeps its bits

``D`` is ``sensor.downscale`` / ``degrade.downscale_lst`` for ``factor = H / h`` with the crop (``sifsrs_degrade``, hkw = 0), so sr
``(H, W)`` and lst ``(h, w)`` must be a pair ``sensor.lr_shape`` gives: 1 < H / h = W / w <= 8.  A cell is an LST pixel (i, j) and
the sr pixels (Y, X) with ``(Y h // H, X w // W) == (i, j)``; it is valid iff the LST pixel is finite, not 0 K and kept by ``mask``
and every sr pixel of it is finite and not 0.  What invalid pixels hold changes no output bit.  ``H == 4 h`` is allowed and runs
these kernels; ``sifsr.conserve`` keeps its kernels, bits and refusals.  Nothing is read back: the statistics stay on the device.
CPU-only use raises SifsrError: there is no fallback.

Out of scope here: ``hkw`` in the operator, batches of rasters, ratios above 8, rerouting ``conserve=`` of the x4 calls, bf16.
"""
from __future__ import annotations

import torch

from . import _lib
from . import conserve as _x4

MAX_ITER = 64
MAX_FACTOR = 8.0


def _call(sr, lst, mask, out, n_iter, relax, mtf):
    """-> (stats (n_iter+1, 4) float64, workspace) after one ``sifsrc_conserve``"""
    _lib.require_gpu(sr, "sr"); _lib.require_gpu(lst, "lst")
    if lst.dim() != 2 or sr.dim() != 2:
        raise _lib.SifsrError(f"expected lst (h,w) and sr (H,W), got {tuple(lst.shape)} and {tuple(sr.shape)}")
    if sr.device != lst.device:
        raise _lib.SifsrError(f"sr is on {sr.device}, lst on {lst.device}")
    (h, w), (H, W) = lst.shape, sr.shape
    n_iter = int(n_iter)
    if not 0 <= n_iter <= MAX_ITER:
        raise _lib.SifsrError(f"n_iter must be in 0..{MAX_ITER}, got {n_iter}")
    if not 0.0 < float(mtf) < 1.0:
        raise _lib.SifsrError(f"mtf must be in (0, 1), got {mtf}")
    need = _lib.call("sifsrc_workspace_bytes", h, w, H, W, n_iter)
    if need == 0:
        raise _lib.SifsrError(f"lst {(h, w)} is not the sensor's view of sr {(H, W)}: need H / h == W / w in (1, {MAX_FACTOR:g}] and "
                              f"(h, w) == sensor.lr_shape(H, W, H / h), sides <= 16384")
    if mask is not None:
        from .gaps import _valid_raster
        mask = _valid_raster(mask, (h, w), lst.device, "mask")
    ws = torch.empty((need,), dtype=torch.uint8, device=lst.device)
    stats = torch.empty((n_iter + 1, 4), dtype=torch.float64, device=lst.device)
    _lib.call("sifsrc_conserve", sr, lst, mask, out, stats, ws, need, h, w, H, W, float(mtf), float(relax), n_iter,
              _lib.stream_ptr(lst.device))
    return stats, ws


def consistency(sr, lst, mask=None, mtf=0.1, return_residual=False):
    """sr (H,W) [K], lst (h,w) [K], mask (h,w) uint8 / bool or None (non-zero = keep) -> the float64 device tensor
    (count, bias, RMSE, max |r|) of ``r = lst - D(sr)`` over the counted cells (count 0: NaN in the other three).
    ``return_residual``: also r (h,w) float32, 0 where the cell is not counted."""
    stats, ws = _call(sr, lst, mask, None, 0, 1.0, mtf)
    if return_residual:
        h, w = lst.shape
        return stats[0], ws[:4 * h * w].view(torch.float32).view(h, w).clone()
    return stats[0]


def conserve(sr, lst, mask=None, n_iter=1, relax=1.0, mtf=0.1, out=None, return_stats=False):
    """``n_iter`` correction steps ``sr += relax * U(lst - D(sr))`` at the pixels of valid cells -> the corrected raster (H,W);
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


def granule_option(fn):
    """``conserve.granule_option`` for the whole-granule calls at a ratio (``ratio.predict_granule``,
    ``ratio.predict_granule_gaps``): the keyword-only option ``conserve=k`` runs k steps of ``rconserve.conserve`` on the blended
    raster, in place, against the call's own ``lst_g`` (and ``mask``).  ``conserve=0``, the default, is the undecorated call."""
    return _x4.granule_option(fn, correct=conserve)
