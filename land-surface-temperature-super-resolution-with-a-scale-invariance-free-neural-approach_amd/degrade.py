"""The sensor model at any ratio (include/sifsr_degrade.h, csrc/degrade.hip): what a coarser sensor sees of a
fine raster.  The reference's ``downscale_Aster_to_coarse`` (90 m -> 926.25 m, utils.py:1759-1793), ``downscale_Aster_to_fine``
(90 m -> 231.656 m, :1796-1830) and ``generic_downscale`` (:1642-1668), and with ``crop`` the cut of ``downscale_LST_SR_to_LR``
(:1671-1706) at any factor:

    reflect pad by hw = hkw or ceil(factor)  ->  Gaussian PSF of ``mtf`` at the target Nyquist frequency with padding="same" on the
    padded raster (its outer hw-wide ring is darkened by zeros, as in the reference)  ->  bicubic resampling by 1 / factor with
    ``F.interpolate`` semantics (A = -0.75, fp32 source coordinates, clamped indices)  ->  optionally the cut of int(hw / factor)

as one banded operator per axis, in float64 on the device.  ``valid`` marks the pixels that hold data (an ASTER scene is a rotated
quadrilateral in a zero-filled raster): an output is valid iff everything its stencil reads is valid and it touches nothing of the
zero ring; invalid outputs hold ``fill_value`` and what invalid pixels hold changes no valid output bit.  No autograd.  CPU-only use
raises SifsrError: there is no fallback."""
from __future__ import annotations

import ctypes

import torch

from . import _lib

COARSE_FACTOR = 926.25 / 90     # ASTER 90 m -> MODIS 1 km (926.25 m)
FINE_FACTOR = 231.656 / 90      # ASTER 90 m -> MODIS 250 m (231.656 m)
MAX_FACTOR, MAX_HALF_WIDTH, MAX_SIDE = 16.0, 16, 16384


def _hkw(hkw):
    if hkw is None:
        return 0
    if int(hkw) != hkw or not 1 <= int(hkw) <= MAX_HALF_WIDTH:
        raise _lib.SifsrError(f"hkw must be None or an integer in 1..{MAX_HALF_WIDTH}, got {hkw}")
    return int(hkw)


def output_shape(h, w, factor, hkw=None, crop=False):
    """-> (oh, ow), the size of ``degrade`` of an (h, w) raster.  SifsrError outside the limits: 1 < factor <= 16, half width
    hw = hkw or ceil(factor) in 1..16, hw + 1 <= h, w <= 16384, both output sides >= 1."""
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    fn = _lib.lib().sifsrs_out_shape
    if fn(int(h), int(w), float(factor), _hkw(hkw), int(bool(crop)), ctypes.byref(oh), ctypes.byref(ow)) != 0:
        raise _lib.SifsrError(f"degrade: raster {(int(h), int(w))}, factor {factor}, hkw {hkw}, crop {bool(crop)} is outside the limits "
                              f"(1 < factor <= {MAX_FACTOR:g}, half width hw = hkw or ceil(factor) in 1..{MAX_HALF_WIDTH}, "
                              f"hw + 1 <= side <= {MAX_SIDE}, an output of at least 1 x 1)")
    return oh.value, ow.value


def degrade(x, factor, mtf=0.1, hkw=None, crop=False, valid=None, fill_value=float("nan"), return_valid=False):
    """x (H,W), (B,H,W) or (B,C,H,W) float32 on the device -> the raster seen at ``factor`` times the pixel size, same leading
    dimensions.  ``valid``: uint8 / bool, (H,W) for every image or shaped as x, non-zero = holds data; outputs whose stencil reads an
    invalid pixel or the zero ring hold ``fill_value``.  Without ``valid`` every value is the reference's, darkened ring included.
    ``return_valid``: also the uint8 map of the valid outputs (shaped as the result; it marks the ring also without ``valid``)."""
    if not isinstance(x, torch.Tensor):
        raise _lib.SifsrError(f"degrade: expected a tensor, got {type(x).__name__}")
    if x.requires_grad:
        raise NotImplementedError("degrade has no backward: detach the raster (the differentiable /4 sensor model is "
                                  "sifsr.downscale_LST_SR_to_LR)")
    _lib.require_gpu(x, "x")
    if x.dim() not in (2, 3, 4):
        raise _lib.SifsrError(f"degrade: expected (H,W), (B,H,W) or (B,C,H,W), got {tuple(x.shape)}")
    if not 0.0 < float(mtf) < 1.0:
        raise _lib.SifsrError(f"mtf must be in (0, 1), got {mtf}")
    lead, (H, W) = tuple(x.shape[:-2]), x.shape[-2:]
    B = 1
    for d in lead:
        B *= d
    oh, ow = output_shape(H, W, factor, hkw, crop)
    if B < 1:
        raise _lib.SifsrError(f"degrade: empty batch {tuple(x.shape)}")
    hk, crop = _hkw(hkw), int(bool(crop))
    v = None
    if valid is not None:
        from .gaps import _valid_raster
        if isinstance(valid, torch.Tensor) and valid.dim() == 2 and len(lead):
            v = _valid_raster(valid, (H, W), x.device).expand(*lead, H, W).contiguous()
        else:
            v = _valid_raster(valid, tuple(x.shape), x.device)
    need = _lib.call("sifsrs_workspace_bytes", B, H, W, float(factor), hk, crop)
    if need == 0:
        raise _lib.SifsrError(f"degrade: a batch of {B} images is outside the limits (1..65535)")
    ws = torch.empty((need,), dtype=torch.uint8, device=x.device)
    out = torch.empty(lead + (oh, ow), dtype=torch.float32, device=x.device)
    ov = torch.empty(lead + (oh, ow), dtype=torch.uint8, device=x.device) if return_valid else None
    _lib.call("sifsrs_degrade", x, v, out, ov, ws, need, B, H, W, float(factor), float(mtf), hk, crop, float(fill_value),
              _lib.stream_ptr(x.device))
    return (out, ov) if return_valid else out


def aster_to_coarse(x, valid=None):
    """``downscale_Aster_to_coarse`` (utils.py:1759-1793): 90 m -> 926.25 m, mtf 0.1, a 23 x 23 PSF.  With ``valid``: ->
    (raster, valid map)."""
    return degrade(x, COARSE_FACTOR, valid=valid, return_valid=valid is not None)


def aster_to_fine(x, valid=None):
    """``downscale_Aster_to_fine`` (utils.py:1796-1830): 90 m -> 231.656 m, mtf 0.1, a 7 x 7 PSF.  With ``valid``: ->
    (raster, valid map)."""
    return degrade(x, FINE_FACTOR, valid=valid, return_valid=valid is not None)


def generic_downscale(x, factor=2.0, mtf=0.1, hkw=3):
    """``generic_downscale`` (utils.py:1642-1668) without its ``padding`` argument ("same" is what the reference runs with)."""
    return degrade(x, factor, mtf=mtf, hkw=hkw)


def simulate_pair(aster_90m, valid=None):
    """One 90 m scene -> (coarse, fine, coarse_valid, fine_valid): the simulated 1 km observation and the 250 m raster it is scored
    against, each with the map of the outputs that read only valid pixels and nothing of the zero ring."""
    coarse, cv = degrade(aster_90m, COARSE_FACTOR, valid=valid, return_valid=True)
    fine, fv = degrade(aster_90m, FINE_FACTOR, valid=valid, return_valid=True)
    return coarse, fine, cv, fv
