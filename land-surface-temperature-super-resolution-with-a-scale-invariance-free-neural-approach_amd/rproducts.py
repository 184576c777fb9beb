"""Patch mining at any ratio (include/sifsr_rproducts.h, csrc/rproducts.hip): ``sifsr.products`` with the side
``hr`` of the fine window as an argument, so that a model can be trained at x3, x2.5 or x2 from the raw integer rasters of a granule.

    decode(lst_raw, nir, red)       Kelvin and NDVI rasters for any fine raster that is p / q of the LST raster
    PatchMiner(window, hr, ...)     census, selection (``sifsrp_select``, unchanged) and gather of the (window, hr) pairs
                                    -> ``products.MinedPatches`` with ``hr`` set: ``statistics``, ``fill``, ``loader``, ``masked_loader``
    patch_counts / expand_valid     the per-patch {n1, n2} of ``rloss.valid_counts`` and the HR mask under an LR mask
    trainable(window, hr)           the rule a pair must meet, or SifsrError naming what failed

The window rules, the acceptance rules and the order of the patches are the reference's (us.split, process_modis.py:88-112,
:172-183, :281-305), which knows x4 only; at ``hr == 4 * window`` the kernels give the bits of ``sifsr.products``.  The epoch loop over
the loaders is ``rloss.train_epoch`` / ``eval_epoch`` / ``fit``.  A pair is trainable when ``ratio.geometry`` accepts it as a tile,
``hr <= 8 * window`` (the fused loss) and the sensor model at ``hr / window`` sees (window, window) of an (hr, hr) patch.
Everything runs on the device; CPU tensors raise SifsrError: there is no CPU path.

Out of scope: a host ``MinedDataset`` at a ratio, a fused batch-assembly kernel (the loader composes existing ops), ratios that
differ per axis, ``GraphedTrainStep`` at a ratio, and bf16."""
from __future__ import annotations

import math

import torch

from . import _lib, gaps, products, ratio, sensor
from .products import QC_MODES, MinedPatches, window_counts


def trainable(window, hr):
    """-> (p, q) with p / q = hr / window in lowest terms, for a pair the whole chain accepts; SifsrError naming the rule that
    failed otherwise (host only)."""
    try:
        window, hr = int(window), int(hr)
    except (TypeError, ValueError):
        raise _lib.SifsrError(f"window and hr must be integers, got {window!r}, {hr!r}") from None
    try:
        g = ratio.geometry((window, window), window, hr)
    except _lib.SifsrError as e:
        raise _lib.SifsrError(f"({window}, {hr}) is not a trainable pair: ratio.geometry refuses it as a tile: {e}") from None
    if hr > 8 * window:
        raise _lib.SifsrError(f"({window}, {hr}) is not a trainable pair: hr <= 8 window is the limit of the fused loss (rloss)")
    got = sensor.lr_shape(hr, hr, hr / window)
    if got != (window, window):
        raise _lib.SifsrError(f"({window}, {hr}) is not a trainable pair: the sensor model at ratio {hr}/{window} sees {got} of an "
                              f"{(hr, hr)} patch, not {(window, window)} (sensor.lr_shape: its crop cuts floor(ceil(factor) / factor) "
                              "cells on each side)")
    return g.p, g.q


def _fine_shape(h, w, fh, fw):
    """the fine raster must be the same rational p / q >= 1 of the LST raster on both axes -> (p, q)"""
    if fh < h or fw < w or fh * w != fw * h:
        raise _lib.SifsrError(f"nir and red {(fh, fw)} must be the same ratio p / q >= 1 of the LST raster {(h, w)} on both axes")
    g = math.gcd(fh, h)
    return fh // g, h // g


def _rasters(lst_raw, nir, red, qc=None):
    lst_raw = products._raster(lst_raw, torch.uint16, "lst_raw")
    nir = products._raster(nir, torch.int16, "nir", lst_raw.device)
    red = products._raster(red, torch.int16, "red", lst_raw.device)
    if nir.shape != red.shape:
        raise _lib.SifsrError(f"nir {tuple(nir.shape)} and red {tuple(red.shape)} differ in shape")
    if qc is not None:
        qc = products._raster(qc, torch.uint8, "qc", lst_raw.device)
        if qc.shape != lst_raw.shape:
            raise _lib.SifsrError(f"qc {tuple(qc.shape)} does not match lst_raw {tuple(lst_raw.shape)}")
    return lst_raw, nir, red, qc


def decode(lst_raw, nir, red, clip=False):
    """``products.decode`` for a fine raster of any size that is the same rational p / q >= 1 (at most 16) of the LST raster on both
    axes: -> (lst_k (h,w), ndvi like nir) float32 device tensors (``sifsrn_decode``), ready for ``ratio.predict_granule``."""
    lst_raw, nir, red, _ = _rasters(lst_raw, nir, red)
    (h, w), (fh, fw) = lst_raw.shape, nir.shape
    p, q = _fine_shape(h, w, fh, fw)
    if p > 16 * q:
        raise _lib.SifsrError(f"decode: the ratio {p}/{q} of {(fh, fw)} over {(h, w)} is above 16")
    lst_k = torch.empty((h, w), dtype=torch.float32, device=lst_raw.device)
    ndvi = torch.empty((fh, fw), dtype=torch.float32, device=lst_raw.device)
    _lib.call("sifsrn_decode", lst_raw, nir, red, lst_k, ndvi, h, w, fh, fw, 1 if clip else 0, _lib.stream_ptr(lst_raw.device))
    return lst_k, ndvi


def patch_counts(valid, hr):
    """valid (N,1,w,w) or (N,w,w) uint8 / bool on the device -> (N,2) int64 on the device: row n = {n1, n2} of patch n, its valid
    cells and the pixels of an hr x hr patch under them -- ``rloss.valid_counts(valid[n:n+1], (hr, hr))`` (``sifsrn_patch_counts``)."""
    if not isinstance(valid, torch.Tensor) or valid.dim() not in (3, 4) or valid.shape[-1] != valid.shape[-2] or valid.shape[0] < 1:
        raise _lib.SifsrError(f"patch_counts: valid must be (N,1,w,w) or (N,w,w), got {getattr(valid, 'shape', type(valid).__name__)}")
    N, w = valid.shape[0], valid.shape[-1]
    if not w <= int(hr) <= ratio.MAX_LST_SIDE:
        raise _lib.SifsrError(f"patch_counts: hr {hr} must lie in {w}..{ratio.MAX_LST_SIDE}")
    v = gaps._valid_raster(valid, (N, w, w) if valid.dim() == 3 else (N, 1, w, w), None, "patch_counts: valid")
    return products._patch_counts(v, w, int(hr))


def expand_valid(valid, size):
    """valid (B,1,h,w) or (B,h,w) uint8 / bool on the device, ``size`` = (H, W) -> uint8 of 0 / 1 shaped (B,1,H,W) or (B,H,W):
    out[Y, X] = valid[Y h // H, X w // W] != 0, the rule of ``ratio.predict_granule_gaps`` and ``rloss`` (``sifsrn_expand_valid``) --
    the HR mask ``metrics.masked_psnr_ssim`` takes at a ratio."""
    if not isinstance(valid, torch.Tensor) or valid.dim() not in (3, 4):
        raise _lib.SifsrError(f"expand_valid: valid must be (B,1,h,w) or (B,h,w), got {getattr(valid, 'shape', type(valid).__name__)}")
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise _lib.SifsrError(f"expand_valid: size must be (H, W), got {size!r}") from None
    B, h, w = valid.shape[0], valid.shape[-2], valid.shape[-1]
    if not (1 <= B <= 65535 and 1 <= h <= H <= ratio.MAX_LST_SIDE and 1 <= w <= W <= ratio.MAX_LST_SIDE):
        raise _lib.SifsrError(f"expand_valid: {tuple(valid.shape)} -> {(H, W)}: needs 1..65535 masks and a size that is no smaller on "
                              f"either axis, at most {ratio.MAX_LST_SIDE}")
    v = gaps._valid_raster(valid, tuple(valid.shape), None, "expand_valid: valid")
    out = torch.empty(tuple(valid.shape[:-2]) + (H, W), dtype=torch.uint8, device=v.device)
    _lib.call("sifsrn_expand_valid", v, out, B, h, w, H, W, _lib.stream_ptr(v.device))
    return out


class PatchMiner:
    """``products.PatchMiner`` for the pairs (LST 1 x ``window`` x ``window``, NDVI 1 x ``hr`` x ``hr``): the same ``add`` / ``finish``
    contract (no transfer in ``add``; one read-back of the count, index and moments per granule in ``finish``), the same
    ``coverage`` and ``qc_mode``.  SifsrError at construction for a pair that is not trainable (``trainable``).  The LST raster
    must have sides that are multiples of q (p / q = hr / window), nir and red are exactly (h p / q, w p / q)."""

    def __init__(self, window, hr, coverage=0.0, qc_mode="MOD21A1D"):
        if qc_mode not in QC_MODES:
            raise ValueError(f"qc_mode must be one of {sorted(QC_MODES)}, got {qc_mode!r}")
        if not 0.0 <= coverage <= 1.0:
            raise ValueError(f"coverage must be in [0, 1], got {coverage}")
        self.p, self.q = trainable(window, hr)
        if int(window) % 4:
            raise _lib.SifsrError(f"window must be a multiple of 4 for the selection (sifsrp_select), got {window}")
        self.window, self.hr, self.coverage, self.qc_mode = int(window), int(hr), float(coverage), qc_mode
        self.max_bad = int(math.floor(self.coverage * self.window ** 2))    # count <= coverage * window**2 on an integer count
        self._granules = []

    def add(self, lst_raw, nir, red, qc=None, granule_id=None):
        """Enqueue census, select and gather of one granule on the current stream.  Returns the granule's device buffers (counts
        (nwin,2), index (nfull,3), n_accepted (1)) for inspection; nothing is read back here."""
        lst_raw, nir, red, qc = _rasters(lst_raw, nir, red, qc)
        mode = QC_MODES[self.qc_mode]
        if mode == 1 and qc is None:
            raise ValueError("qc_mode 'MOD11A1' needs the QC raster")
        ws, hr, (h, w) = self.window, self.hr, lst_raw.shape
        if h < ws or w < ws or h > ratio.MAX_LST_SIDE or w > ratio.MAX_LST_SIDE:
            raise _lib.SifsrError(f"the raster ({h}, {w}) must have sides in {ws} (one window) .. {ratio.MAX_LST_SIDE}")
        if h % self.q or w % self.q:
            raise _lib.SifsrError(f"both sides of the LST raster ({h}, {w}) must be multiples of q = {self.q} ({hr}/{ws} = {self.p}/{self.q})")
        fine = (h // self.q * self.p, w // self.q * self.p)
        if tuple(nir.shape) != fine:
            raise _lib.SifsrError(f"nir and red must be exactly {fine} ({self.p}/{self.q} of the LST raster ({h}, {w})), got {tuple(nir.shape)}")
        nwin, cap = window_counts(h, w, ws)
        dev, s = lst_raw.device, _lib.stream_ptr(lst_raw.device)
        g = {"id": len(self._granules) if granule_id is None else int(granule_id),
             "counts": torch.empty((nwin, 2), dtype=torch.int32, device=dev),
             "index": torch.empty((cap, 3), dtype=torch.int32, device=dev),
             "n_accepted": torch.empty((1,), dtype=torch.int32, device=dev),
             "lst": torch.empty((cap, 1, ws, ws), dtype=torch.float32, device=dev),
             "ndvi": torch.empty((cap, 1, hr, hr), dtype=torch.float32, device=dev),
             "moments": torch.empty((cap, 8), dtype=torch.float64, device=dev)}
        _lib.call("sifsrn_census", lst_raw, qc, nir, red, g["counts"], h, w, ws, hr, mode, s)
        _lib.call("sifsrp_select", g["counts"], g["index"], g["n_accepted"], h, w, ws, self.max_bad, cap, s)
        _lib.call("sifsrn_gather", lst_raw, nir, red, g["index"], g["n_accepted"], g["lst"], g["ndvi"], g["moments"], h, w, ws, hr, cap, s)
        self._granules.append(g)
        return g

    def finish(self):
        """-> ``products.MinedPatches`` (``hr`` set) of everything added so far, in the order added; the miner is empty afterwards."""
        hold = products.PatchMiner.finish(self)                            # (one read-back and one concatenation for both miners)
        return MinedPatches(hold.lst, hold.ndvi, hold.index, hold.moments, self.window, self.hr)
