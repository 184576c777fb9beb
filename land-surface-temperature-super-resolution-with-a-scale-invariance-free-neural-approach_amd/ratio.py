"""Whole-granule prediction at any ratio (include/sifsr_ratio.h, csrc/ratio.hip): what a model trained with
``sensor.train_step(..., factor=3)`` -- or 2.5, or 2 -- needs to be used: a granule goes in at ratio ``hr / window`` and the
super-resolved raster comes out, seamless and gap-aware.

    upsample(x, size)       bicubic resampling to any larger size with an EXACT phase (the operator of ``F.interpolate(size=...,
                            mode="bicubic", align_corners=False)``; torch rounds the scale and the source coordinate per pixel)
    geometry(...)           the tile layout at ratio p / q = hr / window: (p, q, tiles, hr_shape), or SifsrError
    prepare_tiles           the training-batch form: (T,1,w,w) and (T,1,P,P) -> (T,2,P,P)
    granule_to_tiles / blend_tiles / predict_granule / predict_granule_gaps
                            ``pipeline.granule_to_tiles`` / ``pipeline.blend_tiles`` / ``predict.predict_granule`` /
                            ``gaps.predict_granule_gaps`` with the tile side ``hr`` as an argument, on the drivers of ``_granule``

A tile is ``window`` LST pixels and ``hr`` network pixels on a side.  The rules (``sifsrr_geometry``): 1 <= window <= 64; hr a
multiple of 8 in 24..256 with window < hr <= 16 window; with p / q = hr / window in lowest terms, both sides of the LST raster and
``overlap`` are multiples of q, 0 <= 2 overlap <= window, and the NDVI raster is exactly (h p / q, w p / q).  ``hr == 4 * window``
is allowed and runs these kernels; the x4 functions of ``pipeline`` / ``predict`` / ``gaps`` keep theirs.  Everything is fp32 on the
device; CPU tensors raise SifsrError: there is no CPU path.

Fine-tuning on a granule at a ratio and masks in the loss at a ratio are ``sifsr.rloss``; the consistency check
and the residual correction at a ratio are ``sifsr.rconserve`` (§9 f20), which the two granule calls take as the keyword-only
option ``conserve=k``; mining training patches at a ratio, their loaders and the epoch loop are ``sifsr.rproducts`` and
``rloss.train_epoch`` / ``fit`` (§9 f22); ``GranulePredictor`` here is the two granule calls captured into a hipGraph, the
gap-aware one with no host synchronisation, and ``rloss.GraphedTrainStep`` the captured training step (§9 f23).  Out of scope here:
ratios that are not ``hr / window`` for such a pair (926.25 / 90 and 231.656 / 90 stay with ``sifsr.degrade``), rerouting the
drop-ins, and bf16."""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

from . import _granule, _lib, gaps, rconserve
from .rconserve import granule_option
from .pipeline import _UNIT, _stats4, _tile_buffer

Geometry = namedtuple("Geometry", "p q tiles hr_shape")
MAX_LST_SIDE = 16384


def geometry(lst_shape, window, hr, overlap=0, cover_edges=False):
    """-> Geometry(p, q, (tiles_y, tiles_x), (H, W)) of an LST raster ``lst_shape`` cut into tiles of ``window`` LST pixels =
    ``hr`` network pixels (``sifsrr_geometry``: host only); SifsrError for any violation of the rules in the module docstring."""
    try:
        h, w = (int(v) for v in lst_shape)
        window, hr, overlap = int(window), int(hr), int(overlap)
    except (TypeError, ValueError):
        raise _lib.SifsrError(f"geometry: expected an (h, w) shape and integer window / hr / overlap, got {lst_shape!r}, {window!r}, "
                              f"{hr!r}, {overlap!r}") from None
    out6 = (ctypes.c_int * 6)()
    rc = _lib.lib().sifsrr_geometry(h, w, window, hr, overlap, 1 if cover_edges else 0, out6)
    if rc != 0:
        raise _lib.SifsrError(
            f"no tile layout for an LST raster {(h, w)} at window {window}, hr {hr}, overlap {overlap}: need 1 <= window <= 64, hr a "
            f"multiple of 8 in 24..256 with window < hr <= 16 window, and with p / q = hr / window in lowest terms both raster sides "
            f"(window..{MAX_LST_SIDE}) and the overlap multiples of q, 0 <= 2 overlap <= window (status {rc})")
    p, q, ty, tx, H, W = out6
    return Geometry(p, q, (ty, tx), (H, W))


def _layout(lst_g, ndvi_shape, window, hr, overlap, cover_edges):
    """validation shared by the granule entry points (before any launch) -> Geometry"""
    if lst_g.dim() != 2:
        raise _lib.SifsrError(f"lst granule: expected a 2-D raster, got {tuple(lst_g.shape)}")
    g = geometry(lst_g.shape, window, hr, overlap, cover_edges)
    if ndvi_shape is not None and tuple(ndvi_shape) != g.hr_shape:
        raise _lib.SifsrError(f"ndvi granule must be {g.hr_shape} ({g.p}/{g.q} of the LST granule {tuple(lst_g.shape)}), got "
                              f"{tuple(ndvi_shape)}")
    return g


def _tile_layout(lst_g, ndvi_shape, window, hr, overlap, cover_edges):
    """-> the ``_granule.Layout`` at ratio hr / window of the raster ``lst_g``, or ``_layout``'s SifsrError"""
    return _layout_record(_layout(lst_g, ndvi_shape, window, hr, overlap, cover_edges), lst_g.shape, window, hr, overlap, cover_edges)


def _layout_record(g, shape, window, hr, overlap, cover_edges):
    """the ``_granule.Layout`` of an LST raster of ``shape`` whose ``geometry`` is ``g``"""
    lay = (overlap, cover_edges)
    return _granule.Layout(
        window, hr, overlap, cover_edges, g.tiles, g.hr_shape,
        lambda lst_g, ndvi_g, stats, out=None: granule_to_tiles(lst_g, ndvi_g, stats, window, hr, True, *lay, out)[0],
        lambda filled, ndvi_g, stats, active, n_active, cap, out=None: prepare_active_tiles(filled, ndvi_g, stats, active, n_active, cap, window,
                                                                                          hr, *lay, out=out),
        lambda sr, stats, out=None: blend_tiles(sr, shape, window, hr, stats, *lay, out),
        lambda sr, slot, valid, stats, fill_value: blend_active_tiles(sr, slot, valid, window, hr, stats, *lay, fill_value))


def upsample(x, size):
    """Bicubic resampling of x (h,w), (B,h,w) or (B,C,h,w) float32 on the device to ``size = (H, W)``, H >= h and W >= w, each axis
    with its own ratio (``sifsrr_upsample``): A = -0.75, half-pixel centres, indices clamped to the raster -- the operator of
    ``F.interpolate(x, size=(H, W), mode="bicubic", align_corners=False)`` with the phase of every output taken in integers, so an
    axis with H == h is a bit-exact copy and the result is the float64 operator's to fp32 rounding at every ratio.

    This is the ``lst_up`` of ``sensor.train_step``: ``ratio.upsample(lst, (H, W))``."""
    if not isinstance(x, torch.Tensor):
        raise _lib.SifsrError(f"upsample: expected a tensor, got {type(x).__name__}")
    _lib.require_gpu(x, "x")
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise _lib.SifsrError(f"upsample: size must be (H, W), got {size!r}") from None
    if x.dim() not in (2, 3, 4):
        raise _lib.SifsrError(f"upsample: expected (h,w), (B,h,w) or (B,C,h,w), got {tuple(x.shape)}")
    h, w = x.shape[-2:]
    B = x.numel() // max(1, h * w)
    if B < 1 or h < 1 or w < 1 or H < h or W < w or h > MAX_LST_SIDE or w > MAX_LST_SIDE or H > 2 * MAX_LST_SIDE or W > 2 * MAX_LST_SIDE:
        raise _lib.SifsrError(f"upsample: {tuple(x.shape)} -> {(H, W)}: needs a non-empty raster of sides <= {MAX_LST_SIDE} and a size "
                              f"that is no smaller on either axis, at most {2 * MAX_LST_SIDE}")
    out = torch.empty(tuple(x.shape[:-2]) + (H, W), dtype=torch.float32, device=x.device)
    for b in range(0, B, 65535):                                        # (one launch holds 65535 images)
        n = min(65535, B - b)
        _lib.call("sifsrr_upsample", x.reshape(B, h, w)[b:b + n], out.view(B, H, W)[b:b + n], n, h, w, H, W, _lib.stream_ptr(x.device))
    return out


def prepare_tiles(lst, ndvi, stats=None, clip_ndvi=False):
    """lst (T,1,w,w), ndvi (T,1,P,P) -> model input (T,2,P,P) = cat(upsample(z(lst), (P, P)), z(clip(ndvi))): the training-batch
    form of ``granule_to_tiles``, as a column of T one-tile rasters (``sifsrr_tiles_prepare``; one device function with
    ``upsample``).  ``stats=None``: inputs are already normalised."""
    for t, n in ((lst, "lst"), (ndvi, "ndvi")):
        if not isinstance(t, torch.Tensor):
            raise _lib.SifsrError(f"prepare_tiles: {n} must be a tensor, got {type(t).__name__}")
    _lib.require_gpu(lst, "lst"); _lib.require_gpu(ndvi, "ndvi")
    if lst.dim() != 4 or ndvi.dim() != 4 or lst.shape[1] != 1 or lst.shape[2] != lst.shape[3] or ndvi.shape[2] != ndvi.shape[3] \
            or tuple(ndvi.shape[:2]) != (lst.shape[0], 1) or lst.shape[0] < 1:
        raise _lib.SifsrError(f"prepare_tiles expects lst (T,1,w,w) and ndvi (T,1,P,P); got {tuple(lst.shape)}, {tuple(ndvi.shape)}")
    T, w, P = lst.shape[0], lst.shape[2], ndvi.shape[2]
    geometry((w, w), w, P)
    x = torch.empty((T, 2, P, P), dtype=torch.float32, device=lst.device)
    step = max(1, MAX_LST_SIDE // w)                                     # tiles per launch: a raster of (step w, w) LST pixels
    for b in range(0, T, step):
        n = min(step, T - b)
        _lib.call("sifsrr_tiles_prepare", lst[b:b + n], ndvi[b:b + n], x[b:b + n], None, None, n, n * w, w, w, P, 0, 0,
                  *_stats4(stats or _UNIT), 1 if clip_ndvi else 0, _lib.stream_ptr(lst.device))
    return x


def granule_to_tiles(lst_g, ndvi_g, stats, window, hr, clip_ndvi=True, overlap=0, cover_edges=False, out=None):
    """Raw granule rasters lst_g (h,w) [K] and ndvi_g (h p/q, w p/q) -> (x (T,2,hr,hr), (tiles_y, tiles_x)): the tiles of
    ``pipeline.tile_origins`` along each axis, each one z-scored, resampled to hr x hr clamped at the tile and concatenated with
    its clipped, z-scored NDVI block -- what ``prepare_tiles`` gives for the same block.  ``out``: a buffer of at least T tiles to
    write into; the first T tiles of it are returned."""
    _lib.require_gpu(lst_g, "lst granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    g = _layout(lst_g, ndvi_g.shape, window, hr, overlap, cover_edges)
    ty, tx = g.tiles
    x = _tile_buffer(out, ty * tx, 2, hr, lst_g.device, "tile buffer")
    h, w = lst_g.shape
    _lib.call("sifsrr_tiles_prepare", lst_g, ndvi_g, x, None, None, ty * tx, h, w, window, hr, overlap, 1 if cover_edges else 0,
              *_stats4(stats), 1 if clip_ndvi else 0, _lib.stream_ptr(lst_g.device))
    return x, (ty, tx)


def prepare_active_tiles(filled, ndvi_g, stats, active, n_active, cap, window, hr, overlap=0, cover_edges=False, clip_ndvi=True, out=None):
    """-> x (cap,2,hr,hr): x[i] = the network input of tile active[i] for i < min(n_active, cap), the rest untouched; bit-identical
    to that tile of ``granule_to_tiles(filled, ...)``.  ``active`` / ``n_active``: as ``gaps.select_tiles`` left them.  ``out``: a
    buffer of at least ``cap`` tiles to write into (a captured run's static one); its first ``cap`` tiles are returned."""
    _lib.require_gpu(filled, "filled granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    _layout(filled, ndvi_g.shape, window, hr, overlap, cover_edges)
    if int(cap) < 1:
        raise _lib.SifsrError(f"cap must be positive, got {cap}")
    h, w = filled.shape
    x = _tile_buffer(out, int(cap), 2, hr, filled.device, "tile buffer")
    _lib.call("sifsrr_tiles_prepare", filled, ndvi_g, x, active, n_active, int(cap), h, w, window, hr, overlap, 1 if cover_edges else 0,
              *_stats4(stats), 1 if clip_ndvi else 0, _lib.stream_ptr(filled.device))
    return x


def blend_tiles(sr, lst_shape, window, hr, stats, overlap=0, cover_edges=False, out=None):
    """sr (T,1,hr,hr) normalised predictions of the tiles of ``granule_to_tiles`` -> the de-normalised raster (h p/q, w p/q) [K]:
    the normalised feathered blend of ``pipeline.blend_tiles`` with tile side hr and HR overlap ``overlap p / q``
    (``sifsrr_tiles_blend``), every pixel written, pixels no tile covers 0."""
    _lib.require_gpu(sr, "sr")
    g = geometry(lst_shape, window, hr, overlap, cover_edges)
    ty, tx = g.tiles
    if tuple(sr.shape) != (ty * tx, 1, hr, hr):
        raise _lib.SifsrError(f"sr must be {(ty * tx, 1, hr, hr)} for this layout, got {tuple(sr.shape)}")
    if out is None:
        out = torch.empty(g.hr_shape, dtype=torch.float32, device=sr.device)
    _lib.require_gpu(out, "output granule")
    if tuple(out.shape) != g.hr_shape:
        raise _lib.SifsrError(f"output granule must be {g.hr_shape}, got {tuple(out.shape)}")
    h, w = (int(v) for v in lst_shape)
    _lib.call("sifsrr_tiles_blend", sr, None, None, out, h, w, window, hr, overlap, 1 if cover_edges else 0, float(stats["mean_lst"]),
              float(stats["std_lst"]), 0.0, _lib.stream_ptr(sr.device))
    return out


def blend_active_tiles(sr, slot, valid, window, hr, stats, overlap=0, cover_edges=False, fill_value=float("nan")):
    """sr (>= n_active,1,hr,hr) normalised predictions in the order of ``active`` -> the de-normalised raster [K]: ``blend_tiles``
    at the pixels of valid LST cells -- cell (Y q // p, X q // p) of output pixel (Y, X) --, ``fill_value`` at the others."""
    _lib.require_gpu(sr, "sr")
    if not isinstance(valid, torch.Tensor) or valid.dim() != 2:
        raise _lib.SifsrError("valid must be a 2-D tensor")
    g = geometry(valid.shape, window, hr, overlap, cover_edges)
    valid = gaps._valid_raster(valid, valid.shape, sr.device)
    ty, tx = g.tiles
    if sr.dim() != 4 or sr.shape[0] < 1 or tuple(sr.shape[1:]) != (1, hr, hr):
        raise _lib.SifsrError(f"sr must be (n_active, 1, {hr}, {hr}), got {tuple(sr.shape)}")
    if not isinstance(slot, torch.Tensor) or slot.dtype != torch.int32 or tuple(slot.shape) != (ty * tx,) or slot.device != sr.device:
        raise _lib.SifsrError(f"slot must be an int32 device tensor {(ty * tx,)}")
    h, w = valid.shape
    out = torch.empty(g.hr_shape, dtype=torch.float32, device=sr.device)
    _lib.call("sifsrr_tiles_blend", sr, slot.contiguous(), valid, out, h, w, window, hr, overlap, 1 if cover_edges else 0,
              float(stats["mean_lst"]), float(stats["std_lst"]), float(fill_value), _lib.stream_ptr(sr.device))
    return out


@granule_option
@torch.inference_mode()
def predict_granule(model, lst_g, ndvi_g, stats, window=64, hr=192, batch=256, overlap=0, cover_edges=False):
    """``predict.predict_granule`` at ratio ``hr / window``: raw LST raster (h,w) [K] + raw NDVI raster (h p/q, w p/q) ->
    super-resolved LST raster (h p/q, w p/q) [K].  Tiles are cut, normalised, resampled and concatenated by one kernel, pushed
    through the network in eval mode in batches of ``batch``, then de-normalised and blended by another; ``overlap`` (LST pixels,
    a multiple of q, 0..window/2) and ``cover_edges`` are those of ``predict.predict_granule``.

    Keyword-only ``conserve=k`` (``rconserve.granule_option``): k steps of ``rconserve.conserve`` on the blended raster (cells of
    0 K / non-finite LST pixels and the pixels no tile reached keep their bits); 0, the default: none."""
    _lib.require_gpu(lst_g, "lst granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    lay = _tile_layout(lst_g, ndvi_g.shape, window, hr, overlap, cover_edges)                 # (raises before any launch)
    if int(batch) < 1:
        raise _lib.SifsrError(f"batch must be positive, got {batch}")
    model.eval()
    return _granule.predict(model, lay, lst_g, ndvi_g, stats, int(batch))


@granule_option
@torch.inference_mode()
def predict_granule_gaps(model, lst_g, ndvi_g, stats, mask=None, window=64, hr=192, batch=256, overlap=16, cover_edges=True,
                         fill_value=float("nan"), return_info=False):
    """``gaps.predict_granule_gaps`` at ratio ``hr / window``: raw LST raster (h,w) [K] with cloud / ocean / fill pixels as 0 K,
    NaN or inf (and whatever ``mask`` rules out) + raw NDVI raster (h p/q, w p/q) -> the super-resolved raster, ``fill_value`` at
    every output pixel (Y, X) whose LST cell (Y q // p, X q // p) is invalid.

    ``gaps.fill_gaps`` and ``gaps.select_tiles`` run unchanged (they see only the LST raster; ``window`` must be a multiple of 4
    for the selection, ``overlap`` a multiple of q); then the network input of the active tiles only, ceil(n_active / batch)
    eval-mode forwards and the masked blend.  The read of the active count is the call's only host synchronisation.  At valid
    pixels the result is bit-identical to ``predict_granule`` on the filled raster with the same layout; nothing valid: the
    all-``fill_value`` raster, no forward.

    ``return_info``: also {"valid": bool (h,w) device tensor, "n_active": int, "n_tiles": int}.

    Keyword-only ``conserve=k`` (``rconserve.granule_option``): k residual-correction steps on the blended raster
    (``rconserve.conserve`` with the same ``mask``: only cells whose LST pixel is valid move, and the correction fades out towards
    a gap); with ``return_info`` the statistics are ``info["conserve_stats"]``.  0, the default: none."""
    _lib.require_gpu(lst_g, "lst granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    lay = _tile_layout(lst_g, ndvi_g.shape, window, hr, overlap, cover_edges)                 # (raises before any launch)
    if int(window) % 4:
        raise _lib.SifsrError(f"window must be a multiple of 4 for the tile selection, got {window}")
    if int(batch) < 1:
        raise _lib.SifsrError(f"batch must be positive, got {batch}")
    model.eval()
    return _granule.predict_gaps(model, lay, lst_g, ndvi_g, stats, mask, int(batch), fill_value, return_info)


class GranulePredictor(_granule.CapturedGranule):
    """``predict_granule`` -- or, with ``gaps=True``, ``predict_granule_gaps`` -- at ratio ``hr / window`` for ONE granule shape,
    captured into a hipGraph and replayed per granule (``predict.GranulePredictor`` is the x4 one).  All buffers
    are static; the tiles are padded to a whole number of batches, so every forward has the captured batch shape.  ``conserve=k``:
    k ``rconserve.conserve`` steps inside the captured chain (with the mask, when there are gaps).

    ``gaps=False``: ``__call__(lst_g, ndvi_g)`` -> a clone of the raster, the bits of ``predict_granule`` with the same arguments.
    ``gaps=True``: ``__call__(lst_g, ndvi_g, mask=None, return_info=False)`` -> the bits of ``predict_granule_gaps`` -- at the
    ``fill_value`` pixels too -- with NO read of the active count: every slot is forwarded and only the active ones are read
    (``_granule.predict_gaps_fixed``), so granules can follow each other without a host synchronisation, at the price of the
    forwards of the inactive tiles.  ``info``: "valid" and "n_tiles" as the eager call gives them, "n_active" as a (1,) int32
    DEVICE tensor.  Everything ``geometry`` refuses is refused here, before any launch; a raster of another shape in the call.

    Which to use (one MI355X, 625 tiles at (64, 192)): give the captured form a ``batch`` that divides the tile count
    -- at batch 256 it forwards 768 slots, 11.8 ms against 10.3 ms at batch 125.  With 550 of the 625 tiles active the eager
    ``predict_granule_gaps`` takes 9.3 ms and the best replay 10.3 ms; with 619 active both take 10.3 ms.  The eager call is the one
    for gappy granules; the captured one for nearly full granules or a host that must not block."""

    def __init__(self, model, lst_shape, stats, window=64, hr=192, overlap=0, cover_edges=False, batch=256, conserve=0, gaps=False,
                 fill_value=float("nan"), device=None):
        g = geometry(lst_shape, window, hr, overlap, cover_edges)
        window, hr, overlap, cover_edges = int(window), int(hr), int(overlap), bool(cover_edges)
        if gaps and window % 4:
            raise _lib.SifsrError(f"window must be a multiple of 4 for the tile selection, got {window}")
        if int(batch) < 1:
            raise _lib.SifsrError(f"batch must be positive, got {batch}")
        if not 0 <= int(conserve) <= rconserve.MAX_ITER:
            raise _lib.SifsrError(f"conserve must be a step count in 0..{rconserve.MAX_ITER}, got {conserve}")
        dev = device or next(model.parameters()).device
        self.lst_shape, self.window, self.hr, self.overlap, self.cover_edges = tuple(int(v) for v in lst_shape), window, hr, overlap, cover_edges
        lay = _layout_record(g, self.lst_shape, window, hr, overlap, cover_edges)
        self._capture(model, lay, self.lst_shape, stats, batch, conserve, rconserve.conserve, gaps, fill_value, dev)

    def __call__(self, lst_g, ndvi_g, mask=None, return_info=False):
        return self._replay(lst_g, ndvi_g, mask, return_info)
