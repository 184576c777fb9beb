"""Gap-aware whole-granule prediction (include/sifsr_gaps.h, csrc/gaps.hip).

Every real MOD11A1 / MOD21A1D granule has holes: cloud, ocean and fill pixels arrive as raw 0 = 0.0 K (what ``products.decode``
hands over; process_modis.py:96,180 and predict.py:92 treat them as bad).  ``predict.predict_granule`` feeds them to the z-score
and the bicubic x4 as they are -- about -55 sigma each, which spoils valid land around every gap --, spends a forward on tiles
that are all cloud or sea, and returns no mask.  Here, on the device:

    fill_gaps             valid = finite, non-zero and kept by ``mask``; invalid pixels get the mean of the valid pixels of the
                          smallest aligned dyadic block around them that holds one (a push-pull pyramid, bit-defined)
    select_tiles          the tiles of the layout of ``pipeline.tile_origins`` that hold a valid pixel, in order
    predict_granule_gaps  ``_granule.predict_gaps`` on the x4 layout record of ``_tile_layout`` (``ratio`` runs it on its own): fill -> select
                          -> ONE read of the active count -> network input of the active tiles only -> ceil(n_active / batch)
                          forwards -> blend as ``predict_granule`` does, ``fill_value`` where invalid

A valid pixel is blended from exactly the tiles the ungapped path uses (every tile covering a valid pixel is active), so at
valid pixels ``predict_granule_gaps(gappy)`` equals ``predict_granule(filled)`` bit for bit, and a gap-free raster gives
``predict_granule``'s raster.  CPU-only use raises SifsrError: there is no fallback.
"""
from __future__ import annotations

import torch

from . import _granule, _lib, pipeline
from .conserve import granule_option


def _valid_raster(valid, shape, device, what="valid"):
    """-> a uint8 view of a (h, w) uint8 / bool device raster (one byte per pixel, non-zero = keep)"""
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.uint8, torch.bool):
        raise _lib.SifsrError(f"{what} must be a uint8 or bool tensor, got {getattr(valid, 'dtype', type(valid).__name__)}")
    if not valid.is_cuda or (device is not None and valid.device != device):
        raise _lib.SifsrError(f"{what} is on {valid.device}, the raster on {device or 'a ROCm GPU'}")
    if tuple(valid.shape) != tuple(shape):
        raise _lib.SifsrError(f"{what} must be {tuple(shape)}, got {tuple(valid.shape)}")
    return valid.contiguous().view(torch.uint8)


def fill_gaps(lst_g, mask=None):
    """lst_g (h,w) [K], mask (h,w) uint8 / bool or None (non-zero = keep) -> (filled (h,w) float32, valid (h,w) uint8 of 0 / 1).
    valid: finite, not 0 K and kept by the mask; filled: lst_g where valid, elsewhere the mean of the valid pixels of the smallest
    aligned dyadic block around the pixel that holds one (0 everywhere when nothing is valid)."""
    _lib.require_gpu(lst_g, "lst granule")
    if lst_g.dim() != 2 or lst_g.numel() == 0:
        raise _lib.SifsrError(f"lst granule: expected a non-empty 2-D raster, got {tuple(lst_g.shape)}")
    h, w = lst_g.shape
    if mask is not None:
        mask = _valid_raster(mask, (h, w), lst_g.device, "mask")
    need = _lib.call("sifsrg_fill_workspace_bytes", h, w)
    if need == 0:
        raise _lib.SifsrError(f"lst granule {(h, w)} is larger than 16384 x 16384")
    ws = torch.empty((need,), dtype=torch.uint8, device=lst_g.device)
    filled = torch.empty_like(lst_g)
    valid = torch.empty((h, w), dtype=torch.uint8, device=lst_g.device)
    _lib.call("sifsrg_fill", lst_g, mask, filled, valid, ws, need, h, w, _lib.stream_ptr(lst_g.device))
    return filled, valid


def select_tiles(valid, window=64, overlap=0, cover_edges=False):
    """valid (h,w) uint8 / bool -> (slot (T,), active (T,), n_active (1,)) int32 device tensors: the tiles with at least one valid
    pixel in increasing order in active[:n], slot[t] = the position of tile t in it or -1.  Nothing is read back."""
    if not isinstance(valid, torch.Tensor) or valid.dim() != 2:
        raise _lib.SifsrError("valid must be a 2-D tensor")
    ty, tx = pipeline._mosaic_tiles(valid.shape, None, window, overlap, cover_edges)
    valid = _valid_raster(valid, valid.shape, valid.device)
    h, w = valid.shape
    slot = torch.empty((ty * tx,), dtype=torch.int32, device=valid.device)
    active = torch.empty((ty * tx,), dtype=torch.int32, device=valid.device)
    n_active = torch.empty((1,), dtype=torch.int32, device=valid.device)
    _lib.call("sifsrg_tiles_select", valid, slot, active, n_active, h, w, window, overlap, 1 if cover_edges else 0,
              _lib.stream_ptr(valid.device))
    return slot, active, n_active


def prepare_active_tiles(filled, ndvi_g, stats, active, n_active, cap, window=64, overlap=0, cover_edges=False, clip_ndvi=True, out=None):
    """-> x (cap,2,4win,4win): x[i] = the network input of tile active[i] for i < min(n_active, cap), the rest untouched
    (``sifsrg_tiles_prepare``); bit-identical to that tile of ``pipeline.granule_to_tiles(filled, ...)``.  ``out``: a buffer of at
    least ``cap`` tiles to write into (a captured run's static one); its first ``cap`` tiles are returned."""
    _lib.require_gpu(filled, "filled granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    pipeline._mosaic_tiles(filled.shape, ndvi_g.shape, window, overlap, cover_edges)
    if int(cap) < 1:
        raise _lib.SifsrError(f"cap must be positive, got {cap}")
    h, w = filled.shape
    x = pipeline._tile_buffer(out, int(cap), 2, 4 * window, filled.device, "tile buffer")
    _lib.call("sifsrg_tiles_prepare", filled, ndvi_g, x, active, n_active, int(cap), h, w, window, overlap, 1 if cover_edges else 0,
              *pipeline._stats4(stats), 1 if clip_ndvi else 0, _lib.stream_ptr(filled.device))
    return x


def blend_active_tiles(sr, slot, valid, window, stats, overlap=0, cover_edges=False, fill_value=float("nan")):
    """sr (>= n_active,1,4win,4win) normalised predictions in the order of ``active`` -> the de-normalised raster (4h,4w) [K]:
    ``pipeline.blend_tiles`` at valid pixels, ``fill_value`` at invalid ones (``sifsrg_tiles_blend``)."""
    _lib.require_gpu(sr, "sr")
    ty, tx = pipeline._mosaic_tiles(valid.shape, None, window, overlap, cover_edges)
    valid = _valid_raster(valid, valid.shape, sr.device)
    if sr.dim() != 4 or sr.shape[0] < 1 or tuple(sr.shape[1:]) != (1, 4 * window, 4 * window):
        raise _lib.SifsrError(f"sr must be (n_active, 1, {4 * window}, {4 * window}), got {tuple(sr.shape)}")
    if slot.dtype != torch.int32 or tuple(slot.shape) != (ty * tx,):
        raise _lib.SifsrError(f"slot must be int32 {(ty * tx,)}, got {slot.dtype} {tuple(slot.shape)}")
    h, w = valid.shape
    out = torch.empty((4 * h, 4 * w), dtype=torch.float32, device=sr.device)
    _lib.call("sifsrg_tiles_blend", sr, slot, valid, out, h, w, window, overlap, 1 if cover_edges else 0, float(stats["mean_lst"]),
              float(stats["std_lst"]), float(fill_value), _lib.stream_ptr(sr.device))
    return out


def _tile_layout(lst_shape, ndvi_shape, window, overlap, cover_edges, plain=False):
    """-> the x4 ``_granule.Layout`` of an LST raster, or SifsrError; ``plain``: ``predict_granule``'s rule for its default layout"""
    tiles = (pipeline._granule_tiles if plain else pipeline._mosaic_tiles)(lst_shape, ndvi_shape, window, overlap, cover_edges)
    (h, w), lay = (int(v) for v in lst_shape), (overlap, cover_edges)
    return _granule.Layout(
        window, 4 * window, overlap, cover_edges, tiles, (4 * h, 4 * w),
        lambda lst_g, ndvi_g, stats, out=None: pipeline.granule_to_tiles(lst_g, ndvi_g, stats, window, True, *lay, out)[0],
        lambda filled, ndvi_g, stats, active, n_active, cap, out=None: prepare_active_tiles(filled, ndvi_g, stats, active, n_active, cap, window,
                                                                                          *lay, out=out),
        lambda sr, stats, out=None: pipeline.blend_tiles(sr, (h, w), window, stats, *lay, out),
        lambda sr, slot, valid, stats, fill_value: blend_active_tiles(sr, slot, valid, window, stats, *lay, fill_value))


@granule_option
@torch.inference_mode()
def predict_granule_gaps(model, lst_g, ndvi_g, stats, mask=None, window=64, batch=256, overlap=16, cover_edges=True,
                         fill_value=float("nan"), return_info=False):
    """``predict.predict_granule`` for a granule with holes: raw LST raster (h,w) [K] with cloud / ocean / fill pixels as 0 K,
    NaN or inf (and whatever ``mask`` -- (h,w) uint8 / bool, non-zero = keep -- rules out) + raw NDVI raster (4h,4w) -> the
    super-resolved raster (4h,4w) [K], ``fill_value`` wherever the LST pixel is invalid.

    The gaps are filled before the network sees the raster, tiles without a valid pixel cost no forward (the forwards run over
    the active tiles only, in batches of ``batch``, the last one short), and the read of the active count is the call's only
    host synchronisation.  At valid pixels the result is bit-identical to ``predict_granule`` on the filled raster with the same
    layout; nothing is valid: the all-``fill_value`` raster, no forward.

    Keyword-only ``conserve=k`` (``conserve.granule_option``): k residual-correction steps on the blended raster
    (``conserve.conserve`` with the same ``mask``: only cells whose LST pixel is valid move, and the correction fades out towards
    a gap); 0, the default, runs none.

    ``return_info``: also {"valid": bool (h,w) device tensor, "n_active": int, "n_tiles": int} and, with ``conserve`` > 0,
    "conserve_stats": the float64 device tensor (conserve+1, 4) of (count, bias, RMSE, max |r|) before the first step and after
    every step."""
    _lib.require_gpu(lst_g, "lst granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    if lst_g.dim() != 2:
        raise _lib.SifsrError(f"lst granule: expected a 2-D raster, got {tuple(lst_g.shape)}")
    lay = _tile_layout(lst_g.shape, ndvi_g.shape, window, overlap, cover_edges)                          # (raises before any launch)
    if int(batch) < 1:
        raise _lib.SifsrError(f"batch must be positive, got {batch}")
    model.eval()
    return _granule.predict_gaps(model, lay, lst_g, ndvi_g, stats, mask, batch, fill_value, return_info)
