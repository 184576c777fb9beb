"""The whole-granule drivers, once, for the x4 kernels and the kernels at any ratio.

A ``Layout`` describes one tile layout and carries the four launches that depend on the kernel family; it is built once per call,
before any launch, by ``gaps._tile_layout`` (x4: ``pipeline`` / ``gaps``) or ``ratio._tile_layout`` (``ratio``), which raise for a
raster the layout does not fit.  The drivers only enqueue on the current stream: ``predict`` can be captured into a graph,
``predict_gaps`` holds the one host synchronisation of the prediction path, the read of the active count."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib

# prepare(lst_g, ndvi_g, stats, out=None) -> x            prepare_active(filled, ndvi_g, stats, active, n_active, cap) -> x
# blend(sr, stats, out=None) -> raster                    blend_active(sr, slot, valid, stats, fill_value) -> raster
Layout = namedtuple("Layout", "window hr overlap cover_edges tiles hr_shape prepare prepare_active blend blend_active")


def forwards(model, x, batch, sr=None):
    """x (N,2,hr,hr) -> sr (N,1,hr,hr): ceil(N / batch) forwards, the last one short; ``sr``: the buffer to write"""
    if sr is None:
        sr = torch.empty((x.shape[0], 1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    for i in range(0, x.shape[0], batch):
        sr[i:i + batch] = model(x[i:i + batch])
    return sr


def predict(model, lay, lst_g, ndvi_g, stats, batch, x=None, sr=None, out=None, conserve=0):
    """prepare -> batched forwards -> blend.  x / sr / out: static buffers of a captured run (x and sr hold a whole number of
    batches: the tiles past the last real one are zeros and their predictions are never read); None: allocated here and the last
    batch is as short as it is.  conserve (x4 only; at a ratio the option is ``rconserve.granule_option``, around the call): that
    many ``conserve.conserve`` steps on the blended raster, in place (its scratch is allocated here, in a captured run from the
    graph's own pool)."""
    if int(conserve) < 0:
        raise _lib.SifsrError(f"conserve must be a step count >= 0, got {conserve}")
    tiles = lay.prepare(lst_g, ndvi_g, stats, out=x)
    sr = forwards(model, tiles if x is None else x, batch, sr)
    out = lay.blend(sr[:tiles.shape[0]], stats, out=out)
    if int(conserve) > 0:
        from .conserve import conserve as correct
        correct(out, lst_g, None, n_iter=int(conserve), out=out)
    return out


def predict_gaps(model, lay, lst_g, ndvi_g, stats, mask, batch, fill_value, return_info):
    """fill -> select -> the read of the active count -> inputs of the active tiles -> forwards -> masked blend, or the
    all-``fill_value`` raster and no forward when nothing is valid"""
    from . import gaps
    filled, valid = gaps.fill_gaps(lst_g, mask)
    slot, active, n_active = gaps.select_tiles(valid, lay.window, lay.overlap, lay.cover_edges)
    n = int(n_active.item())                                            # the one host sync
    if n == 0:
        out = torch.full(lay.hr_shape, float(fill_value), dtype=torch.float32, device=lst_g.device)
    else:
        x = lay.prepare_active(filled, ndvi_g, stats, active, n_active, n)
        out = lay.blend_active(forwards(model, x, batch), slot, valid, stats, fill_value)
    if return_info:
        return out, {"valid": valid.bool(), "n_active": n, "n_tiles": lay.tiles[0] * lay.tiles[1]}
    return out
