"""Inference call pattern of the reference's predict.py:84-103, batched.

The reference runs one eval-mode forward per 64x64 LST tile (batch 1) and de-normalises with
``* std + mean``; tiles are independent and do not overlap, so here they are stacked and pushed
through the network in large batches (config 4 of BASELINE.json: batch 256).  ``predict_granule`` can also lay the
tiles with an overlap and a last tile flush to each edge and blend them (a seamless, complete raster; not in the reference); it and
``GranulePredictor`` run ``_granule.predict``, shared with ``ratio.predict_granule``, on the x4 layout.  HDF/GeoTIFF I/O is out of
scope; inputs are the already normalised ``lst_up`` / ``ndvi`` tiles.  ``predict_granule_gaps`` (sifsr/gaps.py) is
``predict_granule`` for granules with cloud / ocean / fill pixels: gaps filled, all-gap tiles skipped, the output masked.
``conserve=k`` on the granule calls adds k residual-correction steps after the blend (sifsr/conserve.py): the
output, seen through the sensor's MTF and decimated by 4, then returns the LST raster it was predicted from; 0, the default,
leaves every bit as it was.
"""
from __future__ import annotations

import torch

from . import _granule, _lib
from .conserve import granule_option
from .gaps import _tile_layout, fill_gaps, predict_granule_gaps, select_tiles  # noqa: F401  (the gap-aware path)


@torch.inference_mode()
def predict_tiles(model, lst_up, ndvi, stats, batch=256):
    """(N,1,256,256) x2 -> (N,1,256,256) de-normalised LST [K]  (predict.py:100-101)."""
    model.eval()
    out = torch.empty_like(lst_up)
    for i in range(0, lst_up.shape[0], batch):
        x = torch.cat((lst_up[i:i + batch], ndvi[i:i + batch]), dim=1)
        out[i:i + batch] = model(x) * stats["std_lst"] + stats["mean_lst"]
    return out


@granule_option
@torch.inference_mode()
def predict_granule(model, lst_g, ndvi_g, stats, window=64, batch=256, overlap=0, cover_edges=False):
    """The whole block loop of predict.py:84-103 on the device: raw LST raster (h,w) [K] + raw NDVI raster
    (4h,4w) -> super-resolved LST raster (4h,4w) [K].  Tiles are cut, normalised, bicubic-upsampled and
    concatenated by one kernel, pushed through the network in batches, de-normalised and pasted by another;
    pixels of ragged edge tiles stay 0, as in the reference (``LST_SR = np.zeros(...)``).

    ``overlap`` (LST pixels, 0..window/2) lays the tiles at stride ``window - overlap`` and merges their predictions with a
    normalised feathered blend, which removes the seams between independently predicted tiles; ``cover_edges`` adds a last
    tile flush to the bottom / right edge so that no pixel stays 0.  Both default to the reference's behaviour.

    Keyword-only ``conserve=k`` (``conserve.granule_option``): k steps of ``conserve.conserve`` on the blended raster (cells of
    0 K / non-finite LST pixels and the pixels no tile reached keep their bits); 0, the default: none."""
    model.eval()
    _lib.require_gpu(lst_g, "lst granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    lay = _tile_layout(lst_g.shape, ndvi_g.shape, window, overlap, cover_edges, plain=True)             # (raises before any launch)
    return _granule.predict(model, lay, lst_g, ndvi_g, stats, batch)


def tile_granule(lst_norm, ndvi_norm, window=64):
    """Cut a normalised LST raster (h,w) and its 4x NDVI raster into the non-overlapping tiles of
    predict.py:84-95 (ragged edge tiles are skipped, as in the reference).  Returns
    (lst_tiles (N,1,64,64), ndvi_tiles (N,1,256,256), [(i,j)...])."""
    h, w = lst_norm.shape
    lst_t, ndvi_t, pos = [], [], []
    for i in range(0, h - window + 1, window):
        for j in range(0, w - window + 1, window):
            lst_t.append(lst_norm[i:i + window, j:j + window])
            ndvi_t.append(ndvi_norm[4 * i:4 * (i + window), 4 * j:4 * (j + window)])
            pos.append((i, j))
    return torch.stack(lst_t)[:, None], torch.stack(ndvi_t)[:, None], pos


class GraphedPredictor:
    """BASELINE.json config 4: eval-mode forward of a fixed batch shape captured once into a HIP graph
    (``torch.cuda.CUDAGraph`` == hipGraph on ROCm) and replayed per batch of tiles.

    The whole forward is one C-ABI call that only enqueues kernels on the current stream (no allocation,
    no host sync inside the library), so stream capture records the ~60 launches as graph nodes; replay
    removes the per-launch host cost, which matters at small batch (predict.py runs batch 1 per tile).
    The de-normalisation ``* std + mean`` (predict.py:101) is part of the captured region.
    """

    def __init__(self, model, batch, stats, hr=256, device=None):
        self.model = model.eval()
        dev = device or next(model.parameters()).device
        self.batch, self.stats = int(batch), stats
        self.x = torch.zeros((self.batch, 2, hr, hr), dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.inference_mode():
            for _ in range(2):                      # warm-up: flat-buffer setup, allocator pools
                self.out = self.model(self.x) * stats["std_lst"] + stats["mean_lst"]
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.inference_mode(), torch.cuda.graph(self.graph):
            self.out = self.model(self.x) * stats["std_lst"] + stats["mean_lst"]

    @torch.inference_mode()
    def __call__(self, lst_up, ndvi):
        n = lst_up.shape[0]
        if n > self.batch:
            raise ValueError(f"batch {n} exceeds the captured batch {self.batch}")
        self.x[:n, 0:1].copy_(lst_up)
        self.x[:n, 1:2].copy_(ndvi)
        self.graph.replay()
        return self.out[:n].clone()


def _captured_granule(self, model, lst_shape, stats, window, overlap, cover_edges, batch, device, conserve, gaps=False,
                      fill_value=float("nan")):
    """``GranulePredictor.__init__``: the checks (before any launch), then ``_granule.CapturedGranule._capture``"""
    h, w = (int(v) for v in lst_shape)
    self.lst_shape, self.window = (h, w), int(window)
    self.overlap, self.cover_edges = int(overlap), bool(cover_edges)
    if int(conserve) < 0:
        raise _lib.SifsrError(f"conserve must be a step count >= 0, got {conserve}")
    lay = _tile_layout((h, w), (4 * h, 4 * w), self.window, self.overlap, self.cover_edges, plain=not gaps)
    if int(batch) < 1:
        raise _lib.SifsrError(f"batch must be positive, got {batch}")
    self._capture(model, lay, (h, w), stats, batch, conserve, None, gaps, fill_value, device or next(model.parameters()).device)


class GranulePredictor(_granule.CapturedGranule):
    """``predict_granule`` for ONE granule shape captured into a HIP graph: prepare -> batched eval forwards -> blend, on one
    stream, replayed per granule.  All buffers are static; the tiles are padded with zero tiles to a whole number of batches
    (every forward has the captured batch shape; the padding's predictions are not read).  ``__call__(lst_g, ndvi_g)`` copies
    the rasters in, replays and returns a clone of the output raster -- bit-identical to the eager ``predict_granule`` with the
    same arguments; ``conserve`` steps are part of the captured chain.

    Keyword-only ``gaps=True`` (and ``fill_value``; ``_granule.keyword_options``): the captured form of
    ``predict_granule_gaps`` with the same arguments -- a graph can have a fixed slot count and a device-side active count: every
    slot is forwarded, only the active ones are read (``_granule.predict_gaps_fixed``), and no call reads the count back.
    ``__call__(lst_g, ndvi_g, mask=None, return_info=False)`` then returns the bits of the eager call, ``fill_value`` pixels
    included; ``info["n_active"]`` is a (1,) int32 device tensor.  The defaults keep the object and the bits above."""

    # the constructor's body is ``_captured_granule`` above: ``__init__`` only states the pinned positional signature, and the
    # decorator adds ``gaps=`` / ``fill_value=`` around it (fold them into the signature once the pin in the host test may move)
    @_granule.keyword_options(_captured_granule, gaps=False, fill_value=float("nan"))
    def __init__(self, model, lst_shape, stats, window=64, overlap=0, cover_edges=False, batch=256, device=None, conserve=0):
        """the positional signature (tests/test_conserve_host.py pins its end); ``_captured_granule`` is the body"""

    def __call__(self, lst_g, ndvi_g, mask=None, return_info=False):
        return self._replay(lst_g, ndvi_g, mask, return_info)
