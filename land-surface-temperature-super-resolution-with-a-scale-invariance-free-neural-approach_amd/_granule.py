"""The whole-granule drivers, once, for the x4 kernels and the kernels at any ratio.

A ``Layout`` describes one tile layout and carries the four launches that depend on the kernel family; it is built once per call,
before any launch, by ``gaps._tile_layout`` (x4: ``pipeline`` / ``gaps``) or ``ratio._tile_layout`` (``ratio``), which raise for a
raster the layout does not fit.  The drivers only enqueue on the current stream: ``predict`` can be captured into a graph,
``predict_gaps`` holds the one host synchronisation of the prediction path, the read of the active count, and ``predict_gaps_fixed``
 is ``predict_gaps`` without it: every slot of a static tile buffer is forwarded and only the active ones are read,
so it can be captured too.  ``keyword_options`` is the decorator the captured options of f23 are added with."""
from __future__ import annotations

import functools
import inspect
from collections import namedtuple

import torch

from . import _lib

# prepare(lst_g, ndvi_g, stats, out=None) -> x            prepare_active(filled, ndvi_g, stats, active, n_active, cap, out=None) -> x
# blend(sr, stats, out=None) -> raster                    blend_active(sr, slot, valid, stats, fill_value) -> raster
Layout = namedtuple("Layout", "window hr overlap cover_edges tiles hr_shape prepare prepare_active blend blend_active")


def forwards(model, x, batch, sr=None):
    """x (N,2,hr,hr) -> sr (N,1,hr,hr): ceil(N / batch) forwards, the last one short; ``sr``: the buffer to write"""
    if sr is None:
        sr = torch.empty((x.shape[0], 1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    for i in range(0, x.shape[0], batch):
        sr[i:i + batch] = model(x[i:i + batch])
    return sr


def keyword_options(impl, **defaults):
    """Decorator that gives a public call keyword-only options without touching its parameter list, as ``conserve.granule_option``
    does for ``conserve=k``: the decorated function states the positional signature and the docstring (the host tests pin the
    first; ``inspect.signature`` follows ``__wrapped__`` to it) and ``impl`` -- the same parameters, then the options -- does the
    work.  ``inspect.signature(f, follow_wrapped=False)`` shows the wrapper."""
    def decorate(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*args, **kw):
            options = {k: kw.pop(k, v) for k, v in defaults.items()}
            a = sig.bind(*args, **kw)
            a.apply_defaults()
            return impl(*a.args, **a.kwargs, **options)
        return call
    return decorate


def predict(model, lay, lst_g, ndvi_g, stats, batch, x=None, sr=None, out=None, conserve=0, correct=None):
    """prepare -> batched forwards -> blend.  x / sr / out: static buffers of a captured run (x and sr hold a whole number of
    batches: the tiles past the last real one are zeros and their predictions are never read); None: allocated here and the last
    batch is as short as it is.  conserve (x4 only; at a ratio the option is ``rconserve.granule_option``, around the call): that
    many ``conserve.conserve`` steps on the blended raster, in place (its scratch is allocated here, in a captured run from the
    graph's own pool); ``correct``: the step in its place (``rconserve.conserve`` for a captured run at a ratio)."""
    if int(conserve) < 0:
        raise _lib.SifsrError(f"conserve must be a step count >= 0, got {conserve}")
    tiles = lay.prepare(lst_g, ndvi_g, stats, out=x)
    sr = forwards(model, tiles if x is None else x, batch, sr)
    out = lay.blend(sr[:tiles.shape[0]], stats, out=out)
    if int(conserve) > 0:
        if correct is None:
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


def predict_gaps_fixed(model, lay, lst_g, ndvi_g, stats, mask, batch, fill_value, x, sr, conserve=0, correct=None):
    """``predict_gaps`` with no read of the active count, for a captured run: fill -> select -> the inputs of the active tiles into
    the first ``n_active`` slots of the static ``x`` (a whole number of batches >= the tile count, zero-initialised; the slots past
    ``n_active`` keep what an earlier run left, zeros or the finite inputs of an earlier tile) -> forwards over EVERY slot into the
    static ``sr`` (the eval forward is per image: a slot's prediction does not depend on its neighbours in the batch) -> masked
    blend, which reads slot[t] < n_active only and writes every pixel, so nothing of a stale slot reaches the raster and a raster
    without a valid pixel comes out all ``fill_value`` -> ``conserve`` steps of ``correct`` (default ``conserve.conserve``) with
    the mask.  -> (raster, valid (h,w) uint8, n_active (1,) int32), all on the device; nothing is read back."""
    from . import gaps
    if int(conserve) < 0:
        raise _lib.SifsrError(f"conserve must be a step count >= 0, got {conserve}")
    filled, valid = gaps.fill_gaps(lst_g, mask)
    slot, active, n_active = gaps.select_tiles(valid, lay.window, lay.overlap, lay.cover_edges)
    lay.prepare_active(filled, ndvi_g, stats, active, n_active, x.shape[0], out=x)
    forwards(model, x, batch, sr)
    out = lay.blend_active(sr, slot, valid, stats, fill_value)
    if int(conserve) > 0:
        if correct is None:
            from .conserve import conserve as correct
        correct(out, lst_g, mask, n_iter=int(conserve), out=out)
    return out, valid, n_active


class CapturedGranule:
    """The static buffers, the capture and the replay under ``predict.GranulePredictor`` and ``ratio.GranulePredictor``: ONE
    granule shape, one hipGraph.  ``_capture`` is called by their constructors after every check that needs no launch.

    ``gaps=False``: ``predict`` into the static ``out``.  ``gaps=True``: ``predict_gaps_fixed``; the graph has a fixed slot count
    (every forward has the captured batch shape) and a device-side active count, so one capture serves every mask.  The static
    ``mask`` holds all ones when a call passes none: the kernels read a mask as a predicate only, so that is ``mask=None`` bit for
    bit and one captured form is enough."""

    def _capture(self, model, lay, lst_shape, stats, batch, conserve, correct, gaps, fill_value, dev):
        self.model = model.eval()
        h, w = lst_shape
        self.layout, self.tiles, self.stats = lay, lay.tiles, stats
        self.conserve, self.gaps, self.fill_value, self._correct = int(conserve), bool(gaps), float(fill_value), correct
        n, hr = self.tiles[0] * self.tiles[1], lay.hr
        self.batch = min(int(batch), n)
        padded = -(-n // self.batch) * self.batch
        self.lst = torch.zeros((h, w), dtype=torch.float32, device=dev)
        self.ndvi = torch.zeros(lay.hr_shape, dtype=torch.float32, device=dev)
        self.x = torch.zeros((padded, 2, hr, hr), dtype=torch.float32, device=dev)
        self.sr = torch.zeros((padded, 1, hr, hr), dtype=torch.float32, device=dev)
        if self.gaps:
            self.mask = torch.ones((h, w), dtype=torch.uint8, device=dev)
            self.out = self.valid = self.n_active = None                  # (the capture run's outputs, in the graph's pool)
        else:
            self.out = torch.zeros(lay.hr_shape, dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.inference_mode():
            for _ in range(2):                      # warm-up: flat-buffer setup, allocator pools
                self._run()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.inference_mode(), torch.cuda.graph(self.graph):
            res = self._run()
        if self.gaps:
            self.out, self.valid, self.n_active = res

    def _run(self):
        if self.gaps:
            return predict_gaps_fixed(self.model, self.layout, self.lst, self.ndvi, self.stats, self.mask, self.batch, self.fill_value,
                                      self.x, self.sr, conserve=self.conserve, correct=self._correct)
        return predict(self.model, self.layout, self.lst, self.ndvi, self.stats, self.batch, x=self.x, sr=self.sr, out=self.out,
                       conserve=self.conserve, correct=self._correct)

    @torch.inference_mode()
    def _replay(self, lst_g, ndvi_g, mask=None, return_info=False):
        """copies the rasters (and the mask) in, replays, -> a clone of the raster; nothing is read back.  ``return_info`` (gaps
        only): also {"valid": bool (h,w), "n_active": (1,) int32 DEVICE tensor, "n_tiles": int}"""
        shape, hr_shape = tuple(self.lst.shape), tuple(self.ndvi.shape)
        if tuple(lst_g.shape) != shape or tuple(ndvi_g.shape) != hr_shape:
            raise ValueError(f"captured for an LST raster {shape} and an NDVI raster {hr_shape}; got "
                             f"{tuple(lst_g.shape)}, {tuple(ndvi_g.shape)}")
        if not self.gaps and (mask is not None or return_info):
            raise ValueError("mask and return_info go with gaps=True")
        if mask is not None:
            from .gaps import _valid_raster
            mask = _valid_raster(mask, shape, self.lst.device, "mask")
        self.lst.copy_(lst_g)
        self.ndvi.copy_(ndvi_g)
        if self.gaps:
            if mask is None:
                self.mask.fill_(1)
            else:
                self.mask.copy_(mask)
        self.graph.replay()
        out = self.out.clone()
        if return_info:
            return out, {"valid": self.valid.bool(), "n_active": self.n_active.clone(), "n_tiles": self.tiles[0] * self.tiles[1]}
        return out
