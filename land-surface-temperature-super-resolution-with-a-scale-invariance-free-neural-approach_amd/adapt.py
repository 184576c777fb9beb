"""Fine-tuning a trained model on the granule it is about to predict (include/sifsr_adapt.h, csrc/adapt.hip).

The scale-invariance-free loss needs no high-resolution target: it is computed from the observed 1 km LST and the 250 m NDVI alone.
So a trained ``ModelB_2`` can take a few optimisation steps on the tiles of one granule, with the loss it was trained with, before
it predicts that granule.  A few dozen partly cloudy tiles are no basis for new BatchNorm statistics, so the steps run with FROZEN
statistics: ``model.bn_frozen = True`` makes ``train()`` mode normalise by the running statistics in the forward and the backward
and leave the buffers alone -- ``model.eval()`` afterwards predicts with exactly the network that was optimised.

    frozen_bn        context manager: bn_frozen + train() inside, both restored after
    input_gradient   dL/dx for an upstream gradient (sensitivity maps dSR/dNDVI, dSR/dLST), frozen statistics
    tile_targets     normalised LR targets, validity tiles and the valid count of a batch of active tiles, on the device
    adapt_granule    fill -> select -> ONE read of the active count -> network inputs once -> `steps` masked training steps (``_adapt``)

CPU-only use raises SifsrError: there is no fallback.
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib, gaps, pipeline, train
from .optim import FlatAdam


@contextlib.contextmanager
def frozen_bn(model):
    """``model.bn_frozen = True`` and ``model.train()`` inside the block; the attribute and the mode are put back after."""
    was_frozen, was_training = bool(getattr(model, "bn_frozen", False)), model.training
    model.bn_frozen = True
    model.train()
    try:
        yield model
    finally:
        model.bn_frozen = was_frozen
        model.train(was_training)


@torch.no_grad()
def input_gradient(model, x, dsr=None):
    """x (B,2,H,W) -> dL/dx (B,2,H,W) for the upstream gradient ``dsr`` (B,1,H,W) = dL/dsr (default: ones, the gradient of
    sr.sum()), through the network with its running statistics.  Two C-ABI calls on buffers of their own: parameters, ``.grad``,
    ``flat_grad()``, the BatchNorm buffers and the module's mode are untouched."""
    _lib.require_gpu(x, "input_gradient x")
    if x.dim() != 4 or x.shape[1] != 2:
        raise _lib.SifsrError(f"input_gradient expects (B,2,H,W) = cat(lst_up, ndvi); got {tuple(x.shape)}")
    if getattr(model, "compute_dtype", "fp32") != "fp32":
        raise _lib.SifsrError("the input gradient is fp32 only; set compute_dtype='fp32'")
    B, _, H, W = x.shape
    flat_p, flat_r, _ = model._flat_state(x.device)
    ws_bytes = _lib.call("sifsra_model_workspace_bytes", B, H, W)
    if ws_bytes == 0:
        raise _lib.SifsrError(f"unsupported shape {tuple(x.shape)}")
    if dsr is None:
        dsr = torch.ones((B, 1, H, W), dtype=torch.float32, device=x.device)
    _lib.require_gpu(dsr, "input_gradient dsr")
    if tuple(dsr.shape) != (B, 1, H, W) or dsr.device != x.device:
        raise _lib.SifsrError(f"dsr must be {(B, 1, H, W)} on {x.device}, got {tuple(dsr.shape)} on {dsr.device}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    sr = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    grads = torch.empty_like(flat_p)
    dx = torch.empty_like(x)
    stream = _lib.stream_ptr(x.device)
    _lib.call("sifsra_model_forward", x, sr, flat_p, flat_r, ws, ws_bytes, B, H, W, model._bn_hyper[1], stream)
    _lib.call("sifsra_model_backward", x, dsr, flat_p, grads, dx, ws, ws_bytes, B, H, W, 1, stream)
    return dx


def tile_targets(filled, valid, active, n_active, first, count, stats, window=64, overlap=0, cover_edges=False):
    """-> (lst (count,1,window,window) float32, valid (count,1,window,window) uint8, n_valid one int64), all on the device: the
    loss targets of tiles ``active[(first + i) % n_active]``, i < count, of the layout ``gaps.select_tiles`` used.  ``lst`` is
    the normalised filled tile -- the value ``gaps.prepare_active_tiles`` upsamples, bit for bit.  Nothing is read back."""
    _lib.require_gpu(filled, "filled granule")
    if filled.dim() != 2:
        raise _lib.SifsrError(f"filled granule: expected a 2-D raster, got {tuple(filled.shape)}")
    ty, tx = pipeline._mosaic_tiles(filled.shape, None, window, overlap, cover_edges)
    valid = gaps._valid_raster(valid, filled.shape, filled.device)
    if active.dtype != torch.int32 or tuple(active.shape) != (ty * tx,) or n_active.dtype != torch.int32 or n_active.numel() != 1:
        raise _lib.SifsrError(f"active must be int32 {(ty * tx,)} and n_active one int32, as select_tiles returns them")
    if int(first) < 0 or int(count) < 1:
        raise _lib.SifsrError(f"first must be >= 0 and count positive, got {first}, {count}")
    h, w = filled.shape
    dev = filled.device
    lst = torch.empty((int(count), 1, window, window), dtype=torch.float32, device=dev)
    vt = torch.empty((int(count), 1, window, window), dtype=torch.uint8, device=dev)
    n_valid = torch.empty((), dtype=torch.int64, device=dev)
    _lib.call("sifsra_tile_targets", filled, valid, active, n_active, int(first), int(count), h, w, window, overlap,
              1 if cover_edges else 0, float(stats["mean_lst"]), float(stats["std_lst"]), lst, vt, n_valid, _lib.stream_ptr(dev))
    return lst, vt, n_valid


class Adaptation:
    """What ``adapt_granule`` returns: ``losses`` (steps,3) device tensor of (ds, pl, loss) per step, ``n_active``, the
    ``optimizer`` that took the steps, and ``restore()``."""

    def __init__(self, model, start, losses, n_active, optimizer):
        self._model, self._start = model, start
        self.losses, self.n_active, self.optimizer = losses, n_active, optimizer

    @torch.no_grad()
    def restore(self):
        """Put back the parameters the model had when ``adapt_granule`` was called, bit for bit."""
        if self._start is not None:
            self._model.flat_parameters().copy_(self._start)


def adapt_granule(model, lst_g, ndvi_g, stats, mask=None, steps=20, lr=1e-5, alpha=0.5, gamma=1.0, kind="sr2", batch=16,
                  window=64, overlap=0, cover_edges=False, optimizer=None, graphed=False):
    """``steps`` optimisation steps of the masked SIF loss on the active tiles of one gappy granule (raw LST (h,w) [K], raw NDVI
    (4h,4w), ``mask`` as in ``gaps.fill_gaps``), BatchNorm statistics frozen.  Step i is ``train.train_step(..., valid=, n_valid=)``
    on the min(batch, n_active) tiles from position i * batch of the active list, cyclic, with ``tile_targets``' outputs; the
    optimizer is ``FlatAdam(lr=lr)`` unless one is given.  The read of the active count is the only host synchronisation; no active
    tile: no step, no forward.  Returns an ``Adaptation``; the model's mode and ``bn_frozen`` are as they were.

    ``graphed`` (default False: the loop above, bit for bit): after the read of the active count the step is a
    ``train.GraphedTrainStep(masked=True)`` for min(batch, n_active) tiles -- three eager steps, the fourth captures, the rest
    replay --; the optimizer is then ``FlatAdam(lr=lr, capturable=True)`` unless one is given, which must be capturable
    (ValueError before any launch)."""
    _lib.require_gpu(lst_g, "lst granule"); _lib.require_gpu(ndvi_g, "ndvi granule")
    if lst_g.dim() != 2:
        raise _lib.SifsrError(f"lst granule: expected a 2-D raster, got {tuple(lst_g.shape)}")
    lay = gaps._tile_layout(lst_g.shape, ndvi_g.shape, window, overlap, cover_edges)           # (raises before any launch)
    if int(batch) < 1 or int(steps) < 0:
        raise _lib.SifsrError(f"batch must be positive and steps non-negative, got {batch}, {steps}")

    def step(model, optimizer, lst, xb, vt, n_valid):
        return train.train_step(model, optimizer, lst, xb[:, 0:1], xb[:, 1:2], stats, alpha, gamma, kind, valid=vt, n_valid=n_valid)

    def captured(model, optimizer, b):
        g = train.GraphedTrainStep(model, optimizer, b, stats, alpha, gamma, kind, hr=lay.hr, masked=True)
        return lambda model, optimizer, lst, xb, vt, n_valid: g(lst, xb[:, 0:1], xb[:, 1:2], vt, n_valid)

    return _adapt(model, lay, step, lst_g, ndvi_g, stats, mask, int(steps), int(batch), lr, optimizer, captured if graphed else None)


def _adapt(model, lay, step, lst_g, ndvi_g, stats, mask, steps, batch, lr, optimizer, captured=None):
    """The loop of ``adapt_granule`` here and in ``rloss`` on the ``_granule.Layout`` ``lay``: fill -> select -> one read of the active
    count -> the inputs of the active tiles once -> ``steps`` x ``step(model, optimizer, lst, xb, vt, n_valid)`` -> (ds, pl, loss).
    ``captured(model, optimizer, b)``: builds the step of the graphed loop, a ``GraphedTrainStep`` for b tiles behind the same call;
    ``tile_targets`` and the gather of ``xb`` stay outside its graph (their ``first`` changes per step) and feed its static buffers."""
    if captured is not None and optimizer is not None and not getattr(optimizer, "capturable", False):
        raise ValueError("adapt_granule(graphed=True) needs FlatAdam(..., capturable=True), or no optimizer")
    filled, valid = gaps.fill_gaps(lst_g, mask)
    _, active, n_active = gaps.select_tiles(valid, lay.window, lay.overlap, lay.cover_edges)
    n = int(n_active.item())                                            # the one host sync
    losses = torch.zeros((steps, 3), dtype=torch.float32, device=lst_g.device)
    if n == 0 or steps == 0:
        return Adaptation(model, None, losses[:0] if n == 0 else losses, n, optimizer)
    start = model.flat_parameters().detach().clone()
    x = lay.prepare_active(filled, ndvi_g, stats, active, n_active, n)
    if optimizer is None:
        optimizer = FlatAdam(model.parameters(), lr=lr, capturable=captured is not None)
    b = min(batch, n)
    with frozen_bn(model):
        if captured is not None:
            step = captured(model, optimizer, b)
        for i in range(steps):
            first = (i * batch) % n
            idx = (torch.arange(first, first + b, device=x.device) % n) if first + b > n else slice(first, first + b)
            xb = x[idx]
            lst, vt, n_valid = tile_targets(filled, valid, active, n_active, first, b, stats, lay.window, lay.overlap, lay.cover_edges)
            ds, pl, loss = step(model, optimizer, lst, xb, vt, n_valid)
            losses[i, 0] = ds.detach(); losses[i, 1] = pl.detach(); losses[i, 2] = loss.detach()
    return Adaptation(model, start, losses, n, optimizer)
