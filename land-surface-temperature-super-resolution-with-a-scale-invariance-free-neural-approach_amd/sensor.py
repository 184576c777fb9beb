"""The differentiable sensor model at any ratio (include/sifsr_sensor.h, csrc/degrade.hip): what training with the
scale-invariance-free loss needs when the ratio between the two sensors is not 4.

    downscale(x, factor, ...)   ``degrade.degrade`` with a backward: the reference's ``downscale_LST_SR_to_LR(factor=f)`` (utils.py:
                                1671-1706; ``crop=True``, the default here), ``generic_downscale`` and ``downscale_Aster_to_*`` as
                                autograd ops.  Forward: ``sifsrs_degrade``, the bits of ``degrade.degrade``; backward:
                                ``sifsrt_degrade_bwd``, the transpose of the same banded operator.
    lowpass(x, factor, mtf)     ``get_output_ftm(factor=f)`` (utils.py:1833-1860): the reflect-border Gaussian of the MTF at half
                                width hkw or ceil(factor), forward and adjoint (``sifsrt_lowpass_fwd`` / ``_bwd``).
    sif_loss / train_step       the loss block and the optimisation step (``train._optimise``) of the two training scripts on top of them.

Everything is fp32 on the device, accumulated in float64 and rounded once; CPU tensors raise SifsrError: there is no CPU path.

The loss here is composed from autograd ops and has no mask (``valid`` is an argument of ``downscale`` alone); the fused, masked
loss at a ratio, its training step and ``adapt_granule`` at a ratio are ``sifsr.rloss``; at x4
``sif_ops.sif_loss`` stays the fused path.  Out of scope: ``GraphedTrainStep`` at a ratio, the ``hkw`` argument in the loss, and the
drop-in's ``factor != 4`` calls, which keep their refusal."""
from __future__ import annotations

import torch

from . import _lib, degrade, train
from .sif_ops import huber_loss, sobel_bank


def lr_shape(H, W, factor, hkw=None):
    """-> (h, w) of the coarse raster the sensor sees of an (H, W) one: ``degrade.output_shape(H, W, factor, hkw, crop=True)``."""
    return degrade.output_shape(H, W, factor, hkw, crop=True)


def _images(x, what):
    if not isinstance(x, torch.Tensor):
        raise _lib.SifsrError(f"{what}: expected a tensor, got {type(x).__name__}")
    _lib.require_gpu(x, "x")
    if x.dim() not in (2, 3, 4):
        raise _lib.SifsrError(f"{what}: expected (H,W), (B,H,W) or (B,C,H,W), got {tuple(x.shape)}")
    B = 1
    for d in x.shape[:-2]:
        B *= d
    if B < 1:
        raise _lib.SifsrError(f"{what}: empty batch {tuple(x.shape)}")
    return B, x.shape[-2], x.shape[-1]


def _mtf(mtf):
    if not 0.0 < float(mtf) < 1.0:
        raise _lib.SifsrError(f"mtf must be in (0, 1), got {mtf}")
    return float(mtf)


class _Downscale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, factor, mtf, hkw, crop, valid, fill_value, return_valid):
        with_map = valid is not None
        got = degrade.degrade(x.detach(), factor, mtf=mtf, hkw=hkw, crop=crop, valid=valid, fill_value=fill_value,
                              return_valid=return_valid or with_map)
        out, ov = got if (return_valid or with_map) else (got, None)
        ctx.cfg = (float(factor), float(mtf), degrade._hkw(hkw), int(bool(crop)), tuple(x.shape))
        ctx.save_for_backward(*([ov] if with_map else []))   # without a map every output counts, the darkened ring included
        if not return_valid:
            return out
        ctx.mark_non_differentiable(ov)
        return out, ov

    @staticmethod
    def backward(ctx, g, *_):
        factor, mtf, hk, crop, shape = ctx.cfg
        ov = ctx.saved_tensors[0] if ctx.saved_tensors else None
        g = g.contiguous()
        _lib.require_gpu(g, "the gradient of downscale")
        B, H, W = g.numel() // (g.shape[-2] * g.shape[-1]), shape[-2], shape[-1]
        need = _lib.call("sifsrt_degrade_bwd_workspace_bytes", B, H, W, factor, hk, crop)
        ws = torch.empty((need,), dtype=torch.uint8, device=g.device)
        dx = torch.empty(shape, dtype=torch.float32, device=g.device)
        _lib.call("sifsrt_degrade_bwd", g, ov, dx, ws, need, B, H, W, factor, mtf, hk, crop, _lib.stream_ptr(g.device))
        return dx, None, None, None, None, None, None, None


def downscale(x, factor, mtf=0.1, hkw=None, crop=True, valid=None, fill_value=float("nan"), return_valid=False):
    """``degrade.degrade`` (same arguments, same bits) as an autograd op: x (H,W), (B,H,W) or (B,C,H,W) float32 on the device -> the
    raster seen at ``factor`` times the pixel size.  ``crop`` defaults to True: the cut of ``downscale_LST_SR_to_LR``.  The gradient
    with respect to ``x`` is the transpose of the banded operator; with ``valid``, outputs that hold ``fill_value`` pass no gradient
    (what the incoming gradient holds there, NaN included, is not used) and the gradient is exactly 0 at every invalid pixel.  No
    gradient flows to ``valid``."""
    if not isinstance(x, torch.Tensor):
        raise _lib.SifsrError(f"downscale: expected a tensor, got {type(x).__name__}")
    _mtf(mtf)
    return _Downscale.apply(x, factor, mtf, hkw, crop, valid, fill_value, return_valid)


class _Lowpass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, factor, mtf, hk):
        ctx.cfg = (factor, mtf, hk)
        return _lowpass_call("sifsrt_lowpass_fwd", x, factor, mtf, hk)

    @staticmethod
    def backward(ctx, g):
        return _lowpass_call("sifsrt_lowpass_bwd", g.contiguous(), *ctx.cfg), None, None, None


def _lowpass_call(name, x, factor, mtf, hk):
    B, H, W = _images(x, "lowpass")
    need = _lib.call("sifsrt_lowpass_workspace_bytes", B, H, W, factor, hk)
    if need == 0:
        raise _lib.SifsrError(f"lowpass: raster {tuple(x.shape)}, factor {factor}, hkw {hk or None} is outside the limits (1 < factor <= "
                              f"{degrade.MAX_FACTOR:g}, half width hw = hkw or ceil(factor) in 1..{degrade.MAX_HALF_WIDTH}, hw + 1 <= side <= "
                              f"{degrade.MAX_SIDE}, 1..65535 images)")
    ws = torch.empty((need,), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    _lib.call(name, x, out, ws, need, B, H, W, factor, mtf, hk, _lib.stream_ptr(x.device))
    return out


def lowpass(x, factor, mtf=0.1, hkw=None):
    """``get_output_ftm(x, factor=f, mtf)`` (utils.py:1833-1860) at any factor, autograd-capable: the Gaussian of ``mtf`` at the
    target Nyquist frequency, 2 hw + 1 taps with hw = hkw or ceil(factor), over the raster reflected by hw without repeating the
    edge (needs sides >= hw + 1).  x (H,W), (B,H,W) or (B,C,H,W) float32 on the device -> the same shape."""
    _images(x, "lowpass")
    return _Lowpass.apply(x, float(factor), _mtf(mtf), degrade._hkw(hkw))


def sif_loss(kind, sr, lst, ndvi, factor, mean, std, alpha, gamma):
    """The loss block of the training scripts (kind='sr2': train_model_B_gradFTM.py:99-117; kind='sr1':
    train_model_B_predef_filters.py:111-133) with the sensor model at ``factor``, composed from autograd ops (not fused):

        ds   = huber((downscale(sr * std + mean, factor, mtf=0.1) - mean) / std, lst)
        pl   = huber(sr - lowpass(sr, factor, 0.25), gamma * (ndvi - lowpass(ndvi, factor, 0.25)))          'sr2'
               huber(sobel_bank(sr), gamma * sobel_bank(ndvi))                                              'sr1'
        loss = alpha * ds + (1 - alpha) * pl

    sr, ndvi (B,1,H,W), lst (B,1,*lr_shape(H, W, factor)).  Returns (ds, pl, loss) as 0-d device tensors; only ``loss`` carries a
    gradient."""
    if kind not in ("sr2", "sr1"):
        raise _lib.SifsrError(f"sif_loss: kind must be 'sr2' or 'sr1', got {kind!r}")
    for t, n in ((sr, "sr"), (lst, "lst"), (ndvi, "ndvi")):
        if not isinstance(t, torch.Tensor):
            raise _lib.SifsrError(f"sif_loss: {n} must be a tensor, got {type(t).__name__}")
    if sr.dim() != 4 or sr.shape[1] != 1 or ndvi.shape != sr.shape:
        raise _lib.SifsrError(f"sif_loss expects sr and ndvi (B,1,H,W), got {tuple(sr.shape)} and {tuple(ndvi.shape)}")
    B, _, H, W = sr.shape
    want = (B, 1) + lr_shape(H, W, factor)
    if tuple(lst.shape) != want:
        raise _lib.SifsrError(f"sif_loss: lst must be {want} at factor {factor} (sensor.lr_shape), got {tuple(lst.shape)}")
    for t, n in ((sr, "sr"), (lst, "lst"), (ndvi, "ndvi")):
        _lib.require_gpu(t.detach(), n)
    mean, std = float(mean), float(std)
    down = (downscale(sr * std + mean, factor, mtf=0.1) - mean) / std
    ds = huber_loss(down, lst)
    if kind == "sr2":
        pl = huber_loss(sr - lowpass(sr, factor, 0.25), ndvi - lowpass(ndvi, factor, 0.25), target_scale=gamma)
    else:
        pl = huber_loss(sobel_bank(sr), sobel_bank(ndvi), target_scale=gamma)
    loss = alpha * ds + (1 - alpha) * pl
    return ds.detach(), pl.detach(), loss


def train_step(model, optimizer, lst, lst_up, ndvi, stats, alpha, gamma, factor, kind="sr2", sync_grads=True, return_sr=False):
    """The step of ``train.train_step`` at any ratio: ``sr = model(cat(lst_up, ndvi))``, ``sensor.sif_loss(..., factor)``,
    ``loss.backward()``, ``optimizer.step()``.  lst (B,1,h,w) with (h, w) = ``lr_shape(H, W, factor)``; lst_up, ndvi (B,1,H,W), H
    and W multiples of 8.  ``lst_up`` is plumbing:
    ``F.interpolate(lst, size=(H, W), mode="bicubic", align_corners=False)`` on the device (torch's own kernel); at x4 ``pipeline.bicubic_up4`` stays the
    path.  Works with ``model.bn_frozen`` as the ordinary step does.  Returns device scalars (ds_loss, percep_loss, loss) -- no host
    sync -- and, with ``return_sr``, the detached training-mode prediction."""
    mean, std = stats["mean_lst"], stats["std_lst"]
    loss_fn = lambda sr: sif_loss(kind, sr, lst, ndvi, factor, mean, std, alpha, gamma) + (None,)   # (no dsr: loss.backward())
    ds, pl, loss, *sr = train._optimise(model, optimizer, lst_up, ndvi, loss_fn, sync_grads, return_sr)
    return (ds, pl, loss.detach(), *sr)
