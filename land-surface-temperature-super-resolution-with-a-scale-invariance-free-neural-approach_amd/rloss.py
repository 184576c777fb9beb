"""The scale-invariance-free loss at any ratio as two fused kernels, masked (include/sifsr_rloss.h,
csrc/rloss.hip): what ``sensor.sif_loss`` composes from a few dozen launches, and what it cannot do -- leave out the cloudy cells of
a partly valid patch -- in one call with its gradient.

    valid_counts(valid, hr_shape)      (n1, n2) on the device: the valid LR cells and the HR pixels under them
    sif_loss_with_grad / sif_loss      the loss block at ``factor``, optionally over the valid cells only
    train_step                         ``sensor.train_step`` with the fused loss, ``valid=`` for cloudy patches (``train._optimise``)
    eval_step / train_epoch / eval_epoch / fit
                                       ``train.eval_step`` / ``train_epoch`` / ``eval_epoch`` / ``fit`` at ``factor``, over the loaders
                                       of patches mined at a ratio (``sifsr.rproducts``)
    adapt_granule                      ``adapt.adapt_granule`` at ratio hr / window: its own checks, then the same loop

The LR cell of HR pixel (Y, X) is (Y h // H, X w // W): the rule under which ``ratio.predict_granule_gaps`` masks its output.
Limits (``sifsrq_sif_loss``): 1 < factor <= 8, sides of ceil(factor) + 1 .. 16384, the half width of the sensor model at its
default ceil(factor), at most 65535 images; ``sensor.sif_loss`` (composed, unmasked) serves what lies beyond them.  Everything is
fp32 on the device; CPU tensors raise SifsrError: there is no CPU path.

The consistency check and the residual correction at a ratio are ``sifsr.rconserve``.
Out of scope here: ``GraphedTrainStep`` at a ratio (the call itself can be captured), a captured
``GranulePredictor`` at a ratio, the ``hkw`` argument in the loss, and bf16."""
from __future__ import annotations

import torch

from . import _lib, adapt, gaps, metrics, ratio, rproducts, sensor, train

MAX_FACTOR = 8.0
MAX_SIDE = 16384
_KINDS = {"sr2": 2, "sr1": 1}
_LIMITS = (f"1 < factor <= {MAX_FACTOR:g}, sides of ceil(factor) + 1 .. {MAX_SIDE}, 1..65535 images; sensor.sif_loss serves what lies "
           "beyond these limits")


def _factor(factor, what):
    try:
        f = float(factor)
    except (TypeError, ValueError):
        raise _lib.SifsrError(f"{what}: factor must be a number, got {factor!r}") from None
    if not 1.0 < f <= MAX_FACTOR:
        raise _lib.SifsrError(f"{what}: factor {factor} is outside the limits of the fused loss ({_LIMITS})")
    return f


def _lr_mask(valid, shape, device, what):
    """``gaps._valid_raster`` for one byte per LR cell: (B,1,h,w) or (B,h,w), on ``device`` (None: any GPU)"""
    B, h, w = shape
    want = (B, h, w) if tuple(getattr(valid, "shape", ())) == (B, h, w) else (B, 1, h, w)
    return gaps._valid_raster(valid, want, device, f"{what}: valid")


def valid_counts(valid, hr_shape):
    """valid (B,1,h,w) or (B,h,w) uint8 / bool on the device, ``hr_shape`` = (H, W) of the HR patch -> int64 (2,) on the device:
    n1 = the valid LR cells, n2 = the HR pixels (Y, X) whose cell (Y h // H, X w // W) is valid (``sifsrq_valid_counts``; integer
    arithmetic, nothing is read back).  At x2.5 a cell holds 2 or 3 pixels per axis: n2 is the exact count."""
    if not isinstance(valid, torch.Tensor) or valid.dim() not in (3, 4):
        raise _lib.SifsrError(f"valid_counts: valid must be a (B,1,h,w) or (B,h,w) tensor, got {getattr(valid, 'shape', type(valid).__name__)}")
    try:
        H, W = (int(v) for v in hr_shape)
    except (TypeError, ValueError):
        raise _lib.SifsrError(f"valid_counts: hr_shape must be (H, W), got {hr_shape!r}") from None
    B, h, w = valid.shape[0], valid.shape[-2], valid.shape[-1]
    v = _lr_mask(valid, (B, h, w), None, "valid_counts")
    if not (1 <= B <= 65535 and 1 <= h <= H <= MAX_SIDE and 1 <= w <= W <= MAX_SIDE):
        raise _lib.SifsrError(f"valid_counts: a mask {tuple(valid.shape)} under an HR patch {(H, W)}: needs 1..65535 images and LR sides "
                              f"of 1 .. the HR side <= {MAX_SIDE}")
    counts = torch.empty((2,), dtype=torch.int64, device=v.device)
    _lib.call("sifsrq_valid_counts", v, B, h, w, H, W, counts, _lib.stream_ptr(v.device))
    return counts


def _args(kind, sr, lst, ndvi, factor, valid, counts, what, strict=False):
    """every check that needs no launch -> (k, B, H, W, factor, valid or None, counts or None); ``strict``: valid and counts come
    together or not at all (the C entry point's rule), otherwise missing counts are formed from valid"""
    if kind not in _KINDS:
        raise _lib.SifsrError(f"{what}: kind must be 'sr2' or 'sr1', got {kind!r}")
    for t, n in ((sr, "sr"), (lst, "lst"), (ndvi, "ndvi")):
        if not isinstance(t, torch.Tensor):
            raise _lib.SifsrError(f"{what}: {n} must be a tensor, got {type(t).__name__}")
    if sr.dim() != 4 or sr.shape[1] != 1 or ndvi.shape != sr.shape:
        raise _lib.SifsrError(f"{what} expects sr and ndvi (B,1,H,W), got {tuple(sr.shape)} and {tuple(ndvi.shape)}")
    f = _factor(factor, what)
    B, _, H, W = sr.shape
    if not (1 <= B <= 65535 and H <= MAX_SIDE and W <= MAX_SIDE):
        raise _lib.SifsrError(f"{what}: {tuple(sr.shape)} is outside the limits of the fused loss ({_LIMITS})")
    h, w = sensor.lr_shape(H, W, f)                                       # (raises SifsrError for sides under ceil(factor) + 1)
    if tuple(lst.shape) != (B, 1, h, w):
        raise _lib.SifsrError(f"{what}: lst must be {(B, 1, h, w)} at factor {factor} (sensor.lr_shape), got {tuple(lst.shape)}")
    if (valid is None) != (counts is None) and (strict or valid is None):
        raise _lib.SifsrError(f"{what}: exactly one of valid / counts was given: pass valid with counts = valid_counts(valid, (H, W)), "
                              "or neither" + ("" if strict else " (counts=None with valid forms them)"))
    for t, n in ((sr, "sr"), (lst, "lst"), (ndvi, "ndvi")):
        _lib.require_gpu(t, n)
    if valid is not None:
        valid = _lr_mask(valid, (B, h, w), sr.device, what)
        if counts is None:
            counts = valid_counts(valid, (H, W))
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or tuple(counts.shape) != (2,) or counts.device != sr.device \
                or not counts.is_contiguous():
            raise _lib.SifsrError(f"{what}: counts must be the int64 (2,) device tensor of valid_counts(valid, (H, W))")
    return _KINDS[kind], B, H, W, f, valid, counts


def _call(k, sr, lst, ndvi, B, H, W, f, mean, std, alpha, gamma, valid, counts, with_grad):
    need = _lib.call("sifsrq_sif_loss_workspace_bytes", k, B, H, W, f)
    if need == 0:
        raise _lib.SifsrError(f"sif_loss: {(B, 1, H, W)} at factor {f} is outside the limits of the fused loss ({_LIMITS})")
    ws = torch.empty((need,), dtype=torch.uint8, device=sr.device)
    losses = torch.empty((3,), dtype=torch.float32, device=sr.device)
    dsr = torch.empty_like(sr) if with_grad else None
    _lib.call("sifsrq_sif_loss", k, sr, lst, valid, counts, ndvi, B, H, W, f, float(mean), float(std), float(alpha), float(gamma), ws, need,
              losses, dsr, _lib.stream_ptr(sr.device))
    return losses, dsr


def sif_loss_with_grad(kind, sr, lst, ndvi, factor, mean, std, alpha, gamma, valid=None, counts=None):
    """The loss block of ``sensor.sif_loss`` and d loss / d sr WITHOUT an autograd node, fused (``sifsrq_sif_loss``):

        ds   = mean over the valid LR cells of      huber((downscale(sr std + mean, factor, mtf 0.1) - mean) / std - lst)
        pl   = mean over the HR pixels under them of huber((sr - lowpass(sr, factor, 0.25)) - gamma (ndvi - lowpass(ndvi, ..)))  'sr2'
                                                     huber(sobel_bank(sr) - gamma sobel_bank(ndvi))                              'sr1'
        loss = alpha ds + (1 - alpha) pl

    sr, ndvi (B,1,H,W), lst (B,1,*sensor.lr_shape(H, W, factor)); ``valid`` (B,1,h,w) uint8 / bool marks the LR cells that count,
    ``counts`` = ``valid_counts(valid, (H, W))``; both or neither (exactly one raises SifsrError): without them every cell counts,
    bit for bit what an all-ones mask gives.  ``lst`` under an invalid cell is never read, and the gradient there is what the blur and the low-pass of the valid
    neighbours leave.  -> (losses (3,) = (ds, pl, loss), dsr (B,1,H,W)), device tensors; nothing is read back.  ``sr`` may carry a
    graph; it is only read."""
    srd = sr.detach().contiguous() if isinstance(sr, torch.Tensor) else sr
    lst, ndvi = (t.contiguous() if isinstance(t, torch.Tensor) else t for t in (lst, ndvi))
    k, B, H, W, f, valid, counts = _args(kind, srd, lst, ndvi, factor, valid, counts, "sif_loss_with_grad", strict=True)
    return _call(k, srd, lst, ndvi, B, H, W, f, mean, std, alpha, gamma, valid, counts, True)


class _RatioSifLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sr, lst, ndvi, valid, counts, k, B, H, W, f, mean, std, alpha, gamma):
        losses, dsr = _call(k, sr, lst, ndvi, B, H, W, f, mean, std, alpha, gamma, valid, counts, ctx.needs_input_grad[0])
        ctx.dsr = dsr
        ds, pl, loss = losses[0], losses[1], losses[2]
        ctx.mark_non_differentiable(ds, pl)
        ctx.set_materialize_grads(False)
        return ds, pl, loss

    @staticmethod
    def backward(ctx, g_ds, g_pl, g_loss):
        dsr = ctx.dsr
        ctx.dsr = None
        if g_loss is None:
            return (None,) * 14
        if dsr is None:
            raise _lib.SifsrError("sif_loss: backward called twice (d loss / d sr was released after the first call)")
        return (dsr * g_loss,) + (None,) * 13


def sif_loss(kind, sr, lst, ndvi, factor, mean, std, alpha, gamma, valid=None, counts=None):
    """``sif_loss_with_grad`` as an autograd op: -> (ds, pl, loss) as 0-d device tensors; only ``loss`` carries a gradient (to
    ``sr``), the stored d loss / d sr scaled by the incoming one.  With ``valid`` given and ``counts=None`` the counts are formed
    by ``valid_counts``."""
    srd = sr.contiguous() if isinstance(sr, torch.Tensor) else sr
    lst, ndvi = (t.contiguous() if isinstance(t, torch.Tensor) else t for t in (lst, ndvi))
    k, B, H, W, f, valid, counts = _args(kind, srd.detach() if isinstance(srd, torch.Tensor) else srd, lst, ndvi, factor, valid, counts,
                                         "sif_loss")
    return _RatioSifLoss.apply(srd, lst, ndvi, valid, counts, k, B, H, W, f, mean, std, alpha, gamma)


def train_step(model, optimizer, lst, lst_up, ndvi, stats, alpha, gamma, factor, kind="sr2", valid=None, counts=None, sync_grads=True,
               return_sr=False):
    """``sensor.train_step`` with the fused loss: ``sr = model(cat(lst_up, ndvi))``, the loss and d loss / d sr of
    ``sif_loss_with_grad(..., factor, valid=, counts=)`` (``counts=None`` with ``valid``: formed by ``valid_counts``),
    ``sr.backward(dsr)``, ``optimizer.step()``.  With ``valid`` (B,1,h,w) the step trains on partly cloudy patches:
    ``lst`` / ``lst_up`` are then the FILLED patch and its upsampling, and an invalid cell adds nothing to the loss or the gradient.
    Works with ``model.bn_frozen``.  Under data parallelism each rank normalises by its own counts before the gradients are
    averaged, as ``train.train_step`` does.  Returns device scalars (ds_loss, percep_loss, loss) -- no host sync -- and, with
    ``return_sr``, the detached training-mode prediction."""
    def loss_fn(sr):
        srd, lst_c, ndvi_c = sr.detach().contiguous(), lst.contiguous(), ndvi.contiguous()
        k, B, H, W, f, v, c = _args(kind, srd, lst_c, ndvi_c, factor, valid, counts, "train_step")
        losses, dsr = _call(k, srd, lst_c, ndvi_c, B, H, W, f, stats["mean_lst"], stats["std_lst"], alpha, gamma, v, c, True)
        return losses[0], losses[1], losses[2], dsr

    return train._optimise(model, optimizer, lst_up, ndvi, loss_fn, sync_grads, return_sr)


@torch.inference_mode()
def eval_step(model, lst, lst_up, ndvi, stats, alpha, gamma, factor, kind="sr2", valid=None, counts=None):
    """``train.eval_step`` at ``factor``: eval mode, no gradient, -> (ds, pl, loss) as device scalars.  ``valid`` / ``counts``: as
    ``train_step`` (``counts=None`` with ``valid``: formed by ``valid_counts``)."""
    model.eval()
    sr = model(torch.cat((lst_up, ndvi), dim=1))
    return _eval_losses(sr, lst, ndvi, stats, alpha, gamma, factor, kind, valid, counts, "eval_step")


def _eval_losses(sr, lst, ndvi, stats, alpha, gamma, factor, kind, valid, counts, what):
    sr, lst, ndvi = sr.contiguous(), lst.contiguous(), ndvi.contiguous()
    k, B, H, W, f, v, c = _args(kind, sr, lst, ndvi, factor, valid, counts, what)
    losses, _ = _call(k, sr, lst, ndvi, B, H, W, f, stats["mean_lst"], stats["std_lst"], alpha, gamma, v, c, False)
    return losses[0], losses[1], losses[2]


def _unpack_batch(batch, device):
    """``train._unpack_batch`` for the batches of a loader at a ratio: the fifth item is the (2,) counts of ``valid_counts``, or
    (b,2) per-patch rows that are summed on the device; nothing is read back."""
    if len(batch) not in (3, 5):
        raise _lib.SifsrError(f"a batch has 3 or 5 items, got {len(batch)}")
    lst, lst_up, ndvi = (t.to(device) for t in batch[:3])
    if len(batch) == 3:
        return lst, lst_up, ndvi, None, None
    valid, counts = batch[3].to(device), batch[4].to(device=device, dtype=torch.int64)
    if counts.shape[-1:] != (2,) or counts.dim() not in (1, 2):
        raise _lib.SifsrError(f"the fifth item of a batch at a ratio is the (2,) counts of valid_counts or (b,2) rows, got {tuple(counts.shape)}")
    return lst, lst_up, ndvi, valid, (counts.sum(0) if counts.dim() == 2 else counts).contiguous()


def _score(sr, lst_up, valid, masked_metrics, acc, den):
    """``train._score`` with the LR mask expanded to the HR mask ``metrics.masked_psnr_ssim`` takes at scale 1"""
    if masked_metrics and valid is not None:
        valid = rproducts.expand_valid(valid, sr.shape[-2:])
    train._score(sr, lst_up, valid, masked_metrics, acc, den)


def train_epoch(model, loader, optimizer, stats, alpha, gamma, factor, kind="sr2", device="cuda", with_metrics=True,
                masked_metrics=False):
    """``train.train_epoch`` at ``factor``: one ``rloss.train_step`` per batch of ``loader`` (``MinedPatches.loader`` /
    ``masked_loader`` of patches mined by ``rproducts.PatchMiner``; batches of three, or of five with the counts), -> the epoch means
    (ds_loss, percep_loss, loss, psnr, ssim), read back ONCE per epoch.  PSNR / SSIM score the training-mode prediction against
    ``lst_up``; ``masked_metrics``: over the HR pixels under valid cells only (``rproducts.expand_valid``, then
    ``metrics.masked_psnr_ssim``)."""
    acc = torch.zeros(5, dtype=torch.float64, device=device)
    den = torch.zeros(5, dtype=torch.float64, device=device)
    n = 0
    for batch in loader:
        lst, lst_up, ndvi, valid, counts = _unpack_batch(batch, device)
        ds, pl, loss, sr = train_step(model, optimizer, lst, lst_up, ndvi, stats, alpha, gamma, factor, kind, valid=valid, counts=counts,
                                      return_sr=True)
        acc[0] += ds.detach(); acc[1] += pl.detach(); acc[2] += loss.detach()
        if with_metrics:
            _score(sr, lst_up, valid, masked_metrics, acc, den)
        n += 1
    return train._epoch_means(acc, den, n, with_metrics)


@torch.inference_mode()
def eval_epoch(model, loader, stats, alpha, gamma, factor, kind="sr2", device="cuda", with_metrics=True, masked_metrics=False):
    """``train.eval_epoch`` at ``factor``: eval mode, no gradient; the epoch means of (ds_loss, percep_loss, loss, psnr, ssim)."""
    model.eval()
    acc = torch.zeros(5, dtype=torch.float64, device=device)
    den = torch.zeros(5, dtype=torch.float64, device=device)
    n = 0
    for batch in loader:
        lst, lst_up, ndvi, valid, counts = _unpack_batch(batch, device)
        sr = model(torch.cat((lst_up, ndvi), dim=1))
        ds, pl, loss = _eval_losses(sr, lst, ndvi, stats, alpha, gamma, factor, kind, valid, counts, "eval_epoch")
        acc[0] += ds; acc[1] += pl; acc[2] += loss
        if with_metrics:
            _score(sr, lst_up, valid, masked_metrics, acc, den)
        n += 1
    return train._epoch_means(acc, den, n, with_metrics)


def fit(model, train_loader, val_loader, n_epochs, optimizer, stats, alpha, gamma, factor, kind="sr2", checkpoint=None,
        masked_metrics=False):
    """``train.fit`` at ``factor`` over two loaders (``MinedPatches.loader`` / ``masked_loader``, which shuffle per epoch themselves):
    per epoch one ``train_epoch`` and one ``eval_epoch``, the same ``metrics`` dict, ``best_epoch`` rule and restore of the best
    state through ``checkpoint`` (``train.ModelCheckpoint``).  Returns (model, metrics)."""
    device = next(model.parameters()).device
    return train._fit(model, n_epochs, checkpoint,
                      lambda: train_epoch(model, train_loader, optimizer, stats, alpha, gamma, factor, kind, device, masked_metrics=masked_metrics),
                      lambda: eval_epoch(model, val_loader, stats, alpha, gamma, factor, kind, device, masked_metrics=masked_metrics))


def adapt_granule(model, lst_g, ndvi_g, stats, window, hr, mask=None, steps=20, lr=1e-5, alpha=0.5, gamma=1.0, kind="sr2", batch=16,
                  overlap=0, cover_edges=False, optimizer=None):
    """``adapt.adapt_granule`` at ratio ``hr / window``: ``steps`` optimisation steps of the masked loss on the active tiles of one
    gappy granule (raw LST (h,w) [K], raw NDVI (h p/q, w p/q), ``mask`` as in ``gaps.fill_gaps``), BatchNorm statistics frozen.
    The layout is ``ratio.geometry``'s; fill, selection and loss targets are ``gaps.fill_gaps``, ``gaps.select_tiles`` and
    ``adapt.tile_targets`` (they see the LST raster only), the network inputs ``ratio.prepare_active_tiles``; step i is
    ``rloss.train_step(..., factor=hr / window, valid=)`` on the min(batch, n_active) tiles from position i * batch of the active
    list, cyclic.  A ``(window, hr)`` whose ``sensor.lr_shape(hr, hr, hr / window)`` is not ``(window, window)`` -- (16, 20): the
    sensor model's crop leaves 17 -- is refused before any launch.  The read of the active count is the only host synchronisation;
    no active tile: no step, no forward.  Returns an ``adapt.Adaptation``; the model's mode and ``bn_frozen`` are as they were."""
    for t, n in ((lst_g, "lst granule"), (ndvi_g, "ndvi granule")):
        if not isinstance(t, torch.Tensor):
            raise _lib.SifsrError(f"adapt_granule: {n} must be a tensor, got {type(t).__name__}")
    if lst_g.dim() != 2:
        raise _lib.SifsrError(f"lst granule: expected a 2-D raster, got {tuple(lst_g.shape)}")
    try:
        window, hr = int(window), int(hr)
    except (TypeError, ValueError):
        raise _lib.SifsrError(f"adapt_granule: window and hr must be integers, got {window!r}, {hr!r}") from None
    if window < 1 or hr <= window:
        raise _lib.SifsrError(f"adapt_granule: needs 1 <= window < hr, got window {window}, hr {hr}")
    factor = _factor(hr / window, "adapt_granule")
    if kind not in _KINDS:
        raise _lib.SifsrError(f"adapt_granule: kind must be 'sr2' or 'sr1', got {kind!r}")
    got = sensor.lr_shape(hr, hr, factor)
    if got != (window, window):
        raise _lib.SifsrError(f"adapt_granule: at ratio {hr}/{window} the sensor model sees {got} of an {(hr, hr)} tile, not "
                              f"{(window, window)} (sensor.lr_shape: the crop of the sensor model cuts floor(ceil(factor) / factor) cells on "
                              "each side); choose a window and hr whose LR tile is the window")
    lay = ratio._tile_layout(lst_g, ndvi_g.shape, window, hr, overlap, cover_edges)            # (raises before any launch)
    if window % 4:
        raise _lib.SifsrError(f"window must be a multiple of 4 for the tile selection, got {window}")
    if int(batch) < 1 or int(steps) < 0:
        raise _lib.SifsrError(f"batch must be positive and steps non-negative, got {batch}, {steps}")
    _lib.require_gpu(lst_g, "lst granule"); _lib.require_gpu(ndvi_g, "ndvi granule")

    def step(model, optimizer, lst, xb, vt, n_valid):                       # (the fused loss forms its own counts from vt)
        return train_step(model, optimizer, lst, xb[:, 0:1], xb[:, 1:2], stats, alpha, gamma, factor, kind=kind, valid=vt)

    return adapt._adapt(model, lay, step, lst_g, ndvi_g, stats, mask, int(steps), int(batch), lr, optimizer)
