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
    GraphedTrainStep                   ``train.GraphedTrainStep`` for ``train_step`` at hr / window: the step as one hipGraph, replayed
                                       (DESIGN.md §9 f23); ``train_epoch`` / ``fit`` / ``adapt_granule`` take it as ``graphed=``

The LR cell of HR pixel (Y, X) is (Y h // H, X w // W): the rule under which ``ratio.predict_granule_gaps`` masks its output.
Limits (``sifsrq_sif_loss``): 1 < factor <= 8, sides of ceil(factor) + 1 .. 16384, the half width of the sensor model at its
default ceil(factor), at most 65535 images; ``sensor.sif_loss`` (composed, unmasked) serves what lies beyond them.  Everything is
fp32 on the device; CPU tensors raise SifsrError: there is no CPU path.

The consistency check and the residual correction at a ratio are ``sifsr.rconserve``; the captured granule
predictor at a ratio is ``ratio.GranulePredictor`` (§9 f23).
Out of scope here: gradient exchange inside the captured step, the ``hkw`` argument in the loss, and bf16."""
from __future__ import annotations

import torch

from . import _granule, _lib, adapt, gaps, metrics, ratio, rproducts, sensor, train

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


class GraphedTrainStep:
    """``train.GraphedTrainStep`` for ``rloss.train_step`` at ``factor = hr / window``: one whole step -- cat,
    forward, the fused loss at the ratio, backward, Adam -- captured once into a hipGraph and replayed per batch.  The same capture
    rule (three eager calls, the fourth captures, later calls replay) and the same rules of DESIGN.md §10: the outputs are
    detached, the optimizer is ``FlatAdam(capturable=True)`` (else ValueError), single GPU (no gradient exchange in the graph).

    Static buffers: ``lst`` (batch,1,window,window), ``lst_up`` and ``ndvi`` (batch,1,hr,hr); ``masked``: also ``valid``
    (batch,1,window,window) uint8 and ``counts`` (2,) int64.  The captured region forms ``valid_counts(valid, (hr, hr))`` itself
    and takes the static ``counts`` in its place, by a select on the device, when the call gave counts: one graph serves every
    mask, with the counts given or formed.  ``return_sr``: the step also returns the static training-mode prediction.

    ``(window, hr)`` must be a pair ``rproducts.trainable`` accepts (SifsrError naming the rule, before any launch).  The step
    works under ``adapt.frozen_bn(model)``: the mode of the first call is the mode of the warm-up calls, the capture and every replay,
    and a call whose ``model.bn_frozen`` differs from it is refused."""

    def __init__(self, model, optimizer, batch, stats, alpha, gamma, window, hr, kind="sr2", masked=False, return_sr=False, device=None):
        rproducts.trainable(window, hr)
        window, hr = int(window), int(hr)
        if kind not in _KINDS:
            raise _lib.SifsrError(f"GraphedTrainStep: kind must be 'sr2' or 'sr1', got {kind!r}")
        if int(batch) < 1:
            raise _lib.SifsrError(f"GraphedTrainStep: batch must be positive, got {batch}")
        if not getattr(optimizer, "capturable", False):
            raise ValueError("GraphedTrainStep needs FlatAdam(..., capturable=True)")
        dev = device or next(model.parameters()).device
        batch = int(batch)
        self.model, self.opt, self.batch, self.window, self.hr, self.kind = model, optimizer, batch, window, hr, kind
        self.factor, self.masked, self.return_sr = hr / window, bool(masked), bool(return_sr)
        self.lst = torch.zeros((batch, 1, window, window), dtype=torch.float32, device=dev)
        self.lst_up = torch.zeros((batch, 1, hr, hr), dtype=torch.float32, device=dev)
        self.ndvi = torch.zeros((batch, 1, hr, hr), dtype=torch.float32, device=dev)
        self.valid = torch.zeros((batch, 1, window, window), dtype=torch.uint8, device=dev) if self.masked else None
        self.counts = torch.zeros((2,), dtype=torch.int64, device=dev) if self.masked else None
        self._given = torch.zeros((1,), dtype=torch.bool, device=dev) if self.masked else None

        def step():
            counts = None
            if self.masked:
                counts = torch.where(self._given, self.counts, valid_counts(self.valid, (hr, hr)))
            out = train_step(model, optimizer, self.lst, self.lst_up, self.ndvi, stats, alpha, gamma, self.factor, kind=kind,
                             valid=self.valid, counts=counts, sync_grads=False, return_sr=self.return_sr)
            return tuple(t.detach() for t in out)                       # (detached: train.GraphedTrainStep says why)

        self._eager = step
        self.graph = None
        self.bn_frozen = None                                           # the mode of the first call, and of every later one
        self._warm = 0
        self.out = None

    def __call__(self, lst, lst_up, ndvi, valid=None, counts=None):
        """Copies the batch into the static inputs and runs the step; returns the device scalars (ds, pl, loss) and, with
        ``return_sr``, the prediction -- static tensors once the step replays: the next call overwrites them.  ``masked``:
        ``valid`` is required, and ``counts`` may be None (formed inside the captured region) or a device (2,) / (b,2) int64
        tensor (copied / summed on the device, as ``_unpack_batch`` does); otherwise both are refused.  Nothing is read back."""
        if self.masked != (valid is not None) or (counts is not None and not self.masked):
            raise ValueError("GraphedTrainStep: valid (and counts) go with masked=True, and valid is required with it")
        frozen = bool(getattr(self.model, "bn_frozen", False))
        if self.bn_frozen is None:
            self.bn_frozen = frozen
        if frozen != self.bn_frozen:
            raise ValueError(f"GraphedTrainStep took its first call with model.bn_frozen = {self.bn_frozen}; this call has {frozen}")
        if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dim() not in (1, 2) or counts.shape[-1:] != (2,)
                                   or counts.device != self.counts.device):
            raise ValueError("GraphedTrainStep: counts must be a (2,) or (b,2) integer tensor on the step's device")
        self.lst.copy_(lst); self.lst_up.copy_(lst_up); self.ndvi.copy_(ndvi)
        if self.masked:
            self.valid.copy_(valid.reshape(self.valid.shape))
            self._given.fill_(counts is not None)
            if counts is not None:
                self.counts.copy_(counts.sum(0) if counts.dim() == 2 else counts)
        if self.graph is not None:
            self.graph.replay()
            return self.out
        if self._warm < 3:
            self._warm += 1
            return self._eager()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):          # records the step's kernels; nothing runs yet
            self.out = self._eager()
        self.graph = g
        g.replay()                         # this call's step
        return self.out


def _graphed_for(graphed, model, optimizer, factor, kind, with_metrics, what):
    """the checks of ``graphed=`` in the epoch loops, before the first batch"""
    if graphed is None:
        return
    if not isinstance(graphed, GraphedTrainStep):
        raise ValueError(f"{what}: graphed must be an rloss.GraphedTrainStep, got {type(graphed).__name__}")
    if graphed.model is not model or graphed.opt is not optimizer or graphed.kind != kind or graphed.factor != float(factor):
        raise ValueError(f"{what}: the captured step was built for another model, optimizer, kind or factor "
                         f"(kind {graphed.kind!r}, factor {graphed.factor:g}; the call: {kind!r}, {float(factor):g})")
    if with_metrics and not graphed.return_sr:
        raise ValueError(f"{what}: with_metrics needs a GraphedTrainStep built with return_sr=True")


def _train_epoch(model, loader, optimizer, stats, alpha, gamma, factor, kind, device, with_metrics, masked_metrics, graphed=None):
    _graphed_for(graphed, model, optimizer, factor, kind, with_metrics, "train_epoch")
    acc = torch.zeros(5, dtype=torch.float64, device=device)
    den = torch.zeros(5, dtype=torch.float64, device=device)
    n = 0
    for batch in loader:
        lst, lst_up, ndvi, valid, counts = _unpack_batch(batch, device)
        if graphed is not None and lst.shape[0] == graphed.batch:
            ds, pl, loss, *sr = graphed(lst, lst_up, ndvi, valid, counts)
            sr = sr[0] if sr else None
        else:                                                            # (no step given, or a shorter last batch: batch statistics forbid padding)
            ds, pl, loss, sr = train_step(model, optimizer, lst, lst_up, ndvi, stats, alpha, gamma, factor, kind, valid=valid, counts=counts,
                                          return_sr=True)
        acc[0] += ds.detach(); acc[1] += pl.detach(); acc[2] += loss.detach()
        if with_metrics:
            _score(sr, lst_up, valid, masked_metrics, acc, den)
        n += 1
    return train._epoch_means(acc, den, n, with_metrics)


@_granule.keyword_options(_train_epoch, graphed=None)
def train_epoch(model, loader, optimizer, stats, alpha, gamma, factor, kind="sr2", device="cuda", with_metrics=True,
                masked_metrics=False):
    """``train.train_epoch`` at ``factor``: one ``rloss.train_step`` per batch of ``loader`` (``MinedPatches.loader`` /
    ``masked_loader`` of patches mined by ``rproducts.PatchMiner``; batches of three, or of five with the counts), -> the epoch means
    (ds_loss, percep_loss, loss, psnr, ssim), read back ONCE per epoch.  PSNR / SSIM score the training-mode prediction against
    ``lst_up``; ``masked_metrics``: over the HR pixels under valid cells only (``rproducts.expand_valid``, then
    ``metrics.masked_psnr_ssim``).

    Keyword-only ``graphed=step`` (``_granule.keyword_options``; default None: the calls above, bit for bit): an
    ``rloss.GraphedTrainStep`` built for this model, optimizer, kind and factor -- with ``return_sr=True`` when ``with_metrics`` --
    takes the batches of its captured size; a shorter last batch runs the eager ``train_step`` (batch statistics forbid
    padding)."""


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


def _fit(model, train_loader, val_loader, n_epochs, optimizer, stats, alpha, gamma, factor, kind, checkpoint, masked_metrics, graphed=None):
    _graphed_for(graphed, model, optimizer, factor, kind, True, "fit")
    device = next(model.parameters()).device
    return train._fit(model, n_epochs, checkpoint,
                      lambda: train_epoch(model, train_loader, optimizer, stats, alpha, gamma, factor, kind, device, masked_metrics=masked_metrics,
                                          graphed=graphed),
                      lambda: eval_epoch(model, val_loader, stats, alpha, gamma, factor, kind, device, masked_metrics=masked_metrics))


@_granule.keyword_options(_fit, graphed=None)
def fit(model, train_loader, val_loader, n_epochs, optimizer, stats, alpha, gamma, factor, kind="sr2", checkpoint=None,
        masked_metrics=False):
    """``train.fit`` at ``factor`` over two loaders (``MinedPatches.loader`` / ``masked_loader``, which shuffle per epoch themselves):
    per epoch one ``train_epoch`` and one ``eval_epoch``, the same ``metrics`` dict, ``best_epoch`` rule and restore of the best
    state through ``checkpoint`` (``train.ModelCheckpoint``).  Returns (model, metrics).

    Keyword-only ``graphed=step``: as in ``train_epoch`` (an ``rloss.GraphedTrainStep`` with ``return_sr=True``; the validation
    pass and a restore of the best state run as they did: the parameters keep their addresses)."""


def _adapt_granule(model, lst_g, ndvi_g, stats, window, hr, mask, steps, lr, alpha, gamma, kind, batch, overlap, cover_edges, optimizer,
                   graphed=False):
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

    def captured(model, optimizer, b):
        g = GraphedTrainStep(model, optimizer, b, stats, alpha, gamma, window, hr, kind=kind, masked=True)
        return lambda model, optimizer, lst, xb, vt, n_valid: g(lst, xb[:, 0:1], xb[:, 1:2], vt)

    return adapt._adapt(model, lay, step, lst_g, ndvi_g, stats, mask, int(steps), int(batch), lr, optimizer, captured if graphed else None)


@_granule.keyword_options(_adapt_granule, graphed=False)
def adapt_granule(model, lst_g, ndvi_g, stats, window, hr, mask=None, steps=20, lr=1e-5, alpha=0.5, gamma=1.0, kind="sr2", batch=16,
                  overlap=0, cover_edges=False, optimizer=None):
    """``adapt.adapt_granule`` at ratio ``hr / window``: ``steps`` optimisation steps of the masked loss on the active tiles of one
    gappy granule (raw LST (h,w) [K], raw NDVI (h p/q, w p/q), ``mask`` as in ``gaps.fill_gaps``), BatchNorm statistics frozen.
    The layout is ``ratio.geometry``'s; fill, selection and loss targets are ``gaps.fill_gaps``, ``gaps.select_tiles`` and
    ``adapt.tile_targets`` (they see the LST raster only), the network inputs ``ratio.prepare_active_tiles``; step i is
    ``rloss.train_step(..., factor=hr / window, valid=)`` on the min(batch, n_active) tiles from position i * batch of the active
    list, cyclic.  A ``(window, hr)`` whose ``sensor.lr_shape(hr, hr, hr / window)`` is not ``(window, window)`` -- (16, 20): the
    sensor model's crop leaves 17 -- is refused before any launch.  The read of the active count is the only host synchronisation;
    no active tile: no step, no forward.  Returns an ``adapt.Adaptation``; the model's mode and ``bn_frozen`` are as they were.

    Keyword-only ``graphed=True`` (``_granule.keyword_options``; default False: the loop above, bit for bit): after the read of the
    active count the step is an ``rloss.GraphedTrainStep(masked=True)`` for min(batch, n_active) tiles -- three eager steps, the
    fourth captures, the rest replay; with no optimizer given the loop makes ``FlatAdam(lr=lr, capturable=True)``, and one that is
    given must be capturable (ValueError before any launch)."""
