"""On-device train-time metrics: ``us.psnr_skimage`` / ``us.ssim_skimage`` (utils.py:548-578)
without the per-batch ``.detach().cpu().numpy()`` + scikit-image host stall of train_model_B_gradFTM.py:126-127.

Semantics follow scikit-image 0.22 (the reference's pinned version, environment.yml:402) as the reference calls
it: ``data_range = targets.max() - targets.min()`` over the WHOLE target batch, ``structural_similarity`` defaults
(7x7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, mean over the window-valid interior),
``peak_signal_noise_ratio = 10 log10(range^2 / mse)``, then the mean over the batch.  scikit-image is not
installed in the build container: the oracle is a numpy/scipy restatement of that published algorithm and the
parity with scikit-image itself is *unpinned*.

``aster_metrics`` / ``gradient_strata`` (f5): the per-pair evaluation table of model_perf_aster_formatds.py:371-437 (PSNR,
SSIM, RMSE, the three gradient-stratum RMSEs, GSSIM of utils.py:1904-2005, RMSE_grad), one (B,8) float64 row per pair.

``masked_aster_metrics`` / ``masked_psnr_ssim`` (f10): both for rasters with gaps -- a term is counted iff every pixel its stencil
reads is valid.  ``aster_metrics`` and ``psnr_ssim`` are what they were.
"""
from __future__ import annotations

import torch

from . import _lib
from .sif_ops import _taps_c


def psnr_ssim(predictions, targets):
    """(B,1,H,W) x2 -> (psnr, ssim) as 0-d device tensors (batch means); no host synchronisation."""
    _lib.require_gpu(predictions, "predictions"); _lib.require_gpu(targets, "targets")
    if predictions.shape != targets.shape or predictions.dim() != 4 or predictions.shape[1] != 1:
        raise _lib.SifsrError("psnr_ssim expects two (B,1,H,W) tensors")
    B, _, H, W = predictions.shape
    nbytes = _lib.call("sifsr_psnr_ssim_scratch_bytes", B, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=predictions.device)
    out = torch.empty(2, dtype=torch.float32, device=predictions.device)
    _lib.call("sifsr_psnr_ssim", predictions.detach(), targets.detach(), B, H, W, scratch, nbytes, out,
              _lib.stream_ptr(predictions.device))
    return out[0], out[1]


def psnr_skimage(predictions, targets):
    """Drop-in for us.psnr_skimage on device tensors (returns a 0-d device tensor; call .item() when needed)."""
    return psnr_ssim(predictions, targets)[0]


def ssim_skimage(predictions, targets):
    """Drop-in for us.ssim_skimage on device tensors (returns a 0-d device tensor)."""
    return psnr_ssim(predictions, targets)[1]


# ---- per-pair ASTER evaluation table, model_perf_aster_formatds.py:371-437 ----------------------------
# The column names of :507 without 'LPIPS' (that column: aster_table / METRIC_NAMES_WITH_LPIPS below, sifsr.lpips).
METRIC_NAMES = ("PSNR", "SSIM", "RMSE", "RMSE (low grad per image)", "RMSE (mean grad per image)",
                "RMSE (high grad per image)", "GSSIM", "RMSE_grad")


def _check_pairs(reference, prediction):
    _lib.require_gpu(reference, "reference"); _lib.require_gpu(prediction, "prediction")
    if reference.shape != prediction.shape or reference.dim() != 4 or reference.shape[1] != 1:
        raise _lib.SifsrError("aster_metrics expects two (B,1,H,W) tensors of the same shape")
    B, _, H, W = reference.shape
    if H < 16 or W < 16:
        raise _lib.SifsrError(f"aster_metrics needs H, W >= 16, got {H}x{W}")
    return B, H, W


def aster_metrics(reference, prediction, data_range=None):
    """Per-pair evaluation metrics, columns ``METRIC_NAMES``, of model_perf_aster_formatds.py:371-437 on the device.

    reference (ASTER, overlap_11) and prediction (overlap_22): (B,1,H,W) float32 device tensors, H, W >= 16 -> (B,8) float64
    device tensor; no host synchronisation.  Or two lists of (H,W) / (1,H,W) / (1,1,H,W) device tensors of mixed sizes:
    pairs of one shape run as one batch, rows come back in list order.

    data_range None: per pair, R = max(a u b) - min(a u b) in float32 (:373-374), as the evaluation passes it to PSNR, SSIM
    and GSSIM.  The strata RMSEs (:379-404) divide by N, not by the stratum size: the reference's
    ``filter((0.0).__ne__, ...)`` runs on np.float32 elements, for which ``float.__ne__`` returns NotImplemented (truthy),
    so nothing is filtered and the zeroed entries stay in the mean.
    """
    if isinstance(reference, (list, tuple)):
        return _aster_metrics_list(reference, prediction, data_range)
    B, H, W = _check_pairs(reference, prediction)
    nbytes = _lib.call("sifsr_eval_metrics_scratch_bytes", B, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=reference.device)
    out = torch.empty(B, 8, dtype=torch.float64, device=reference.device)
    _lib.call("sifsr_eval_metrics", reference.detach(), prediction.detach(), B, H, W, _taps_c(0.1, 4, None),
              -1.0 if data_range is None else float(data_range), scratch, nbytes, out, _lib.stream_ptr(reference.device))
    return out


def _as_hw(t, what):
    if not isinstance(t, torch.Tensor):
        raise _lib.SifsrError(f"{what} must be a device tensor")
    if t.dim() > 2 and all(s == 1 for s in t.shape[:-2]):
        t = t.reshape(t.shape[-2:])
    if t.dim() != 2:
        raise _lib.SifsrError(f"{what}: expected an (H,W), (1,H,W) or (1,1,H,W) image, got {tuple(t.shape)}")
    return t


def _aster_metrics_list(references, predictions, data_range):
    if len(references) != len(predictions) or not references:
        raise _lib.SifsrError("aster_metrics: two non-empty lists of the same length expected")
    refs = [_as_hw(r, "reference") for r in references]
    preds = [_as_hw(p, "prediction") for p in predictions]
    groups = {}
    for i, (r, p) in enumerate(zip(refs, preds)):
        if r.shape != p.shape:
            raise _lib.SifsrError(f"pair {i}: reference {tuple(r.shape)} and prediction {tuple(p.shape)} differ")
        groups.setdefault(tuple(r.shape), []).append(i)
    out = torch.empty(len(refs), 8, dtype=torch.float64, device=refs[0].device)
    for idx in groups.values():
        rows = aster_metrics(torch.stack([refs[i] for i in idx])[:, None], torch.stack([preds[i] for i in idx])[:, None],
                             data_range)
        out[torch.tensor(idx, device=out.device)] = rows
    return out


def gradient_strata(reference):
    """The gradient strata of model_perf_aster_formatds.py:379-404 alone, (B,1,H,W) float32 device tensor ->
    (g (B,1,H,W) = |ref - get_output_ftm(ref)|, q25 (B,), q75 (B,) = np.percentile(g, 25 / 75) per image (numpy 2.x 'linear'
    in float32, exact order statistics), counts (B,3) int32 = #(g < q25), #(q25 <= g <= q75), #(g >= q75))."""
    B, H, W = _check_pairs(reference, reference)
    g = torch.empty_like(reference)
    q = torch.empty(B, 2, dtype=torch.float32, device=reference.device)
    counts = torch.empty(B, 3, dtype=torch.int32, device=reference.device)
    _lib.call("sifsr_gradient_strata", reference.detach(), B, H, W, _taps_c(0.1, 4, None), g, q, counts,
              _lib.stream_ptr(reference.device))
    return g, q[:, 0], q[:, 1], counts


# ---- the nine-column table (include/sifsr_lpips.h) ------------------------------------------------------------
# The column names of model_perf_aster_formatds.py:507, in its order.
METRIC_NAMES_WITH_LPIPS = METRIC_NAMES[:7] + ("LPIPS",) + METRIC_NAMES[7:]


def aster_table(reference, prediction, lpips, data_range=None):
    """The reference's per-pair table with all nine columns ``METRIC_NAMES_WITH_LPIPS`` -> (B,9) float64 device tensor.

    ``lpips``: a ``sifsr.lpips.LPIPS`` (it carries the weights the caller supplied); the column is its ``pairs`` path, the pair
    min/max-normalised to [0, 1] and repeated to three channels (model_perf_aster_formatds.py:373-374, :405-410).  The other eight
    columns are ``aster_metrics(reference, prediction, data_range)`` bit for bit; tensors or lists as it takes them."""
    rows = aster_metrics(reference, prediction, data_range)
    if isinstance(reference, (list, tuple)):
        lp = lpips.pairs(list(reference), list(prediction))
    else:
        lp = lpips.pairs(reference, prediction)
    return torch.cat((rows[:, :7], lp[:, 5:6], rows[:, 7:]), dim=1)


# ---- scoring rasters with gaps (include/sifsr_scores.h) ------------------------------------------------------
COUNT_NAMES = ("n0 (valid pixels)", "n1 (3x3 all valid)", "n3 (7x7 all valid)", "n4 (9x9 all valid)", "ns (image-clipped 9x9 all valid)")


def _check_valid(valid, shape, what):
    if not isinstance(valid, torch.Tensor) or not valid.is_cuda or valid.dtype not in (torch.uint8, torch.bool):
        raise _lib.SifsrError(f"{what} must be a uint8 or bool device tensor")
    if valid.dim() == len(shape) + 1 and valid.shape[1] == 1:
        valid = valid[:, 0]
    if tuple(valid.shape) != tuple(shape):
        raise _lib.SifsrError(f"{what}: expected shape {tuple(shape)}, got {tuple(valid.shape)}")
    return (valid.to(torch.uint8) if valid.dtype == torch.bool else valid).contiguous()


def _masked_eval(reference, prediction, valid, data_range):
    B, H, W = _check_pairs(reference, prediction)
    if valid is not None:
        valid = _check_valid(valid, (B, H, W), "valid")
    nbytes = _lib.call("sifsrv_eval_metrics_scratch_bytes", B, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=reference.device)
    out = torch.empty(B, 8, dtype=torch.float64, device=reference.device)
    counts = torch.empty(B, 5, dtype=torch.int32, device=reference.device)
    _lib.call("sifsrv_eval_metrics", reference.detach(), prediction.detach(), valid, B, H, W, _taps_c(0.1, 4, None),
              -1.0 if data_range is None else float(data_range), scratch, nbytes, out, counts, _lib.stream_ptr(reference.device))
    return out, counts, scratch


def masked_aster_metrics(reference, prediction, valid=None, data_range=None, return_counts=False):
    """``aster_metrics`` for rasters with gaps: a term is counted iff every pixel its stencil reads is valid, and each mean
    divides by the number of terms counted (include/sifsr_scores.h).

    A pixel is valid iff both images are finite and non-zero there (NaN and 0 K are the project's no-data values) and ``valid``
    -- a uint8 / bool device tensor (B,H,W) or (B,1,H,W), any non-zero byte = usable, or None -- allows it.  PSNR / RMSE run
    over the valid pixels, RMSE_grad over the pixels with an all-valid 3x3 neighbourhood, SSIM 7x7, GSSIM 9x9, the strata RMSEs
    over the pixels whose 9x9 PSF window, clipped to the image, is all valid; ``data_range`` None: max - min over the valid
    pixels of both images.  A column without a term is NaN.  What an invalid pixel holds changes no output bit, and with every
    pixel valid the rows are ``aster_metrics``'s bit for bit.

    Tensors or lists of mixed sizes as ``aster_metrics`` takes them (``valid`` then a list as well, or None).
    ``return_counts``: also the (B,5) int32 counts ``COUNT_NAMES``.  No host synchronisation."""
    if isinstance(reference, (list, tuple)):
        return _masked_aster_metrics_list(reference, prediction, valid, data_range, return_counts)
    out, counts, _ = _masked_eval(reference, prediction, valid, data_range)
    return (out, counts) if return_counts else out


def _masked_aster_metrics_list(references, predictions, valid, data_range, return_counts):
    if len(references) != len(predictions) or not references or (valid is not None and len(valid) != len(references)):
        raise _lib.SifsrError("masked_aster_metrics: non-empty lists of the same length expected")
    refs = [_as_hw(r, "reference") for r in references]
    preds = [_as_hw(p, "prediction") for p in predictions]
    masks = None if valid is None else [_as_hw(v, "valid") for v in valid]
    groups = {}
    for i, (r, p) in enumerate(zip(refs, preds)):
        if r.shape != p.shape or (masks is not None and masks[i].shape != r.shape):
            raise _lib.SifsrError(f"pair {i}: reference {tuple(r.shape)}, prediction {tuple(p.shape)} and valid differ in shape")
        groups.setdefault(tuple(r.shape), []).append(i)
    out = torch.empty(len(refs), 8, dtype=torch.float64, device=refs[0].device)
    counts = torch.empty(len(refs), 5, dtype=torch.int32, device=refs[0].device)
    for idx in groups.values():
        v = None if masks is None else torch.stack([masks[i].to(torch.uint8) for i in idx])
        rows, cnt = masked_aster_metrics(torch.stack([refs[i] for i in idx])[:, None], torch.stack([preds[i] for i in idx])[:, None],
                                         v, data_range, True)
        where = torch.tensor(idx, device=out.device)
        out[where], counts[where] = rows, cnt
    return (out, counts) if return_counts else out


def masked_gradient_strata(reference, prediction, valid=None):
    """The strata of ``masked_aster_metrics`` alone: (g (B,1,H,W) = |ref - get_output_ftm(ref)| with NaN at every pixel outside
    the strata set, q25 (B,), q75 (B,) = np.percentile of the eligible g per image ('linear', float32), counts (B,5))."""
    out, counts, scratch = _masked_eval(reference, prediction, valid, None)
    B, _, H, W = reference.shape
    n = B * H * W * 4
    g = scratch[:n].view(torch.float32).view(B, 1, H, W).clone()
    rq = scratch[(n + 255) // 256 * 256:][:B * 16].view(torch.float32).view(B, 4)
    return g, rq[:, 1].clone(), rq[:, 2].clone(), counts


def masked_psnr_ssim(predictions, targets, valid, return_counts=False):
    """``psnr_ssim`` over the valid pixels of a masked batch (include/sifsr_scores.h): (B,1,H,W) x2 and ``valid``, a uint8 / bool
    device tensor (B,1,h,w) or (B,h,w) with (h,w) = (H,W) or (H/4,W/4) -- the LR mask of ``MinedPatches.masked_loader`` -- ->
    (psnr, ssim) as 0-d device tensors.  data_range = max - min of the valid target pixels of the batch; per image PSNR over the
    valid pixels and SSIM over the pixels whose 7x7 window is all valid; the means run over the images that contribute, NaN
    where none does.  ``return_counts``: also the (2,) int32 numbers of contributing images.  No host synchronisation; with
    every byte valid the pair is ``psnr_ssim``'s bit for bit."""
    _lib.require_gpu(predictions, "predictions"); _lib.require_gpu(targets, "targets")
    if predictions.shape != targets.shape or predictions.dim() != 4 or predictions.shape[1] != 1:
        raise _lib.SifsrError("masked_psnr_ssim expects two (B,1,H,W) tensors")
    B, _, H, W = predictions.shape
    if not isinstance(valid, torch.Tensor) or valid.dim() not in (3, 4):
        raise _lib.SifsrError("valid must be a (B,1,h,w) or (B,h,w) uint8 or bool device tensor")
    h, w = valid.shape[-2:]
    if (h, w) == (H, W):
        scale = 1
    elif (4 * h, 4 * w) == (H, W):
        scale = 4
    else:
        raise _lib.SifsrError(f"valid {tuple(valid.shape)} is neither the mask of the {H}x{W} images nor of their 4x4 cells")
    valid = _check_valid(valid, (B, h, w), "valid")
    nbytes = _lib.call("sifsrv_psnr_ssim_scratch_bytes", B, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=predictions.device)
    out = torch.empty(2, dtype=torch.float32, device=predictions.device)
    counts = torch.empty(2, dtype=torch.int32, device=predictions.device)
    _lib.call("sifsrv_psnr_ssim", predictions.detach(), targets.detach(), valid, scale, B, H, W, scratch, nbytes, out, counts,
              _lib.stream_ptr(predictions.device))
    return (out[0], out[1], counts) if return_counts else (out[0], out[1])
