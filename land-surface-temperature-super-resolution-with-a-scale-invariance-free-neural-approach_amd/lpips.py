"""LPIPS-VGG16 on the device (include/sifsr_lpips.h): the ninth column of the per-pair ASTER table.

The reference's metric is the ``piq`` variant vendored in lpips.py:226-292, :351-358, called at model_perf_aster_formatds.py:134
with ``distance='mse'``, ``reduction='mean'``, ``mean=[0,0,0]``, ``std=[1,1,1]``: VGG16 ``features`` up to relu5_3, five taps,
unit-normalised in the channel direction, squared differences weighted by the learned linear weights, averaged over space.

The reference downloads both weight files.  Nothing is fetched here, ever: the caller supplies them --

    vgg16_weights   torchvision's ``vgg16`` state dict (keys ``features.0.weight`` ...) or that of its ``features`` alone
                    (``0.weight`` ...), or a path ``torch.load`` can read; normally ``vgg16-397923af.pth`` from
                    ``~/.cache/torch/hub/checkpoints/`` of a machine that has run the reference's evaluation;
    lpips_weights   piq's list of five ``(1, C, 1, 1)`` tensors (C = 64, 128, 256, 512, 512), or a path; normally
                    ``lpips_weights.pt`` from the same directory (release v0.4.0 of photosynthesis-team/photosynthesis.metrics).
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib

IMAGENET_MEAN = [0.485, 0.456, 0.406]     # lpips.py:133-134
IMAGENET_STD = [0.229, 0.224, 0.225]
CONV_MODULES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)           # torchvision vgg16().features indices of the convs
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
TAP_MODULES = (3, 8, 15, 22, 29)                                           # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
TAP_CHANNELS = (64, 128, 256, 512, 512)
LAYER_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3", "LPIPS")
N_VGG_PARAMS = sum(9 * ci * co + co for ci, co in CONV_CHANNELS)           # 14,714,688
N_LIN = sum(TAP_CHANNELS)                                                  # 1472
WORKSPACE_CAP = 2 << 30       # bytes of workspace one call may take; larger batches are chunked (rows do not depend on the chunking)

_WHERE = ("Nothing is downloaded by this package.  The VGG16 weights are torchvision's `vgg16-397923af.pth` and the linear weights piq's "
          "`lpips_weights.pt` (photosynthesis-team/photosynthesis.metrics release v0.4.0); a machine that has run the reference's "
          "evaluation holds both under ~/.cache/torch/hub/checkpoints/.  Pass state dicts or paths (drop-in: the environment "
          "variables SIFSR_VGG16_WEIGHTS and SIFSR_LPIPS_WEIGHTS).")


def _load(obj, what):
    if obj is None:
        raise _lib.SifsrError(f"LPIPS: no {what} given.  {_WHERE}")
    if isinstance(obj, (str, os.PathLike)):
        if not os.path.isfile(obj):
            raise _lib.SifsrError(f"LPIPS: {what} file {os.fspath(obj)!r} not found.  {_WHERE}")
        obj = torch.load(obj, map_location="cpu")
    return obj


def flatten_vgg16(weights) -> torch.Tensor:
    """state dict (``features.N.weight`` or ``N.weight`` keys) -> the 13 (weight OIHW, bias) pairs, flat fp32, in module order"""
    sd = _load(weights, "VGG16 weights")
    if not isinstance(sd, dict):
        raise _lib.SifsrError(f"LPIPS: the VGG16 weights must be a state dict, got {type(sd).__name__}")
    parts = []
    for m, (ci, co) in zip(CONV_MODULES, CONV_CHANNELS):
        for kind, shape in (("weight", (co, ci, 3, 3)), ("bias", (co,))):
            t = sd.get(f"features.{m}.{kind}", sd.get(f"{m}.{kind}"))
            if t is None:
                raise _lib.SifsrError(f"LPIPS: the VGG16 state dict has neither 'features.{m}.{kind}' nor '{m}.{kind}'.  {_WHERE}")
            if tuple(t.shape) != shape:
                raise _lib.SifsrError(f"LPIPS: VGG16 {m}.{kind} has shape {tuple(t.shape)}, expected {shape}")
            parts.append(t.detach().to("cpu", torch.float32).reshape(-1))
    flat = torch.cat(parts)
    assert flat.numel() == N_VGG_PARAMS
    return flat


def flatten_lin(weights) -> torch.Tensor:
    """piq's list of five (1,C,1,1) tensors (or one flat tensor of 1472) -> flat fp32"""
    w = _load(weights, "LPIPS linear weights")
    if isinstance(w, torch.Tensor):
        w = list(torch.split(w.reshape(-1), list(TAP_CHANNELS))) if w.numel() == N_LIN else [w]
    if not isinstance(w, (list, tuple)) or len(w) != 5:
        raise _lib.SifsrError("LPIPS: the linear weights must be five tensors, one per tap (64, 128, 256, 512, 512 channels)")
    parts = []
    for t, c in zip(w, TAP_CHANNELS):
        t = torch.as_tensor(t)
        if t.numel() != c:
            raise _lib.SifsrError(f"LPIPS: a linear weight has {t.numel()} elements, expected {c}")
        parts.append(t.detach().to("cpu", torch.float32).reshape(-1))
    return torch.cat(parts)


def _c3(v, what):
    v = [float(f) for f in v]
    if len(v) != 3:
        raise _lib.SifsrError(f"LPIPS: {what} must have three entries")
    return (ctypes.c_float * 3)(*v)


def max_pairs(H: int, W: int) -> int:
    """pairs of H x W images one C-ABI call takes: below the 4 GiB limit of the convolution's buffer addressing and WORKSPACE_CAP"""
    hard = ((1 << 32) - 4096 - 1) // (2 * H * W * 64 * 4)
    soft = max(1, WORKSPACE_CAP // (3 * 2 * H * W * 64 * 4))
    return min(hard, soft)


class LPIPS:
    """LPIPS-VGG16 of lpips.py:313-358 with weights supplied by the caller (see the module docstring).

    ``__call__(x, y)``: (N,3,H,W) float32 device tensors, nominally in [0, 1] -> the LPIPS reduced over N ('mean', 'sum') or (N,)
    ('none'), float64, on the device.  ``layers(x, y)`` -> (N,6): the five layer terms and their sum.  ``pairs(a, b)``: the table
    path for one-channel rasters (N,1,H,W) / (N,H,W), min/max-normalised per pair on the device, mean 0 / std 1 -> (N,6).
    Each also takes two lists of images of mixed sizes (rows in list order).  H, W >= 16.  A pair with a non-finite pixel (or, in
    ``pairs``, a constant pair) gives a NaN row.  No host synchronisation."""

    def __init__(self, vgg16_weights, lpips_weights, mean=IMAGENET_MEAN, std=IMAGENET_STD, reduction="mean"):
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"LPIPS: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
        self.reduction = reduction
        self.mean, self.std = _c3(mean, "mean"), _c3(std, "std")
        self._vgg = flatten_vgg16(vgg16_weights)
        self._lin = flatten_lin(lpips_weights)
        self._packed = {}

    def packed(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.SifsrError(f"LPIPS runs on a ROCm GPU (gfx950) only, got device {device}; there is no CPU path.")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._packed:
            n = _lib.call("sifsrl_pack_floats")
            packed = torch.empty(n, dtype=torch.float32, device=device)
            vgg, lin = self._vgg.to(device), self._lin.to(device)
            _lib.call("sifsrl_pack", vgg, lin, packed, _lib.stream_ptr(device))
            self._packed[key] = packed
        return self._packed[key]

    # ---- one shape -------------------------------------------------------------------------------------------------------------
    def _run(self, x, y, pairs):
        _lib.require_gpu(x, "x"); _lib.require_gpu(y, "y")
        if pairs:
            if x.dim() == 4 and x.shape[1] == 1:
                x = x[:, 0]
            if y.dim() == 4 and y.shape[1] == 1:
                y = y[:, 0]
            ok = x.dim() == 3 and x.shape == y.shape
        else:
            ok = x.dim() == 4 and x.shape[1] == 3 and x.shape == y.shape
        if not ok:
            raise _lib.SifsrError("LPIPS expects two (N,3,H,W) tensors of the same shape" if not pairs
                                  else "LPIPS.pairs expects two (N,1,H,W) or (N,H,W) tensors of the same shape")
        N, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        if N < 1 or H < 16 or W < 16:
            raise _lib.SifsrError(f"LPIPS needs N >= 1 and H, W >= 16 (relu5_3 would be empty), got N = {N}, {H}x{W}")
        chunk = max_pairs(H, W)
        if chunk < 1:
            raise _lib.SifsrError(f"LPIPS: one pair of {H}x{W} images exceeds the 4 GiB limit of the convolution's buffer addressing")
        x, y = x.detach().contiguous(), y.detach().contiguous()
        packed = self.packed(x.device)
        out = torch.empty(N, 6, dtype=torch.float64, device=x.device)
        n0 = min(N, chunk)
        nbytes = _lib.call("sifsrl_workspace_bytes", n0, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        for i in range(0, N, chunk):
            n = min(chunk, N - i)
            if pairs:
                _lib.call("sifsrl_lpips_pairs", x[i:i + n], y[i:i + n], n, H, W, packed, ws, nbytes, out[i:i + n], _lib.stream_ptr(x.device))
            else:
                _lib.call("sifsrl_lpips", x[i:i + n], y[i:i + n], n, H, W, self.mean, self.std, packed, ws, nbytes, out[i:i + n],
                          _lib.stream_ptr(x.device))
        return out

    # ---- lists of mixed sizes --------------------------------------------------------------------------------------------------
    def _run_list(self, xs, ys, pairs):
        if not isinstance(ys, (list, tuple)) or len(xs) != len(ys) or not xs:
            raise _lib.SifsrError("LPIPS: two non-empty lists of the same length expected")
        nd = 2 if pairs else 3

        def img(t, what):
            if not isinstance(t, torch.Tensor):
                raise _lib.SifsrError(f"{what} must be a device tensor")
            while t.dim() > nd and t.shape[0] == 1:
                t = t[0]
            if t.dim() != nd or (not pairs and t.shape[0] != 3):
                raise _lib.SifsrError(f"{what}: expected {'an (H,W) / (1,H,W)' if pairs else 'a (3,H,W) / (1,3,H,W)'} image, got {tuple(t.shape)}")
            return t
        xs, ys = [img(t, "x") for t in xs], [img(t, "y") for t in ys]
        groups = {}
        for i, (a, b) in enumerate(zip(xs, ys)):
            if a.shape != b.shape:
                raise _lib.SifsrError(f"pair {i}: {tuple(a.shape)} and {tuple(b.shape)} differ")
            groups.setdefault(tuple(a.shape), []).append(i)
        out = torch.empty(len(xs), 6, dtype=torch.float64, device=xs[0].device)
        for idx in groups.values():
            rows = self._run(torch.stack([xs[i] for i in idx]), torch.stack([ys[i] for i in idx]), pairs)
            for k, i in enumerate(idx):             # (device-to-device row copies: an index tensor would be a host-to-device copy)
                out[i].copy_(rows[k])
        return out

    def layers(self, x, y):
        """-> (N,6) float64 device tensor, columns ``LAYER_NAMES``"""
        return self._run_list(x, y, False) if isinstance(x, (list, tuple)) else self._run(x, y, False)

    def pairs(self, a, b):
        """the table path (model_perf_aster_formatds.py:373-374, :407-408) -> (N,6) float64 device tensor"""
        return self._run_list(a, b, True) if isinstance(a, (list, tuple)) else self._run(a, b, True)

    def _reduce(self, v):
        return v if self.reduction == "none" else (v.mean(dim=0) if self.reduction == "mean" else v.sum(dim=0))

    def __call__(self, x, y):
        return self._reduce(self.layers(x, y)[:, 5])
