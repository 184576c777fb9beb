#!/usr/bin/env python3
"""Time the differentiable sensor model at any ratio (include/sifsr_sensor.h).

    python tools/time_sensor.py [--windows 9] [--reps 5] [--warmup 3] [--batch 64] [--no-step] [--out FILE.json]

Every figure is the median (with minimum and maximum) over `windows` windows of `reps` back-to-back calls between two HIP events on
the current stream, the stream synchronised before and after each window, after `warmup` calls of every variant of the shape; the
variants of one shape ALTERNATE window by window inside the one process, so that clock and cache state are shared.  Profiler off;
kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/time_sensor.py ...` run.

Per shape -- (64,1,192,192) at factor 3 and (64,1,256,256) at factor 4, both cropped as the loss uses them, and one 700 x 830 scene at
926.25 / 90 --:
  sifsr_fwd       `degrade.degrade`: the forward of the same shape, with its allocations
  sifsr_bwd       `sifsrt_degrade_bwd` with the allocations `sensor.downscale`'s backward makes (workspace and dx)
  sifsr_fwd_bwd   `sensor.downscale` then `torch.autograd.grad`
  torch_fwd / torch_fwd_bwd   the reference's composition on the same device under torch autograd: F.pad(reflect), F.conv2d with the
                  (2 hw + 1)^2 fp32 kernel and padding="same", F.interpolate(scale_factor=1/factor, mode="bicubic"), the crop
  div4_fwd_bwd / div4_bwd     at factor 4: `sifsr.downscale_LST_SR_to_LR` and `sifsr_gauss9_decimate4_bwd`, the fused /4 kernels
  lowpass_fwd_bwd / torch_lowpass_fwd_bwd   `sensor.lowpass` at mtf 0.25 and the reference's pad / conv2d / crop
and one optimisation step at `--batch` patches of HR 192: `sensor.train_step` at factor 3 (LR 64) beside the ordinary x4
`train.train_step` (LR 48).  No ratio is asserted.  Nothing is fetched; inputs are seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternating(variants, windows, reps, warmup):
    """variants {name: fn} -> {name: {median_ms, min_ms, max_ms}} per call"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(windows):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / reps)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "windows": windows, "reps": reps}
            for k, v in ms.items()}


def torch_blur(x, factor, mtf):
    from dropin.utils import generate_psf_kernel
    k = torch.from_numpy(generate_psf_kernel(1.0, factor, mtf, None)).to(x.device)
    hw = (k.shape[-1] - 1) // 2
    return F.conv2d(F.pad(x, (hw, hw, hw, hw), mode="reflect"), k[None, None], padding="same"), hw


def torch_downscale(x, factor, mtf=0.1, crop=True):
    """utils.py:1671-1706 (crop) / :1759-1830 (no crop) on a (B,1,H,W) device tensor"""
    x, hw = torch_blur(x, factor, mtf)
    x = F.interpolate(x, scale_factor=1 / factor, mode="bicubic")
    c = int(hw / factor) if crop else 0
    return x[:, :, c:x.shape[-2] - c, c:x.shape[-1] - c]


def torch_lowpass(x, factor, mtf=0.25):
    x, hw = torch_blur(x, factor, mtf)
    return x[:, :, hw:x.shape[-2] - hw, hw:x.shape[-1] - hw]


def shape_variants(sifsr, shape, factor, crop):
    from sifsr import _lib, degrade, sensor
    B, _, H, W = shape
    x = (300.0 + 5.0 * torch.randn(shape, device="cuda")).requires_grad_(True)
    oh, ow = degrade.output_shape(H, W, factor, None, crop)
    d = torch.randn((B, 1, oh, ow), device="cuda")
    dl = torch.randn(shape, device="cuda")
    xd = x.detach()

    def bwd():
        need = _lib.call("sifsrt_degrade_bwd_workspace_bytes", B, H, W, float(factor), 0, int(crop))
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        dx = torch.empty(shape, device="cuda")
        _lib.call("sifsrt_degrade_bwd", d, None, dx, ws, need, B, H, W, float(factor), 0.1, 0, int(crop), _lib.stream_ptr(x.device))
        return dx

    v = {"sifsr_fwd": lambda: degrade.degrade(xd, factor, crop=crop),
         "sifsr_bwd": bwd,
         "sifsr_fwd_bwd": lambda: torch.autograd.grad(sensor.downscale(x, factor, crop=crop), x, d),
         "torch_fwd": lambda: torch_downscale(xd, factor, crop=crop),
         "torch_fwd_bwd": lambda: torch.autograd.grad(torch_downscale(x, factor, crop=crop), x, d),
         "lowpass_fwd_bwd": lambda: torch.autograd.grad(sensor.lowpass(x, factor, 0.25), x, dl),
         "torch_lowpass_fwd_bwd": lambda: torch.autograd.grad(torch_lowpass(x, factor), x, dl)}
    if factor == 4 and crop:
        taps = sifsr.sif_ops._taps_c(0.1, 4, None)

        def div4_bwd():
            gx = torch.empty(shape, device="cuda")
            _lib.call("sifsr_gauss9_decimate4_bwd", d, taps, gx, B, H, W, _lib.stream_ptr(x.device))
            return gx

        v["div4_fwd_bwd"] = lambda: torch.autograd.grad(sifsr.downscale_LST_SR_to_LR(x), x, d)
        v["div4_bwd"] = div4_bwd
    check = {"fwd_max_abs_K": float((degrade.degrade(xd, factor, crop=crop) - torch_downscale(xd, factor, crop=crop)).abs().max()),
             "bwd_max_abs": float((v["sifsr_fwd_bwd"]()[0] - v["torch_fwd_bwd"]()[0]).abs().max())}
    return v, check


def step_variants(sifsr, batch, hr=192):
    from sifsr import sensor, train
    stats = {"mean_lst": 300.0, "std_lst": 10.0}
    out = {}
    for name, factor in (("sensor_step_x3", 3.0), ("train_step_x4", 4.0)):
        torch.manual_seed(0)
        m = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda()
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-4)
        h, w = sensor.lr_shape(hr, hr, factor)
        lst = torch.randn((batch, 1, h, w), device="cuda")
        up = F.interpolate(lst, size=(hr, hr), mode="bicubic", align_corners=False).contiguous()
        ndvi = torch.randn((batch, 1, hr, hr), device="cuda")
        if factor == 3.0:
            out[name] = lambda m=m, opt=opt, lst=lst, up=up, ndvi=ndvi: sensor.train_step(m, opt, lst, up, ndvi, stats, 0.5, 1.0, 3.0)
        else:
            out[name] = lambda m=m, opt=opt, lst=lst, up=up, ndvi=ndvi: train.train_step(m, opt, lst, up, ndvi, stats, 0.5, 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_sensor.py needs a ROCm GPU"
    import sifsr
    from sifsr import degrade
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for tag, shape, factor, crop in ((f"{args.batch}x1x192x192 factor 3", (args.batch, 1, 192, 192), 3.0, True),
                                     (f"{args.batch}x1x256x256 factor 4", (args.batch, 1, 256, 256), 4.0, True),
                                     ("1x1x700x830 factor 926.25/90", (1, 1, 700, 830), degrade.COARSE_FACTOR, False)):
        variants, check = shape_variants(sifsr, shape, factor, crop)
        result["shapes"][tag] = {"against_torch": check, "per_call": alternating(variants, args.windows, args.reps, args.warmup)}
    if not args.no_step:
        result["step"] = {"batch": args.batch, "hr": 192, "per_call": alternating(step_variants(sifsr, args.batch), args.windows, args.reps, args.warmup)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
