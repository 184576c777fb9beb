#!/usr/bin/env python3
"""Time the fused, masked SIF loss at any ratio (include/sifsr_rloss.h) beside the composed path.

    python tools/time_rloss.py [--windows 9] [--reps 5] [--warmup 3] [--batch 64] [--only HR] [--no-step] [--out FILE.json]

Every figure is the median (with minimum and maximum) over `windows` windows of `reps` back-to-back calls between two HIP events on
the current stream, the stream synchronised before and after each window, after `warmup` calls of every variant of the shape; the
variants of one shape ALTERNATE window by window inside the one process, so that clock and cache state are shared.  Profiler off;
kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/time_rloss.py --only 192 --no-step` run (one
shape per run: the statistics are per kernel name).

Per shape -- (B,1,192,192) at factor 3, (B,1,160,160) at factor 2.5 and (B,1,256,256) at factor 4 --, forward plus backward of the
'sr2' loss on the same tensors:
  composed        `sensor.sif_loss(...)[2].backward()`: the yardstick, the parent's path
  fused           `rloss.sif_loss(...)[2].backward()`, all valid (no mask)
  fused_masked    the same with 35 % of the LR cells invalid and their counts given (`counts=valid_counts(valid, (H, W))`, formed once)
  fused_masked_counted   ... with `counts=None`: the two launches of `valid_counts` inside every call
  fused_call      `rloss.sif_loss_with_grad` alone (no autograd node), all valid
  div4_masked     at factor 4: `sifsr.masked_sif_loss_with_grad`, the fused /4 kernels, all valid
and one optimisation step at `--batch` patches of HR 192 at factor 3: `rloss.train_step` beside `sensor.train_step`.  No ratio is
asserted.  Nothing is fetched; inputs are seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_sensor import alternating  # noqa: E402

MEAN, STD, ALPHA, GAMMA = 307.2378, 5.5698, 0.5, -0.25


def loss_variants(sifsr, shape, factor):
    from sifsr import rloss, sensor
    B, _, H, W = shape
    h, w = sensor.lr_shape(H, W, factor)
    sr = (1.3 * torch.randn(shape, device="cuda")).requires_grad_(True)
    lst, ndvi = torch.randn((B, 1, h, w), device="cuda"), torch.randn(shape, device="cuda").clamp(-3, 3)
    valid = (torch.rand((B, 1, h, w), device="cuda") > 0.35).to(torch.uint8)
    counts = rloss.valid_counts(valid, (H, W))

    def backward(loss_fn):
        def run():
            sr.grad = None
            loss_fn()[2].backward()
            return sr.grad
        return run

    v = {"composed": backward(lambda: sensor.sif_loss("sr2", sr, lst, ndvi, factor, MEAN, STD, ALPHA, GAMMA)),
         "fused": backward(lambda: rloss.sif_loss("sr2", sr, lst, ndvi, factor, MEAN, STD, ALPHA, GAMMA)),
         "fused_masked": backward(lambda: rloss.sif_loss("sr2", sr, lst, ndvi, factor, MEAN, STD, ALPHA, GAMMA, valid=valid, counts=counts)),
         "fused_masked_counted": backward(lambda: rloss.sif_loss("sr2", sr, lst, ndvi, factor, MEAN, STD, ALPHA, GAMMA, valid=valid)),
         "fused_call": lambda: rloss.sif_loss_with_grad("sr2", sr, lst, ndvi, factor, MEAN, STD, ALPHA, GAMMA)}
    if factor == 4:
        ones = torch.ones((B, 1, h, w), dtype=torch.uint8, device="cuda")
        n = torch.tensor(B * h * w, dtype=torch.int64, device="cuda")
        v["div4_masked"] = lambda: sifsr.masked_sif_loss_with_grad("sr2", sr, lst, ones, n, ndvi, MEAN, STD, ALPHA, GAMMA)
    a, b = v["composed"]().clone(), v["fused"]().clone()
    check = {"dsr_rel_err_against_composed": float((a - b).abs().max() / a.abs().max()), "invalid_share": float((valid == 0).float().mean())}
    return v, check


def step_variants(sifsr, batch, hr=192, factor=3.0):
    from sifsr import rloss, sensor
    stats = {"mean_lst": 300.0, "std_lst": 10.0}
    out = {}
    for name in ("sensor_step_x3", "rloss_step_x3", "rloss_step_x3_masked"):
        torch.manual_seed(0)
        m = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda()
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-4)
        h, w = sensor.lr_shape(hr, hr, factor)
        lst = torch.randn((batch, 1, h, w), device="cuda")
        up = F.interpolate(lst, size=(hr, hr), mode="bicubic", align_corners=False).contiguous()
        ndvi = torch.randn((batch, 1, hr, hr), device="cuda")
        valid = (torch.rand((batch, 1, h, w), device="cuda") > 0.35).to(torch.uint8)
        if name == "sensor_step_x3":
            out[name] = lambda m=m, opt=opt, lst=lst, up=up, ndvi=ndvi: sensor.train_step(m, opt, lst, up, ndvi, stats, 0.5, 1.0, factor)
        elif name == "rloss_step_x3":
            out[name] = lambda m=m, opt=opt, lst=lst, up=up, ndvi=ndvi: rloss.train_step(m, opt, lst, up, ndvi, stats, 0.5, 1.0, factor)
        else:
            out[name] = lambda m=m, opt=opt, lst=lst, up=up, ndvi=ndvi, valid=valid: rloss.train_step(m, opt, lst, up, ndvi, stats, 0.5, 1.0,
                                                                                                     factor, valid=valid)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", type=int, default=None, help="HR side of the one shape to time (192, 160 or 256)")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_rloss.py needs a ROCm GPU"
    import sifsr
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for hr, factor in ((192, 3.0), (160, 2.5), (256, 4.0)):
        if args.only not in (None, hr):
            continue
        variants, check = loss_variants(sifsr, (args.batch, 1, hr, hr), factor)
        result["shapes"][f"{args.batch}x1x{hr}x{hr} factor {factor:g}"] = {
            "check": check, "per_call": alternating(variants, args.windows, args.reps, args.warmup)}
    if not args.no_step:
        result["step"] = {"batch": args.batch, "hr": 192, "factor": 3.0,
                          "per_call": alternating(step_variants(sifsr, args.batch), args.windows, args.reps, args.warmup)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
