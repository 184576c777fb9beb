#!/usr/bin/env python3
"""Time the consistency check and the residual correction at any ratio (include/sifsr_rconserve.h) beside the
composed path, beside the x4 kernels of f12, and inside whole-granule prediction.

    python tools/time_rconserve.py [--windows 9] [--reps 5] [--warmup 3] [--side 1200] [--only HR] [--no-granule] [--out FILE.json]

Every figure is the median (with minimum and maximum) over `windows` windows of `reps` back-to-back calls between two HIP events on
the current stream, the stream synchronised before and after each window, after `warmup` calls of every variant of the shape; the
variants of one shape ALTERNATE window by window inside the one process, so that clock and cache state are shared.  Profiler off;
kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/time_rconserve.py --only 192 --no-granule` run.

Per shape -- an LST granule of `side` x `side` at (window, hr) = (64, 192), (64, 160) and (64, 256), with 35 % of the cells invalid
(blobs of cloud) and with none --, on the same tensors:
  step            `rconserve.conserve(sr, lst, mask, n_iter=1, out=buf)`: the table kernel, two residual kernels, one correction, the
                  finish (the second residual is the statistics row after the step)
  check           `rconserve.consistency(sr, lst, mask)`: the table kernel, one residual kernel, the finish
  composed        `sensor.downscale(sr, factor, valid=pixel mask, return_valid=True)`, the residual under `torch.where`,
                  `ratio.upsample` and `torch.where` into a new raster -- one step without its statistics, the pixel mask formed once
  x4_step / x4_check   at hr 256 only: `conserve.conserve(n_iter=1)` / `conserve.consistency` of f12 on the same rasters
and, unless --no-granule, `ratio.predict_granule_gaps` of the gappy granule at (64, 192) and (64, 160), overlap 16, covered edges,
with `conserve=0` and `conserve=1`.  The byte floor of one step is 3 * 4 * H * W bytes (sr read by the residual, read and written by
the correction); `step` holds two residual kernels, so its floor is 4 * 4 * H * W.  No ratio is asserted.  Nothing is fetched; inputs
are seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_sensor import alternating  # noqa: E402

STATS = {"mean_lst": 307.2378, "std_lst": 5.5698, "mean_ndvi": 0.4, "std_ndvi": 0.25}


def cloud_mask(side, share, seed):
    """blobs: a smooth random field thresholded at the `share` quantile -> uint8 (side, side), 0 under cloud"""
    if share <= 0:
        return None
    g = torch.Generator().manual_seed(seed)
    f = torch.nn.functional.interpolate(torch.randn((1, 1, side // 24 + 2, side // 24 + 2), generator=g), size=(side, side), mode="bicubic",
                                        align_corners=False)[0, 0]
    return (f > torch.quantile(f.flatten()[::7], share)).to(torch.uint8)


def rasters(side, hr, share, seed=0):
    p, q = {192: (3, 1), 160: (5, 2), 256: (4, 1)}[hr]             # hr / 64 in lowest terms
    H = side * p // q
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="ij")
    sr = (300.0 + 6.0 * torch.sin(y / 53.0) * torch.cos(x / 37.0) + 0.8 * torch.randn((H, H), generator=g)).cuda()
    mask = cloud_mask(side, share, seed + 1)
    return sr, mask if mask is None else mask.cuda(), (p, q)


def shape_variants(sifsr, side, hr, share):
    from sifsr import conserve, ratio, rconserve, sensor
    sr, mask, (p, q) = rasters(side, hr, share)
    H = sr.shape[0]
    factor = H / side
    lst = sensor.downscale(sr + 0.3, factor).contiguous() + 0.05 * torch.randn((side, side), device="cuda")
    buf = torch.empty_like(sr)
    cells = torch.arange(H, device="cuda") * side // H
    c = torch.ones((side, side), dtype=torch.bool, device="cuda") if mask is None else mask.bool()
    pix = c[cells][:, cells].to(torch.uint8).contiguous()

    def composed():
        d, ov = sensor.downscale(sr, factor, valid=pix, fill_value=0.0, return_valid=True)
        r = torch.where(ov.bool() & c, lst - d, torch.zeros_like(lst))
        return torch.where(pix.bool(), sr + ratio.upsample(r, (H, H)), sr)

    v = {"step": lambda: rconserve.conserve(sr, lst, mask, n_iter=1, out=buf),
         "check": lambda: rconserve.consistency(sr, lst, mask),
         "composed": composed}
    if hr == 256:
        v["x4_step"] = lambda: conserve.conserve(sr, lst, mask, n_iter=1, out=buf)
        v["x4_check"] = lambda: conserve.consistency(sr, lst, mask)
    out, stats = rconserve.conserve(sr, lst, mask, n_iter=1, return_stats=True)
    ref = composed()
    m = pix.bool()
    check = {"hr_shape": [H, H], "factor": factor, "invalid_share": float((~c).float().mean()), "stats": stats.cpu().tolist(),
             "max_abs_diff_against_composed_K": float((out[m] - ref[m]).abs().max()), "step_floor_bytes": 3 * 4 * H * H}
    return v, check


def granule_variants(sifsr, side, hr, share):
    from sifsr import ratio
    sr, mask, (p, q) = rasters(side, hr, share)
    H = sr.shape[0]
    torch.manual_seed(0)
    model = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda().eval()
    lst = (307.0 + 5.5 * torch.randn((side, side), device="cuda"))
    lst = torch.where(mask.bool(), lst, torch.zeros_like(lst)) if mask is not None else lst
    ndvi = (0.5 + 0.3 * torch.randn((H, H), device="cuda")).clamp(-1, 1)
    kw = dict(window=64, hr=hr, batch=256, overlap=16, cover_edges=True)
    return {f"gaps_conserve{k}": (lambda k=k: ratio.predict_granule_gaps(model, lst, ndvi, STATS, conserve=k, **kw)) for k in (0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=1200)
    ap.add_argument("--only", type=int, default=None, help="hr of the one shape to time (192, 160 or 256)")
    ap.add_argument("--no-granule", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_rconserve.py needs a ROCm GPU"
    import sifsr
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "shapes": {}, "granule": {}}
    for hr in (192, 160, 256):
        if args.only not in (None, hr):
            continue
        for share in (0.35, 0.0):
            variants, check = shape_variants(sifsr, args.side, hr, share)
            per_call = alternating(variants, args.windows, args.reps, args.warmup)
            floor = check["step_floor_bytes"]
            # `step` = table + 2 residual + correction + finish and `check` = table + residual + finish: their difference is the one
            # residual kernel and the one correction kernel of a step, whose byte floor is 3 * 4 * H * W
            one = per_call["step"]["median_ms"] - per_call["check"]["median_ms"]
            check["step_minus_check_ms"] = one
            check["step_TBps_against_floor"] = floor / (one * 1e-3) / 1e12 if one > 0 else None
            check["share_of_8_TBps"] = check["step_TBps_against_floor"] / 8.0 if one > 0 else None
            result["shapes"][f"lst {args.side}x{args.side} hr {hr} gaps {share:g}"] = {"check": check, "per_call": per_call}
        if not args.no_granule and hr != 256:
            result["granule"][f"lst {args.side}x{args.side} hr {hr} gaps 0.35"] = alternating(
                granule_variants(sifsr, args.side, hr, 0.35), max(3, args.windows // 3), 1, 1)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
