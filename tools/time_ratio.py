#!/usr/bin/env python3
"""Time whole-granule prediction at any ratio (include/sifsr_ratio.h).

    python tools/time_ratio.py [--windows 9] [--reps 5] [--warmup 3] [--side 1200] [--gaps 0.35] [--batch 256]
                               [--only granule,gaps,upsample,kernels] [--out FILE.json]

Every figure is the median (with minimum and maximum) over `windows` windows of `reps` back-to-back calls between two HIP events on
the current stream, the stream synchronised before and after each window, after `warmup` calls of every variant of the group; the
variants of one group ALTERNATE window by window inside the one process, so that clock and cache state are shared.  Profiler off;
kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/time_ratio.py --only kernels` run.

  granule    `ratio.predict_granule` on a side x side LST granule at (64, 192) and (64, 160), overlap 16, cover_edges, beside
             `predict.predict_granule` at x4 on the same LST raster (each with an NDVI raster of its own size)
  gaps       `ratio.predict_granule_gaps` on the same granule and layouts with `gaps` of the pixels in cloud-like holes
  upsample   `ratio.upsample` (64,1,64,64) -> 192 beside `F.interpolate(mode="bicubic")` on the same device, and their difference
             from the float64 operator
  kernels    the prepare and blend calls alone, at (64, 192), (64, 160) and x4 (`pipeline.granule_to_tiles` / `blend_tiles`), with
             the bytes each moves: prepare reads the LST raster and one NDVI block per tile and writes two planes per tile, blend
             reads one plane per tile and writes the raster

No ratio is asserted.  Nothing is fetched; inputs are seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATS = {"mean_lst": 307.2378, "std_lst": 5.5698, "mean_ndvi": 0.6452, "std_ndvi": 0.1683}
LAYOUT = dict(overlap=16, cover_edges=True)


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


def granule(side, hr, seed=0):
    """a side x side LST raster [K] (the same for every hr) and an NDVI raster at hr / 64 of it"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lst = 307.0 + 5.5 * torch.randn((side, side), device="cuda", generator=g)
    n = side * hr // 64
    ndvi = 0.5 + 0.3 * torch.randn((n, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + hr))
    return lst, ndvi


def holes(side, fraction, seed=1):
    """cloud-like holes: a coarse random field, smoothed and cut at the quantile that leaves `fraction` of the pixels invalid"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.randn((1, 1, side // 200 + 2, side // 200 + 2), device="cuda", generator=g)
    field = F.interpolate(coarse, size=(side, side), mode="bicubic", align_corners=False)[0, 0]
    return field < torch.quantile(field.flatten()[::7], fraction)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=1200)
    ap.add_argument("--gaps", type=float, default=0.35)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default="granule,gaps,upsample,kernels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ratio.py needs a ROCm GPU"
    import sifsr
    from sifsr import pipeline, predict, ratio
    groups = set(args.only.split(","))
    torch.manual_seed(0)
    model = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda().eval()
    side, win = args.side, 64
    rasters = {hr: granule(side, hr) for hr in (192, 160, 256)}
    lst = rasters[192][0]
    timing = (args.windows, args.reps, args.warmup)
    result = {"device": torch.cuda.get_device_name(0), "lst_granule": [side, side], "window": win, **LAYOUT, "batch": args.batch}

    if "granule" in groups:
        v = {f"ratio_{hr}": (lambda hr=hr: ratio.predict_granule(model, lst, rasters[hr][1], STATS, win, hr, args.batch, **LAYOUT))
             for hr in (192, 160)}
        v["x4_256"] = lambda: predict.predict_granule(model, lst, rasters[256][1], STATS, win, args.batch, **LAYOUT)
        result["granule"] = {"tiles": list(ratio.geometry((side, side), win, 192, 16, True).tiles),
                             "per_call": alternating(v, *timing)}
    if "gaps" in groups:
        gappy = torch.where(holes(side, args.gaps), torch.zeros_like(lst), lst)
        info = {hr: ratio.predict_granule_gaps(model, gappy, rasters[hr][1], STATS, None, win, hr, args.batch, return_info=True, **LAYOUT)[1]
                for hr in (192, 160)}
        v = {f"ratio_gaps_{hr}": (lambda hr=hr: ratio.predict_granule_gaps(model, gappy, rasters[hr][1], STATS, None, win, hr, args.batch,
                                                                           **LAYOUT)) for hr in (192, 160)}
        result["gaps"] = {"invalid_fraction": float((gappy == 0).float().mean()),
                          "active_tiles": {str(hr): [i["n_active"], i["n_tiles"]] for hr, i in info.items()},
                          "per_call": alternating(v, *timing)}
    if "upsample" in groups:
        x = torch.randn((64, 1, 64, 64), device="cuda")
        v = {"ratio_upsample": lambda: ratio.upsample(x, (192, 192)),
             "torch_interpolate": lambda: F.interpolate(x, size=(192, 192), mode="bicubic", align_corners=False)}
        ref = F.interpolate(x.double().cpu(), size=(192, 192), mode="bicubic", align_corners=False)
        result["upsample"] = {"shape": "64x1x64x64 -> 192", "per_call": alternating(v, *timing),
                              "max_abs_from_float64": {k: float((fn().double().cpu() - ref).abs().max()) for k, fn in v.items()}}
    if "kernels" in groups:
        out = {}
        for hr in (192, 160, 256):
            ndvi = rasters[hr][1]
            ty, tx = ratio.geometry((side, side), win, hr, 16, True).tiles
            T, n = ty * tx, ndvi.shape[0]
            x = torch.empty((T, 2, hr, hr), device="cuda")
            sr = torch.randn((T, 1, hr, hr), device="cuda")
            o = torch.empty((n, n), device="cuda")
            v = {f"ratio_prepare_{hr}": lambda: ratio.granule_to_tiles(lst, ndvi, STATS, win, hr, True, out=x, **LAYOUT),
                 f"ratio_blend_{hr}": lambda: ratio.blend_tiles(sr, (side, side), win, hr, STATS, out=o, **LAYOUT)}
            if hr == 256:
                v["x4_prepare_256"] = lambda: pipeline.granule_to_tiles(lst, ndvi, STATS, win, True, out=x, **LAYOUT)
                v["x4_blend_256"] = lambda: pipeline.blend_tiles(sr, (side, side), win, STATS, out=o, **LAYOUT)
            per = alternating(v, *timing)
            nbytes = {"prepare": 4 * (side * side + 3 * T * hr * hr), "blend": 4 * (T * hr * hr + n * n)}
            for name, r in per.items():
                r["bytes"] = nbytes["prepare" if "prepare" in name else "blend"]
                r["GB_per_s"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e9
            out.update(per)
        result["kernels"] = out
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
