#!/usr/bin/env python3
"""Time the sharpening baselines at any ratio (csrc/rbaselines_api.h, sifsr/rbaselines.py) beside
`sifsr.baselines` at x4 on the same coarse rasters.

    python tools/time_rbaselines.py [--windows 9] [--reps 5] [--warmup 2] [--only methods,passes] [--sizes aster,granule]
                                    [--out FILE.json]

Every figure is the median (with minimum and maximum) over `windows` windows of `reps` back-to-back calls between two HIP events on
the current stream, the stream synchronised before and after each window, after `warmup` calls of every variant of the group; the
variants of one group ALTERNATE window by window inside the one process, so that clock and cache state are shared.  Profiler off.

  sizes     aster: a batch of 83 pairs with coarse 64 x 64; granule: one 1200 x 1200 coarse raster
  methods   tsharp, atprk, aatprk (with `variogram=` given: the host's fits are the same code at every scale and are not what this
            change adds) and dms (10 estimators, seed 0, whole) at x3 and x2 (x2.5 for tsharp and dms) through sifsr.rbaselines,
            beside sifsr.baselines at x4
  passes    the fine-raster entry points alone -- sifsrh_sharpen modes 0, 1, 2, sifsrh_predict, sifsrh_aggregate (pow4, no std),
            sifsrh_correct -- at the same ratios beside their x4 counterparts sifsrb_sharpen, sifsrd_predict, sifsrd_aggregate,
            sifsrd_correct, with the bytes per fine pixel each must move (sharpen, predict, correct: 4 in + 4 out; aggregate: 4 in;
            the coarse operands are counted in `bytes` but are a few per cent), the GB/s that makes and its share of 8 TB/s

No ratio is asserted.  Nothing is fetched; inputs are seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_ratio import alternating  # noqa: E402

VARIO = (15.5, 4450.0)
HBM_GBS = 8000.0
SIZES = {"aster": (83, 64, 64), "granule": (1, 1200, 1200)}


def fields(B, h, w, p, q, seed):
    """(lst (B,1,h,w), ndvi_coarse (B,1,h,w), ndvi_fine (B,1,H,W)): a smooth index with noise, its cell mean, lst regressed on it"""
    from sifsr import rbaselines as RB
    H, W = h // q * p, w // q * p
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None] * (4.0 * q / p)
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :] * (4.0 * q / p)
    ph = torch.rand((B, 3, 1, 1), generator=g, device="cuda") * 6.283
    nf = 0.4 + 0.3 * torch.sin(yy / 37 + ph[:, 0]) * torch.cos(xx / 29 + ph[:, 1]) + 0.12 * torch.sin(yy / 11 + xx / 13 + ph[:, 2]) \
        + 0.03 * torch.randn((B, H, W), generator=g, device="cuda")
    nf = nf.clamp(-1, 1)[:, None].contiguous()
    nc = RB.dms_aggregate(nf, coarse=(h, w))[0].float()[:, None].contiguous()
    cy = torch.arange(h, device="cuda", dtype=torch.float32)[:, None]
    lst = 312 - 14 * nc + 1.5 * torch.sin(cy / 7) + 0.4 * torch.randn((B, 1, h, w), generator=g, device="cuda")
    return lst.contiguous(), nc, nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="methods,passes")
    ap.add_argument("--sizes", default="aster,granule")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_rbaselines.py needs a ROCm GPU"
    import sifsr
    from sifsr import baselines as BL
    from sifsr import rbaselines as RB
    L = sifsr._lib
    RB.bound()
    S = lambda: torch.cuda.current_stream().cuda_stream
    groups, timing = set(args.only.split(",")), (args.windows, args.reps, args.warmup)
    result = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "reps": args.reps, "sizes": {}}
    for size in args.sizes.split(","):
        B, h, w = SIZES[size]
        ratios = {"x3": (3, 1), "x2": (2, 1), "x2.5": (5, 2), "x4": (4, 1)}
        data = {k: fields(B, h, w, p, q, 1) for k, (p, q) in ratios.items()}
        lst, nc = data["x4"][0], data["x4"][1]                       # the same coarse rasters for every ratio
        fine = {k: v[2] for k, v in data.items()}
        res = {"lst": [B, h, w], "fine": {k: list(v.shape[2:]) for k, v in fine.items()}}
        if "methods" in groups:
            per = {}
            for name, rs in (("tsharp", ("x3", "x2.5")), ("atprk", ("x3", "x2")), ("aatprk", ("x3", "x2")), ("dms", ("x3", "x2.5"))):
                kw = {"variogram": VARIO} if "prk" in name else ({"n_estimators": 10, "seed": 0} if name == "dms" else {})
                args_of = (lambda f: (lst, f)) if name == "dms" else (lambda f: (lst, nc, f))
                v = {f"{name}_{r}": (lambda r=r: getattr(RB, name)(*args_of(fine[r]), **kw)) for r in rs}
                v[f"{name}_x4_baselines"] = lambda: getattr(BL, name)(*args_of(fine["x4"]), **kw)
                per.update(alternating(v, *timing))
            res["methods"] = per
        if "passes" in groups:
            per = {}
            fit = torch.empty((B, 2), dtype=torch.float64, device="cuda")
            L.call("sifsrb_linfit", lst, nc, fit, B, h, w, 285.0, S())
            coef = torch.empty((B, 2, h, w), dtype=torch.float64, device="cuda")
            L.call("sifsrb_linfit_window", lst, nc, fit, coef, B, h, w, 2, 285.0, S())
            delta = torch.empty((B, h, w), dtype=torch.float64, device="cuda")
            L.call("sifsrb_residual", lst, nc, fit, 0, delta, B, h, w, S())
            m4 = torch.empty((B, h, w), dtype=torch.float64, device="cuda")
            small = BL.dms_model(lst[:1, :, :64, :64].contiguous(), fine["x4"][:1, :, :256, :256].contiguous(), n_estimators=10, seed=0)
            model = {k: small[k].expand(B, *small[k].shape[1:]).contiguous() for k in ("thresholds", "nleaf", "leaves")}
            coarse_bytes = {0: 4 + 8, 1: 4 + 8, 2: 16 + 8}           # per coarse cell: lst or coef, delta
            for mode, rs in ((0, ("x3", "x2.5")), (1, ("x3", "x2")), (2, ("x3", "x2"))):
                v, nbytes = {}, {}
                for r in rs + ("x4",):
                    p, q = ratios[r]
                    f, o = fine[r], torch.empty_like(fine[r])
                    H, W = f.shape[2:]
                    lam = torch.from_numpy(RB.kriging_weights(*VARIO, 926.0, p)[None].repeat(B, 0)).cuda() if mode else None
                    c = coef if mode == 2 else fit
                    if r == "x4":
                        key = f"sifsrb_sharpen_mode{mode}_x4"
                        v[key] = lambda f=f, o=o, lam=lam, c=c: L.call("sifsrb_sharpen", lst, f, c, delta, lam, o, B, h, w, mode, S())
                    else:
                        key = f"sifsrh_sharpen_mode{mode}_{r}"
                        v[key] = lambda f=f, o=o, lam=lam, c=c, H=H, W=W: L.call("sifsrh_sharpen", lst, f, c, delta, lam, o, B, h, w, H,
                                                                                   W, mode, S())
                    nbytes[key] = (8 * B * H * W + coarse_bytes[mode] * B * h * w, 8)
                t = alternating(v, *timing)
                for k in t:
                    t[k]["bytes"], t[k]["bytes_per_fine_pixel"] = nbytes[k]
                per.update(t)
            for what in ("predict", "aggregate", "correct"):
                v, nbytes = {}, {}
                for r in ("x3", "x2.5", "x4"):
                    f, o = fine[r], torch.empty_like(fine[r])
                    H, W = f.shape[2:]
                    if what == "predict":
                        new = lambda f=f, o=o, H=H, W=W: L.call("sifsrh_predict", f, model["thresholds"], model["nleaf"], model["leaves"], o,
                                                               B, 10, H, W, S())
                        old = lambda f=f, o=o: L.call("sifsrd_predict", f, model["thresholds"], model["nleaf"], model["leaves"], o, B, 10, h,
                                                      w, S())
                        nb = (8 * B * H * W, 8)
                    elif what == "aggregate":
                        new = lambda f=f, H=H, W=W: L.call("sifsrh_aggregate", f, m4, None, B, h, w, H, W, 1, S())
                        old = lambda f=f: L.call("sifsrd_aggregate", f, m4, None, B, h, w, 1, S())
                        nb = (4 * B * H * W + 8 * B * h * w, 4)
                    else:
                        sr = (300 + 20 * f).contiguous()
                        L.call("sifsrh_aggregate" if r != "x4" else "sifsrd_aggregate", sr, m4, None, B, h, w, *((H, W) if r != "x4" else ()),
                               1, S())
                        mm = m4.clone()
                        new = lambda sr=sr, mm=mm, o=o, H=H, W=W: L.call("sifsrh_correct", lst, sr, mm, o, B, h, w, H, W, S())
                        old = lambda sr=sr, mm=mm, o=o: L.call("sifsrd_correct", lst, sr, mm, o, B, h, w, S())
                        nb = (8 * B * H * W + 12 * B * h * w, 8)
                    key = f"sifsrd_{what}_x4" if r == "x4" else f"sifsrh_{what}_{r}"
                    v[key], nbytes[key] = (old if r == "x4" else new), nb
                    if r == "x4":                                    # and the new entry point at x4, beside its counterpart
                        v[f"sifsrh_{what}_x4"], nbytes[f"sifsrh_{what}_x4"] = new, nb
                t = alternating(v, *timing)
                for k in t:
                    t[k]["bytes"], t[k]["bytes_per_fine_pixel"] = nbytes[k]
                per.update(t)
            for r in per.values():
                r["GB_per_s"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e9
                r["share_of_8TBs"] = r["GB_per_s"] / HBM_GBS
            res["passes"] = per
        result["sizes"][size] = res
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
