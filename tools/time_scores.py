#!/usr/bin/env python3
"""Time the valid-pixel scores (include/sifsr_scores.h) next to the unmasked entry points they instantiate.

    python tools/time_scores.py [--runs 30] [--warmup 5] [--out FILE.json]

Median / minimum / maximum over `runs` calls (after `warmup`) between HIP events on the current stream, at B = 64 of 256 x 256 and
at B = 8 of 335 x 374 (an ASTER overlap), of
  * `sifsr_eval_metrics`, the unmasked per-pair table -- the yardstick: its kernels are the same code as before this row (the
    non-MASKED instantiations), so its time is the previous revision's,
  * `sifsrv_eval_metrics` with every pixel valid, and with about 35 % invalid (seeded blobs per image: a 6 x 6 field of N(0, 1)
    draws enlarged bicubically and thresholded at its 0.35 quantile), on the SAME image pairs,
and at B = 64 of 256 x 256 of `sifsr_psnr_ssim` against `sifsrv_psnr_ssim` (scale 4, the LR mask of the masked loader) in the same
two states.  The only expectation that can be derived in advance is the traffic: the masked calls write and read one validity byte
per pixel on top of the eight bytes of the two images per pass.  No ratio is asserted anywhere; DESIGN.md records what was measured.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64, 256, 256), (8, 335, 374))
FRACTION = 0.35


def blobs(seed, n, h, w, fraction):
    """bool (n, h, w): True = invalid, about `fraction` of the pixels of every image"""
    coarse = torch.from_numpy(np.random.RandomState(seed).standard_normal((n, 1, 6, 6)).astype(np.float32))
    field = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bicubic", align_corners=False)[:, 0]
    return field < torch.quantile(field.reshape(n, -1), fraction, dim=1).reshape(n, 1, 1)


def pairs(seed, n, h, w):
    """Kelvin-scale reference / prediction pairs: a smooth field and a noisy copy of it"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((n, 1, h, w), generator=g).cumsum(2).cumsum(3) * 0.05 + 300
    b = a + 0.4 * torch.randn((n, 1, h, w), generator=g) + 0.2
    return a.float().contiguous().cuda(), b.float().contiguous().cuda()


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_scores.py needs a ROCm GPU"
    import sifsr
    from sifsr import sif_ops
    L = sifsr._lib
    S = lambda: torch.cuda.current_stream().cuda_stream
    taps = sif_ops._taps_c(0.1, 4, None)
    result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "eval_metrics": {}, "psnr_ssim": {}}
    for B, H, W in SHAPES:
        a, b = pairs(B + H, B, H, W)
        ones = torch.ones((B, H, W), dtype=torch.uint8, device="cuda")
        gappy = (~blobs(2, B, H, W, FRACTION)).to(torch.uint8).cuda()
        need0, need1 = L.call("sifsr_eval_metrics_scratch_bytes", B, H, W), L.call("sifsrv_eval_metrics_scratch_bytes", B, H, W)
        ws = torch.empty((max(need0, need1),), dtype=torch.uint8, device="cuda")
        out8 = torch.empty((B, 8), dtype=torch.float64, device="cuda")
        counts5 = torch.empty((B, 5), dtype=torch.int32, device="cuda")
        masked = lambda m: (lambda: L.call("sifsrv_eval_metrics", a, b, m, B, H, W, taps, -1.0, ws, need1, out8, counts5, S()))
        calls = {"unmasked": lambda: L.call("sifsr_eval_metrics", a, b, B, H, W, taps, -1.0, ws, need0, out8, S()),
                 "masked_all_valid": masked(ones), "masked_35_invalid": masked(gappy)}
        row = {k: timed(f, args.runs, args.warmup) for k, f in calls.items()}
        for k in ("masked_all_valid", "masked_35_invalid"):
            row[k]["over_unmasked"] = row[k]["median_ms"] / row["unmasked"]["median_ms"]
        row["invalid_fraction"] = float((gappy == 0).float().mean())
        row["scratch_bytes"] = {"unmasked": need0, "masked": need1}
        result["eval_metrics"][f"B{B}_{H}x{W}"] = row
    B, H, W = SHAPES[0]
    t, p = pairs(5, B, H, W)
    ones = torch.ones((B, H // 4, W // 4), dtype=torch.uint8, device="cuda")
    gappy = (~blobs(3, B, H // 4, W // 4, FRACTION)).to(torch.uint8).cuda()
    need0, need1 = L.call("sifsr_psnr_ssim_scratch_bytes", B, H, W), L.call("sifsrv_psnr_ssim_scratch_bytes", B, H, W)
    ws = torch.empty((max(need0, need1),), dtype=torch.uint8, device="cuda")
    out2, counts2 = torch.empty(2, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")
    masked = lambda m: (lambda: L.call("sifsrv_psnr_ssim", p, t, m, 4, B, H, W, ws, need1, out2, counts2, S()))
    calls = {"unmasked": lambda: L.call("sifsr_psnr_ssim", p, t, B, H, W, ws, need0, out2, S()),
             "masked_all_valid": masked(ones), "masked_35_invalid": masked(gappy)}
    row = {k: timed(f, args.runs, args.warmup) for k, f in calls.items()}
    for k in ("masked_all_valid", "masked_35_invalid"):
        row[k]["over_unmasked"] = row[k]["median_ms"] / row["unmasked"]["median_ms"]
    row["invalid_fraction"] = float((gappy == 0).float().mean())
    result["psnr_ssim"][f"B{B}_{H}x{W}_scale4"] = row
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
