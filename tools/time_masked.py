#!/usr/bin/env python3
"""Time the masked SIF loss and the per-patch fill (include/sifsr_masked.h) at the training shape: B = 64,
256 x 256, kind sr2.

    python tools/time_masked.py [--runs 30] [--warmup 5] [--out FILE.json]

Median / minimum / maximum over `runs` calls (after `warmup`) between HIP events on the current stream of
  * `sifsr_sif_loss`, the unmasked loss with its gradient -- the yardstick: this row leaves that call's arithmetic and instruction
    mix as they were, so the time is the previous revision's,
  * `sifsrm_sif_loss` with every LR pixel valid, and with about 35 % invalid (seeded blobs per image: a 6 x 6 field of N(0, 1)
    draws enlarged bicubically to 64 x 64 and thresholded at its 0.35 quantile), on the SAME sr / lst / ndvi,
  * `sifsrm_patches_fill` at N = 324, w = 64 (the full windows of one 1200 x 1200 granule) with the same share of holes.
What to read from it: the mask adds one byte per 16 HR pixels to what pass A reads (about 0.4 %), so the masked medians should
lie inside the min-max spread of the unmasked one.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD, ALPHA, GAMMA = 307.2378, 5.5698, 0.5, -0.25
B, HR, KIND = 64, 256, 2


def blobs(seed, n, side, fraction):
    """bool (n, 1, side, side): True = invalid, about `fraction` of the pixels of every image"""
    coarse = torch.from_numpy(np.random.RandomState(seed).standard_normal((n, 1, 6, 6)).astype(np.float32))
    field = torch.nn.functional.interpolate(coarse, size=(side, side), mode="bicubic", align_corners=False)
    return field < torch.quantile(field.reshape(n, -1), fraction, dim=1).reshape(n, 1, 1, 1)


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
    assert torch.cuda.is_available(), "time_masked.py needs a ROCm GPU"
    import sifsr
    from sifsr import dataset, sif_ops
    L = sifsr._lib
    S = lambda: torch.cuda.current_stream().cuda_stream
    lst, lst_up, ndvi = dataset.synthetic_device_batch(B, "cuda", hr=HR)
    sr = (lst_up + 0.5 * torch.randn(lst_up.shape, generator=torch.Generator().manual_seed(1)).cuda()).contiguous()
    t1, t2 = sif_ops._taps_c(0.1, 4, None), sif_ops._taps_c(0.25, 4, None)
    need = L.call("sifsr_sif_loss_workspace_bytes", KIND, B, HR, HR)
    assert need == L.call("sifsrm_sif_loss_workspace_bytes", KIND, B, HR, HR)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    losses, dsr = torch.empty(3, device="cuda"), torch.empty_like(sr)
    all_valid = torch.ones((B, 1, HR // 4, HR // 4), dtype=torch.uint8, device="cuda")
    gappy = (~blobs(2, B, HR // 4, 0.35)).to(torch.uint8).cuda()
    count = lambda v: v.sum(dtype=torch.int64)

    def masked(valid):
        n = count(valid)
        return lambda: L.call("sifsrm_sif_loss", KIND, sr, lst, valid, n, ndvi, B, HR, HR, MEAN, STD, ALPHA, GAMMA, t1, t2, ws, need,
                              losses, dsr, S())

    calls = {
        "sif_loss": lambda: L.call("sifsr_sif_loss", KIND, sr, lst, ndvi, B, HR, HR, MEAN, STD, ALPHA, GAMMA, t1, t2, ws, need, losses, dsr, S()),
        "masked_all_valid": masked(all_valid),
        "masked_35_invalid": masked(gappy),
    }
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "hr": HR, "kind": "sr2",
              "invalid_fraction": float((gappy == 0).float().mean())}
    result.update({k: timed(f, args.runs, args.warmup) for k, f in calls.items()})
    for k in ("masked_all_valid", "masked_35_invalid"):
        result[k]["over_unmasked"] = result[k]["median_ms"] / result["sif_loss"]["median_ms"]
    # the per-patch fill: the 324 full windows of a 1200 x 1200 granule
    n, w = 324, 64
    patches = (torch.randn((n, 1, w, w), generator=torch.Generator().manual_seed(3)) * 5.5 + 307).cuda()
    patches[blobs(4, n, w, 0.35).cuda()] = 0.0
    filled, valid = torch.empty_like(patches), torch.empty(patches.shape, dtype=torch.uint8, device="cuda")
    moments = torch.empty((n, 5), dtype=torch.float64, device="cuda")
    result["patches_fill"] = timed(lambda: L.call("sifsrm_patches_fill", patches, filled, valid, moments, n, w, S()), args.runs, args.warmup)
    result["patches_fill"].update(n=n, w=w, invalid_fraction=float((valid == 0).float().mean()))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
