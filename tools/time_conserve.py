#!/usr/bin/env python3
"""Time the conservation check and correction (include/sifsr_conserve.h) on one MODIS-sized granule: 1200 x 1200
LST -> 4800 x 4800 super-resolved, about 30 % of the granule as gaps (the blobs of tools/time_gaps.py).

    python tools/time_conserve.py [--size 1200] [--gaps 0.3] [--runs 10] [--warmup 3] [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_conserve.py --profile-pass
    python tools/time_conserve.py --kernel-stats FILE [--size 1200]     (no GPU needed; FILE: the *_kernel_stats.csv under DIR)

Reported, median / minimum / maximum over `runs` calls after `warmup`, between HIP events on the current stream, profiler off:
  * `sifsrk_conserve` at n_iter = 0 (one residual launch + the finish), n_iter = 1 and 2, in place and into a second buffer; the
    difference n_iter 2 - n_iter 1 is one correction step (one apply + one residual launch);
  * `predict_granule_gaps(conserve=1)` and `(conserve=0)` on the same granule, and the difference: what the option adds.
With --kernel-stats: the mean time of the residual and the apply kernel from a `rocprofv3 --kernel-trace --stats` run of
--profile-pass (a run of its own) and the GB/s they reach against the bytes they must move -- one read of sr (64 h w bytes) for
the residual; one read and one write of sr for the apply, of which a call in place touches only the cells with c.
The raster is the network's own output for a seeded random model; nothing is fetched.  Timing needs a GPU: there is no fallback."""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_gaps import BATCH, COVER, OVERLAP, STATS, WINDOW, granule, timed  # noqa: E402

HBM_PEAK_TBS = 8.0               # the HBM peak DESIGN.md §9 takes its floors from


def kernel_stats(path, h, w, valid_share):
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}
    out = {}
    for key, nbytes in (("conserve_residual_kernel", 64.0 * h * w), ("conserve_apply_kernel", 128.0 * h * w)):
        hit = [r for n, r in rows.items() if key in n]
        if not hit:
            continue
        calls = int(hit[0]["Calls"])
        us = float(hit[0]["TotalDurationNs"]) / calls / 1e3
        out[key] = {"calls": calls, "mean_us": us, "bytes_nominal": nbytes, "gbs_nominal": nbytes / us / 1e3}
        if key == "conserve_apply_kernel" and valid_share is not None:
            out[key]["gbs_in_place_valid_cells_only"] = nbytes * valid_share / us / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1200)
    ap.add_argument("--gaps", type=float, default=0.30)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--valid-share", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    h = args.size
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats, h, h, args.valid_share), indent=1))
        return
    assert torch.cuda.is_available(), "time_conserve.py needs a ROCm GPU"
    import sifsr
    from sifsr import conserve as C
    L = sifsr._lib
    S = lambda: torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    model = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda().eval()
    lst_np, ndvi_np = granule(1, h, args.gaps)
    lst, ndvi = torch.from_numpy(lst_np).cuda(), torch.from_numpy(ndvi_np).cuda()
    kw = dict(window=WINDOW, batch=BATCH, overlap=OVERLAP, cover_edges=COVER)
    sr0 = sifsr.predict.predict_granule_gaps(model, lst, ndvi, STATS, **kw)
    taps = sifsr.sif_ops._taps_c(0.1, 4, None)
    need = L.call("sifsrk_workspace_bytes", h, h, 2)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    stats = torch.empty((3, 4), dtype=torch.float64, device="cuda")
    work, other = sr0.clone(), torch.empty_like(sr0)

    def call(n_iter, out):
        return lambda: L.call("sifsrk_conserve", work, lst, None, out, stats, ws, need, h, h, taps, 1.0, n_iter, S())

    if args.profile_pass:
        for _ in range(3):
            call(1, work)()
        torch.cuda.synchronize()
        return
    row = C.consistency(sr0, lst).cpu().numpy()
    valid_share = float(((lst != 0) & torch.isfinite(lst)).float().mean())
    calls = {"check_n_iter_0": call(0, None), "n_iter_1_in_place": call(1, work), "n_iter_2_in_place": call(2, work),
             "n_iter_1_second_buffer": call(1, other),
             "predict_granule_gaps_conserve_0": lambda: sifsr.predict.predict_granule_gaps(model, lst, ndvi, STATS, **kw),
             "predict_granule_gaps_conserve_1": lambda: sifsr.predict.predict_granule_gaps(model, lst, ndvi, STATS, conserve=1, **kw)}
    # (the in-place calls keep correcting `work`: the time of a launch does not depend on the values)
    t = {k: timed(f, args.runs, args.warmup) for k, f in calls.items()}
    result = {"device": torch.cuda.get_device_name(0), "lst": [h, h], "sr": [4 * h, 4 * h], "gap_share": 1.0 - valid_share,
              "counted_cells": int(row[0]), "rmse_before_K": float(row[2]), "calls": t,
              "one_step_ms": t["n_iter_2_in_place"]["median_ms"] - t["n_iter_1_in_place"]["median_ms"],
              "added_by_conserve_1_ms": t["predict_granule_gaps_conserve_1"]["median_ms"] - t["predict_granule_gaps_conserve_0"]["median_ms"],
              "sr_bytes": 64 * h * h, "hbm_peak_tbs": HBM_PEAK_TBS,
              "least_ms_residual": 64 * h * h / HBM_PEAK_TBS / 1e9, "least_ms_apply": 128 * h * h / HBM_PEAK_TBS / 1e9}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
