#!/usr/bin/env python3
"""Time on-device LPIPS (include/sifsr_lpips.h) at the size of the reference's ASTER set: 83 pairs of 256 x 256.

    python tools/time_lpips.py [--pairs 83] [--size 256] [--runs 10] [--warmup 3] [--cpu-pairs 2] [--out FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_lpips.py --profile-pass
    python tools/time_lpips.py --kernel-stats FILE       (no GPU needed; FILE: the ONE *_kernel_stats.csv that run wrote under DIR)

Reported:
  * ms per pair of `LPIPS.pairs` (the table path, batches chunked as the Python interface chunks them): median / minimum / maximum
    over `runs` calls after `warmup`, between HIP events on the current stream, profiler off;
  * achieved fp32 TFLOP/s -- the 2 * 9 * cin * cout * h * w operations of the 13 convolutions of both images, computed from the
    shapes below, over the WHOLE call -- against the 157.3 TFLOP/s fp32 matrix bound DESIGN.md §4 uses (an end-to-end rate over
    peak, not a kernel's share of peak);
  * the CPU torch fp32 restatement (tests/lpips_reference.py) on the same host, per pair: what the reference does today;
  * with --kernel-stats: the share of the kernel time spent in the convolutions (MFMA + direct), in bias / ReLU / pool, in the
    distance kernel and in the rest, from a `rocprofv3 --kernel-trace --stats` run of --profile-pass (a run of its own).
The weights are the closed-form ones of tests/lpips_reference.py; nothing is fetched.  Timing needs a GPU: there is no fallback."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_TFLOPS = 157.3
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
POOL_AFTER = (1, 3, 6, 9)


def conv_flops_per_pair(H, W):
    """multiply-adds x 2 of the 13 convolutions, both images of a pair"""
    total, h, w = 0, H, W
    for l, (ci, co) in enumerate(CONV_CHANNELS):
        total += 2 * 9 * ci * co * h * w
        if l in POOL_AFTER:
            h, w = h // 2, w // 2
    return 2 * total


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


def kernel_shares(path):
    rows = list(csv.DictReader(open(path)))
    groups = {"conv": 0.0, "bias_relu_pool": 0.0, "distance": 0.0, "other": 0.0}
    for r in rows:
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "lpips_" not in name and "conv3x3_mfma_kernel" not in name:
            continue                                   # torch's own copies and fills are not part of the C-ABI call
        key = ("conv" if "conv3x3_mfma_kernel" in name or "lpips_conv_direct" in name else
               "bias_relu_pool" if "lpips_bias_relu" in name else "distance" if "lpips_distance" in name else "other")
        groups[key] += ns
    tot = sum(groups.values())
    return {"kernel_ms_total": tot / 1e6, "share": {k: v / tot for k, v in groups.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=83)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=2)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_shares(args.kernel_stats), indent=1))
        return
    assert torch.cuda.is_available(), "time_lpips.py needs a ROCm GPU"
    import sifsr
    from tests import lpips_reference as R
    N, H, W = args.pairs, args.size, args.size
    sd, lin = R.state_dicts()
    model = sifsr.lpips.LPIPS(sd, lin, reduction="none")
    a, b = R.rasters(N, H, W, seed=1)
    A, B = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    call = lambda: model.pairs(A, B)
    if args.profile_pass:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        return
    rows = call()
    torch.cuda.synchronize()
    assert torch.isfinite(rows).all()
    t = timed(call, args.runs, args.warmup)
    flops = conv_flops_per_pair(H, W) * N
    result = {"device": torch.cuda.get_device_name(0), "pairs": N, "size": [H, W], "pairs_per_call": min(N, sifsr.lpips.max_pairs(H, W)),
              "gpu": t, "gpu_ms_per_pair": t["median_ms"] / N, "conv_gflop_per_pair": flops / N / 1e9,
              "achieved_fp32_tflops_end_to_end": flops / (t["median_ms"] * 1e-3) / 1e12, "peak_fp32_tflops": PEAK_FP32_TFLOPS}
    result["share_of_peak_end_to_end"] = result["achieved_fp32_tflops_end_to_end"] / PEAK_FP32_TFLOPS
    result["lpips_mean"] = float(rows[:, 5].mean())
    # the CPU torch fp32 restatement on this host: what the reference does today
    n = max(1, min(args.cpu_pairs, N))
    R.pair_terms(a[:1], b[:1], dtype=torch.float32)
    t0 = time.perf_counter()
    cpu = R.pair_terms(a[:n], b[:n], dtype=torch.float32)
    result["cpu_fp32_ms_per_pair"] = (time.perf_counter() - t0) * 1e3 / n
    result["cpu_threads"] = torch.get_num_threads()
    result["max_rel_dev_gpu_vs_cpu_fp32"] = float(np.max(np.abs(rows[:n].cpu().numpy() - cpu) / np.abs(cpu)))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
