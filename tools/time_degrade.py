#!/usr/bin/env python3
"""Time the sensor model at any ratio (include/sifsr_degrade.h) on one ASTER-sized scene, 700 x 830 at 90 m, and on
a batch of 64 such scenes.

    python tools/time_degrade.py [--height 700] [--width 830] [--batch 64] [--runs 10] [--warmup 3] [--out FILE.json]

Reported, median / minimum / maximum over `runs` calls after `warmup`, between HIP events on the current stream, profiler off:
  * `sifsr.degrade.aster_to_coarse` (-> 70 x 82), `aster_to_fine` (-> 274 x 324) and `simulate_pair` (both, with a validity map),
    for one scene and for the batch; each call includes its workspace and output allocations from the caching allocator;
  * for comparison the reference's own three-call composition on the same device in torch-ROCm: F.pad(reflect), F.conv2d with the
    (2 hw + 1)^2 fp32 kernel and padding="same", F.interpolate(scale_factor=1/factor, mode="bicubic"), for both factors and both
    batch sizes; and the largest difference between the two results, as a check that they compute the same thing.
No ratio is asserted.  Nothing is fetched; the scene is seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_gaps import timed  # noqa: E402


def torch_composition(x, factor, mtf=0.1):
    """utils.py:1759-1830 on a (B,1,H,W) device tensor"""
    from dropin.utils import generate_psf_kernel
    k = torch.from_numpy(generate_psf_kernel(1.0, factor, mtf, None)).to(x.device)
    hw = (k.shape[-1] - 1) // 2
    x = F.pad(x, (hw, hw, hw, hw), mode="reflect")
    x = F.conv2d(x, k[None, None], padding="same")
    return F.interpolate(x, scale_factor=1 / factor, mode="bicubic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=700)
    ap.add_argument("--width", type=int, default=830)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_degrade.py needs a ROCm GPU"
    import sifsr
    from sifsr import degrade as D
    H, W = args.height, args.width
    rs = np.random.RandomState(0)
    y, x = np.mgrid[0:H, 0:W]
    scene = (300.0 + 6.0 * np.sin(0.05 * x) * np.cos(0.07 * y) + rs.standard_normal((H, W))).astype(np.float32)
    valid = (np.abs((x - W / 2) * 0.6 + (y - H / 2)) < 0.45 * H) & (np.abs((y - H / 2) * 0.6 - (x - W / 2)) < 0.45 * W)
    one = torch.from_numpy(scene).cuda()
    many = one[None].repeat(args.batch, 1, 1).contiguous()
    v_one = torch.from_numpy(valid.astype(np.uint8)).cuda()
    result = {"device": torch.cuda.get_device_name(0), "scene": [H, W], "batch": args.batch, "valid_share": float(valid.mean()),
              "coarse": list(D.output_shape(H, W, D.COARSE_FACTOR)), "fine": list(D.output_shape(H, W, D.FINE_FACTOR)), "sifsr": {}, "torch": {}}
    for tag, t, v in (("one", one, v_one), (f"batch{args.batch}", many, v_one)):
        calls = {"aster_to_coarse": lambda t=t: D.aster_to_coarse(t), "aster_to_fine": lambda t=t: D.aster_to_fine(t),
                 "simulate_pair": lambda t=t, v=v: D.simulate_pair(t, v)}
        result["sifsr"][tag] = {k: timed(f, args.runs, args.warmup) for k, f in calls.items()}
        t4 = t[None, None] if t.dim() == 2 else t[:, None]
        ref = {"coarse": lambda t4=t4: torch_composition(t4, D.COARSE_FACTOR), "fine": lambda t4=t4: torch_composition(t4, D.FINE_FACTOR),
               "pair": lambda t4=t4: (torch_composition(t4, D.COARSE_FACTOR), torch_composition(t4, D.FINE_FACTOR))}
        result["torch"][tag] = {k: timed(f, args.runs, args.warmup) for k, f in ref.items()}
    result["max_abs_difference_K"] = {"coarse": float((D.aster_to_coarse(one) - torch_composition(one[None, None], D.COARSE_FACTOR)[0, 0]).abs().max()),
                                      "fine": float((D.aster_to_fine(one) - torch_composition(one[None, None], D.FINE_FACTOR)[0, 0]).abs().max())}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
