#!/usr/bin/env python3
"""Time fine-tuning with frozen BatchNorm statistics (sifsr/adapt.py, include/sifsr_adapt.h).

    python tools/time_adapt.py [--runs 10] [--warmup 3] [--size 1200] [--steps 20] [--batches 16,64] [--out FILE.json]

Reported, median / minimum / maximum over `runs` calls after `warmup`, between HIP events on the current stream, profiler off:
  * `sifsra_conv_in_dgrad` alone at B = 64, 256 x 256, with the bytes it moves (B H W 136) as GB/s, beside
    `sifsr_conv_in_bn_relu_bwd` (BatchNorm-backward reduce + finalize + the fused first-layer weight gradient) on the same tensors;
  * one optimisation step (forward + masked loss + backward + Adam, `train.train_step`) at each batch size, 256 x 256: the ordinary
    batch-statistics step, the frozen step, and the frozen step with the input gradient requested;
  * `adapt.adapt_granule` (`steps` steps at batch 16) on a `size` x `size` granule with the synthetic gaps of tools/time_gaps.py
    (35 % invalid), beside `predict_granule_gaps` on the same granule.
No ratio is asserted.  Nothing is fetched; all inputs are seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_gaps import BATCH, COVER, OVERLAP, STATS, WINDOW, granule, timed  # noqa: E402


def op_level(L, B, H, W, runs, warmup):
    g, y = torch.randn(B, H, W, 16, device="cuda"), torch.randn(B, H, W, 16, device="cuda")
    x = torch.randn(B, 2, H, W, device="cuda")
    scale, shift = torch.rand(16, device="cuda") + 0.5, 0.1 * torch.randn(16, device="cuda")
    mean, invstd = 0.1 * torch.randn(16, device="cuda"), torch.rand(16, device="cuda") + 0.5
    coef = torch.cat((scale.double(), 0.01 * torch.randn(32, device="cuda").double()))
    w = torch.randn(16, 2, 3, 3, device="cuda") / 3
    dx = torch.empty_like(x)
    S = torch.cuda.current_stream().cuda_stream
    r = {"conv_in_dgrad": timed(lambda: L.call("sifsra_conv_in_dgrad", g, y, scale, shift, coef, w, dx, B, H, W, S), runs, warmup)}
    r["conv_in_dgrad"]["bytes"] = B * H * W * 136
    r["conv_in_dgrad"]["GB_per_s"] = r["conv_in_dgrad"]["bytes"] / r["conv_in_dgrad"]["median_ms"] / 1e6
    # the yardstick: sifsr_conv_in_bn_relu_bwd = BatchNorm-backward reduce + finalize + conv_in_wgrad_fused on the same (g, y) plus x
    scratch = torch.empty(1024 * 288, device="cuda")
    dgamma, dbeta, dw = torch.empty(16, device="cuda"), torch.empty(16, device="cuda"), torch.empty(288, device="cuda")
    coef2 = torch.empty(48, dtype=torch.float64, device="cuda")
    r["conv_in_bn_relu_bwd_chain"] = timed(lambda: L.call("sifsr_conv_in_bn_relu_bwd", x, g, y, scale, shift, mean, invstd, scratch, 1024, dw,
                                                          dgamma, dbeta, coef2, B, H, W, S), runs, warmup)
    return r


def steps(sifsr, B, runs, warmup):
    from oracle import sif_oracle as O
    lst, lst_up, ndvi = (t.cuda() for t in O.synthetic_batch(3, B))
    valid = (torch.rand(B, 1, 64, 64, device="cuda") > 0.3).to(torch.uint8)
    n_valid = valid.sum().to(torch.int64)
    out = {}
    for name, frozen, dx in (("training_step", False, False), ("frozen_step", True, False), ("frozen_step_with_dx", True, True)):
        torch.manual_seed(0)
        m = sifsr.ModelB_2(2).cuda()
        m.bn_frozen = frozen
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-5)
        up = lst_up.clone().requires_grad_(True) if dx else lst_up
        out[name] = timed(lambda: sifsr.train.train_step(m, opt, lst, up, ndvi, STATS, 0.5, -0.25, "sr2", valid=valid, n_valid=n_valid),
                          runs, warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_adapt.py needs a ROCm GPU"
    import sifsr
    from sifsr import _lib as L
    result = {"device": torch.cuda.get_device_name(0), "op_B64_256x256": op_level(L, 64, 256, 256, args.runs, args.warmup)}
    for B in (int(b) for b in args.batches.split(",") if b):
        result[f"step_B{B}_256x256"] = steps(sifsr, B, args.runs, args.warmup)
    lst, ndvi = (torch.from_numpy(a).cuda() for a in granule(0, args.size, 0.35))
    torch.manual_seed(0)
    model = sifsr.ModelB_2(2).cuda()
    res = sifsr.adapt.adapt_granule(model, lst, ndvi, STATS, steps=1, batch=16)
    g = {"n_active": res.n_active, "steps": args.steps, "batch": 16}
    g["adapt_granule"] = timed(lambda: sifsr.adapt.adapt_granule(model, lst, ndvi, STATS, steps=args.steps, batch=16), args.runs, args.warmup)
    g["predict_granule_gaps"] = timed(lambda: sifsr.gaps.predict_granule_gaps(model, lst, ndvi, STATS, window=WINDOW, batch=BATCH,
                                                                              overlap=OVERLAP, cover_edges=COVER), args.runs, args.warmup)
    result[f"granule_{args.size}"] = g
    print(json.dumps(result, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
