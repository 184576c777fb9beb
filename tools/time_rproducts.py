#!/usr/bin/env python3
"""Time patch mining at a ratio (include/sifsr_rproducts.h) beside the x4 miner, and one loader batch beside one step.

    python tools/time_rproducts.py [--windows 9] [--reps 5] [--warmup 3] [--batch 64] [--side 1200] [--out FILE.json]

Every figure is the median (with minimum and maximum) over `windows` windows of `reps` back-to-back calls between two HIP events on
the current stream, the stream synchronised before and after each window, after `warmup` calls of every variant; the variants
ALTERNATE window by window inside the one process, so that clock and cache state are shared (tools/time_sensor.py: `alternating`).

  add_x3, add_x2.5   `rproducts.PatchMiner.add` (census, select, gather and the allocation of the granule's buffers) on a
                     `side` x `side` LST granule at (64, 192) and (64, 160): fine rasters of 3 and 2.5 times the side
  add_x4             `products.PatchMiner.add` on the same LST raster with the fine rasters of 4 times the side
      each also as TB/s of fine bytes read: 2 arrays x 2 bytes x hr^2 x (full windows, the census, + accepted windows, the gather)
  loader_batch       one masked loader batch of `batch` patches at (64, 192): index_select, two z-scores, `ratio.prepare_tiles`,
                     the summed counts
  train_step         one `rloss.train_step` on that batch
No ratio is asserted.  Nothing is fetched; inputs are seeded.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_sensor import alternating  # noqa: E402


def granule(side, p, q, seed, zeros=0.0):
    rs = np.random.RandomState(seed)
    lst = rs.randint(13000, 16500, (side, side)).astype(np.uint16)
    if zeros:
        lst[rs.uniform(size=lst.shape) < zeros] = 0
    fine = side * p // q
    nir, red = rs.randint(1, 6000, (fine, fine)).astype(np.int16), rs.randint(1, 3000, (fine, fine)).astype(np.int16)
    return tuple(torch.from_numpy(a).cuda() for a in (lst, nir, red))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--side", type=int, default=1200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_rproducts.py needs a ROCm GPU"
    import sifsr
    from sifsr import products, rloss, rproducts
    result = {"device": torch.cuda.get_device_name(0), "lst_side": args.side}

    variants, fine_bytes = {}, {}
    for name, hr, (p, q) in (("add_x3", 192, (3, 1)), ("add_x2.5", 160, (5, 2)), ("add_x4", 256, (4, 1))):
        rasters = granule(args.side, p, q, 7)
        miner = products.PatchMiner(64) if hr == 256 else rproducts.PatchMiner(64, hr)

        def add(miner=miner, rasters=rasters):
            miner._granules = []                                               # (the buffers of the call before are released)
            return miner.add(*rasters)

        g = add()
        nfull = products.window_counts(args.side, args.side, 64)[1]
        fine_bytes[name] = 4 * hr * hr * (nfull + int(g["n_accepted"]))
        variants[name] = add
    per_call = alternating(variants, args.windows, args.reps, args.warmup)
    for name, t in per_call.items():
        t["fine_bytes"] = fine_bytes[name]
        for k in ("median", "min", "max"):
            t[f"tb_per_s_at_{k}_ms"] = fine_bytes[name] / (t[f"{k}_ms"] * 1e-3) / 1e12
    result["add"] = per_call

    miner = rproducts.PatchMiner(64, 192, coverage=0.05)
    miner.add(*granule(args.side, 3, 1, 8, zeros=0.01))
    mined = miner.finish()
    stats = mined.statistics(None, valid_only=True)
    loader = mined.masked_loader(None, args.batch, stats, shuffle=False)
    lst, lst_up, ndvi, valid, counts = next(iter(loader))
    torch.manual_seed(0)
    model = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda()
    opt = sifsr.FlatAdam(model.parameters(), lr=1e-4)
    result["batch"] = {"patches": len(mined), "batch": int(lst.shape[0]), "invalid_share": float((valid == 0).float().mean()),
                       "per_call": alternating({"loader_batch": lambda: next(iter(loader)),
                                                "train_step": lambda: rloss.train_step(model, opt, lst, lst_up, ndvi, stats, 0.5, -0.25, 3.0,
                                                                                       valid=valid, counts=counts)},
                                               args.windows, args.reps, args.warmup)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
