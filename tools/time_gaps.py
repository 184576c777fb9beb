#!/usr/bin/env python3
"""Time gap-aware whole-granule prediction (sifsr/gaps.py) on one MODIS-sized granule: 1200 x 1200 LST,
4800 x 4800 NDVI, window 64 / overlap 16 / covering (625 tiles), batch 256.

    python tools/time_gaps.py [--runs 30] [--warmup 5] [--out FILE.json]

Scenarios: 0 %, about 35 % and about 60 % of the LST pixels invalid, in blobs.  Blob generator (seeded): a 10 x 10 field of
N(0, 1) draws (np.random.RandomState(seed)), enlarged to 1200 x 1200 by bicubic interpolation (torch, align_corners=False); the
pixels below the field's `fraction` quantile are set to 0 K -- smooth blobs a few hundred pixels across, like cloud decks.

Per scenario: median / minimum / maximum over `runs` calls (after `warmup`) between HIP events on the current stream of
  * `predict_granule_gaps`, the whole call (it holds one host synchronisation, the read of the active count),
  * each of the four entry points alone (sifsrg_fill, sifsrg_tiles_select, sifsrg_tiles_prepare, sifsrg_tiles_blend),
  * `predict_granule` on the same raster with the same layout -- the yardstick: that path is unchanged by this row, so the call
    timed here is the previous revision's,
and n_active / n_tiles.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATS = {"mean_lst": 307.2378, "std_lst": 5.5698, "mean_ndvi": 0.6452, "std_ndvi": 0.1683}
WINDOW, OVERLAP, COVER, BATCH = 64, 16, True, 256


def blobs(seed, h, fraction):
    """bool (h, h): True = invalid, about `fraction` of the pixels"""
    if fraction <= 0:
        return np.zeros((h, h), bool)
    coarse = torch.from_numpy(np.random.RandomState(seed).standard_normal((1, 1, 10, 10)).astype(np.float32))
    field = torch.nn.functional.interpolate(coarse, size=(h, h), mode="bicubic", align_corners=False)[0, 0].numpy()
    return field < np.quantile(field, fraction)


def granule(seed, h, fraction):
    rs = np.random.RandomState(seed)
    lst = (rs.standard_normal((h, h)) * 5.5 + 307).astype(np.float32)
    ndvi = np.clip(rs.standard_normal((4 * h, 4 * h)) * 0.3 + 0.5, -1, 1).astype(np.float32)
    lst[blobs(seed + 1, h, fraction)] = 0.0
    return lst, ndvi


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
    ap.add_argument("--size", type=int, default=1200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_gaps.py needs a ROCm GPU"
    import sifsr
    from sifsr import gaps as G
    L = sifsr._lib
    S = lambda: torch.cuda.current_stream().cuda_stream
    h = args.size
    torch.manual_seed(0)
    model = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda().eval()
    lay = (WINDOW, OVERLAP, 1)
    m = (float(STATS["mean_lst"]), float(STATS["std_lst"]), float(STATS["mean_ndvi"]), float(STATS["std_ndvi"]))
    result = {"device": torch.cuda.get_device_name(0), "granule": [h, h], "window": WINDOW, "overlap": OVERLAP, "cover_edges": COVER,
              "batch": BATCH, "scenarios": {}}
    for name, fraction in (("gaps_0", 0.0), ("gaps_35", 0.35), ("gaps_60", 0.60)):
        lst_np, ndvi_np = granule(1, h, fraction)
        lst, ndvi = torch.from_numpy(lst_np).cuda(), torch.from_numpy(ndvi_np).cuda()
        out, info = G.predict_granule_gaps(model, lst, ndvi, STATS, window=WINDOW, batch=BATCH, overlap=OVERLAP, cover_edges=COVER,
                                           return_info=True)
        n, T = info["n_active"], info["n_tiles"]
        filled, valid = G.fill_gaps(lst)
        slot, active, n_dev = G.select_tiles(valid, WINDOW, OVERLAP, COVER)
        need = L.call("sifsrg_fill_workspace_bytes", h, h)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        x = torch.empty((max(n, 1), 2, 4 * WINDOW, 4 * WINDOW), device="cuda")
        sr = torch.randn((max(n, 1), 1, 4 * WINDOW, 4 * WINDOW), device="cuda")
        calls = {
            "predict_granule_gaps": lambda: G.predict_granule_gaps(model, lst, ndvi, STATS, window=WINDOW, batch=BATCH, overlap=OVERLAP,
                                                                   cover_edges=COVER),
            "predict_granule": lambda: sifsr.predict.predict_granule(model, lst, ndvi, STATS, window=WINDOW, batch=BATCH,
                                                                     overlap=OVERLAP, cover_edges=COVER),
            "fill": lambda: L.call("sifsrg_fill", lst, None, filled, valid, ws, need, h, h, S()),
            "select": lambda: L.call("sifsrg_tiles_select", valid, slot, active, n_dev, h, h, *lay, S()),
            "prepare": lambda: L.call("sifsrg_tiles_prepare", filled, ndvi, x, active, n_dev, x.shape[0], h, h, *lay, *m, 1, S()),
            "blend": lambda: L.call("sifsrg_tiles_blend", sr, slot, valid, out, h, h, *lay, m[0], m[1], float("nan"), S()),
        }
        sc = {k: timed(f, args.runs, args.warmup) for k, f in calls.items()}
        sc.update(invalid_fraction=float((valid == 0).float().mean()), n_active=n, n_tiles=T, active_share=n / T,
                  gaps_over_plain=sc["predict_granule_gaps"]["median_ms"] / sc["predict_granule"]["median_ms"])
        result["scenarios"][name] = sc
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
