#!/usr/bin/env python3
"""Time the patch mining of sifsr/products.py on one MODIS-sized granule (1200 x 1200 LST, 4800 x 4800 NIR / Red).

    python tools/time_products.py [--runs 30] [--warmup 5] [--out FILE.json]

Per scenario (every window accepted; every other full window rejected by one LST fill pixel): the median, minimum and maximum of
`PatchMiner.add` (census + select + gather, enqueue to completion) and of each entry point alone, between HIP events on the
current stream; next to them the bytes the pass has to move, the time those bytes take at the HBM peak of 8 TB/s, and the
single-core time of the NumPy restatement tests/products_reference.py on the same arrays.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def granule(seed, h=1200, reject_every_other=False, ws=64):
    rs = np.random.RandomState(seed)
    lst = rs.randint(13000, 16500, (h, h)).astype(np.uint16)
    nir = rs.randint(1, 6000, (4 * h, 4 * h)).astype(np.int16)
    red = rs.randint(1, 3000, (4 * h, 4 * h)).astype(np.int16)
    if reject_every_other:
        for n, (r, c) in enumerate((r, c) for c in range(0, h - ws + 1, ws) for r in range(0, h - ws + 1, ws)):
            if n % 2:
                lst[r + 7, c + 9] = 0
    return lst, nir, red


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
    assert torch.cuda.is_available(), "time_products.py needs a ROCm GPU"
    import sifsr
    from sifsr import products as P
    from tests import products_reference as R
    L = sifsr._lib
    S = lambda: torch.cuda.current_stream().cuda_stream
    h = 1200
    in_bytes = h * h * 2 + 2 * (4 * h) ** 2 * 2                       # census reads LST, NIR, Red once (QC mode 0)
    patch_bytes = 64 * 64 * (2 + 4) + 256 * 256 * (2 * 2 + 4) + 64    # gather: raw window in, both patches and one moment row out
    result = {"device": torch.cuda.get_device_name(0), "granule": [h, h], "scenarios": {}}
    for name, half in (("all_accepted", False), ("half_accepted", True)):
        lst, nir, red = granule(1, h, half)
        d = [torch.from_numpy(a).cuda() for a in (lst, nir, red)]
        miner = P.PatchMiner()
        g = miner.add(*d)
        n = int(g["n_accepted"].item())
        nwin, cap = P.window_counts(h, h)

        def add():
            miner._granules.clear()                                   # keep one granule's buffers alive, not `runs` of them
            miner.add(*d)

        calls = {
            "add": add,
            "census": lambda: L.call("sifsrp_census", d[0], None, d[1], d[2], g["counts"], h, h, 64, 0, S()),
            "select": lambda: L.call("sifsrp_select", g["counts"], g["index"], g["n_accepted"], h, h, 64, 0, cap, S()),
            "gather": lambda: L.call("sifsrp_gather", d[0], d[1], d[2], g["index"], g["n_accepted"], g["lst"], g["ndvi"], g["moments"],
                                     h, h, 64, cap, S()),
        }
        sc = {k: timed(f, args.runs, args.warmup) for k, f in calls.items()}
        total = in_bytes + n * (patch_bytes + 0)
        sc.update(accepted=n, windows=nwin, full_windows=cap, bytes_census=in_bytes, bytes_gather=n * patch_bytes,
                  bytes_total=in_bytes + n * patch_bytes, hbm_floor_ms=1e3 * total / HBM_PEAK,
                  add_GBps=total / (sc["add"]["median_ms"] * 1e-3) / 1e9)
        t0 = time.perf_counter()
        counts, index, *_ = R.mine({"lst_raw": lst, "qc": None, "nir": nir, "red": red})
        sc["restatement_single_core_s"] = time.perf_counter() - t0
        assert len(index) == n and np.array_equal(g["index"][:n].cpu().numpy(), index)
        result["scenarios"][name] = sc
    lst, nir, red = granule(1, h)
    d = [torch.from_numpy(a).cuda() for a in (lst, nir, red)]
    result["decode"] = timed(lambda: P.decode(*d), args.runs, args.warmup)
    result["decode"]["bytes"] = h * h * (2 + 4) + (4 * h) ** 2 * (4 + 4)
    result["decode"]["hbm_floor_ms"] = 1e3 * result["decode"]["bytes"] / HBM_PEAK
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
