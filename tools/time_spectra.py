#!/usr/bin/env python3
"""Time the Fourier scores for rasters of any size (include/sifsr_spectra.h, sifsr/spectra.py) at the size of the
reference's ASTER evaluation: 83 pairs of about 250 x 230 pixels (every pair its own l x c rectangle, none a power of two), seven
methods per pair, and one 1000 x 1000 raster.

    python tools/time_spectra.py [--pairs 83] [--methods 7] [--runs 10] [--warmup 3] [--out FILE.json]

Reported, median / minimum / maximum over `runs` calls after `warmup`, profiler off:
  * `spectral_scores` over all pairs, wall clock from the call to the returned (pairs, K, 6) array: 83 launches chains of K + 2
    rasters each, one read-back per pair and the host algebra;
  * the device part alone, between HIP events on the current stream: the same 83 `sifsrf_fft2_attenuation` chains without the
    read-back;
  * `attenuation_spectra` and `fft2_magnitude` of one 1000 x 1000 raster (two chirp axes, M = 2048), between HIP events.
There is no earlier path for such sizes to compare with.  The rasters are seeded noise around 300 K; the time of a launch does not
depend on the values.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_gaps import timed  # noqa: E402


def wall(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=83)
    ap.add_argument("--methods", type=int, default=7)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_spectra.py needs a ROCm GPU"
    import sifsr
    from sifsr import spectra
    rs = np.random.RandomState(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    sizes = [(int(rs.randint(220, 281)), int(rs.randint(200, 261))) for _ in range(args.pairs)]
    sizes = [(h + ((h & (h - 1)) == 0), w + ((w & (w - 1)) == 0)) for h, w in sizes]       # 256 -> 257: no radix-2 axis
    field = lambda *s: 300 + 5 * torch.randn(s, generator=gen, device="cuda")
    aster = [field(h, w) for h, w in sizes]
    bic = [field(h, w) for h, w in sizes]
    preds = [field(args.methods, h, w) for h, w in sizes]
    stacks = [torch.cat((a[None], b[None], p)) for a, b, p in zip(aster, bic, preds)]
    big = field(1000, 1000)
    t = {"spectral_scores_wall": wall(lambda: spectra.spectral_scores(aster, bic, preds), args.runs, args.warmup),
         "spectra_of_all_pairs_device": timed(lambda: [spectra.attenuation_spectra(s) for s in stacks], args.runs, args.warmup),
         "attenuation_spectra_1000x1000": timed(lambda: spectra.attenuation_spectra(big), args.runs, args.warmup),
         "fft2_magnitude_1000x1000": timed(lambda: spectra.fft2_magnitude(big), args.runs, args.warmup)}
    result = {"device": torch.cuda.get_device_name(0), "pairs": args.pairs, "methods": args.methods,
              "mean_size": [float(np.mean([h for h, _ in sizes])), float(np.mean([w for _, w in sizes]))],
              "rasters": args.pairs * (args.methods + 2), "calls": t,
              "per_pair_ms": t["spectral_scores_wall"]["median_ms"] / args.pairs}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
