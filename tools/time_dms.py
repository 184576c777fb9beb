#!/usr/bin/env python3
"""Time the DMS sharpener (include/sifsr_dms.h) at the two sizes its users run: the 83 ASTER pairs of the
comparison as one batch (64 x 64 LST -> 256 x 256) and one MODIS-sized granule (1200 x 1200 NDVI, 300 x 300 LST).

    python tools/time_dms.py [--runs 10] [--warmup 3] [--estimators 10] [--out FILE.json]

Reported, median / minimum / maximum over `runs` calls after `warmup`, between HIP events on the current stream:
  * `dms` whole (draw, sorts, fit, prediction, correction), `dms_model` (stages 1-3 with the torch.sort / randint plumbing) and
    `dms_apply` (stages 4-5) on their own,
  * the entry points alone: `sifsrd_fit` (B x E workgroups: the stage with little parallelism), `sifsrd_predict`,
    `sifsrd_aggregate` + `sifsrd_correct`, with the bytes the two raster passes must move and the GB/s that makes.
The rasters are seeded smooth fields with noise; nothing is fetched.  Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_gaps import timed  # noqa: E402


def fields(B, h, w, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    yy = torch.arange(4 * h, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(4 * w, device="cuda", dtype=torch.float32)[None, :]
    ph = torch.rand((B, 3, 1, 1), generator=g, device="cuda") * 6.283
    nf = 0.4 + 0.3 * torch.sin(yy / 37 + ph[:, 0]) * torch.cos(xx / 29 + ph[:, 1]) + 0.12 * torch.sin(yy / 11 + xx / 13 + ph[:, 2]) \
        + 0.03 * torch.randn((B, 4 * h, 4 * w), generator=g, device="cuda")
    nf = nf.clamp(-1, 1)[:, None].contiguous()
    lst = 312 - 14 * torch.nn.functional.avg_pool2d(nf, 4) + 0.4 * torch.randn((B, 1, h, w), generator=g, device="cuda")
    return lst.contiguous(), nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--estimators", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_dms.py needs a ROCm GPU"
    import sifsr
    from sifsr import baselines as BL
    L = sifsr._lib
    S = lambda: torch.cuda.current_stream().cuda_stream
    E = args.estimators
    result = {"device": torch.cuda.get_device_name(0), "estimators": E, "cases": {}}
    for name, (B, h, w) in (("aster_83_pairs", (83, 64, 64)), ("granule_1200", (1, 300, 300))):
        lst, nf = fields(B, h, w, 1)
        model = BL.dms_model(lst, nf, n_estimators=E, seed=0)
        N = h * w
        # the fit's own inputs, as dms_model builds them
        ts = BL.dms_training_set(lst, nf)
        inf32 = torch.full((), float("inf"), device="cuda")
        perm = torch.sort(torch.where(ts["good"], ts["x"].float(), inf32), dim=1, stable=True).indices
        xs, ws = ts["x"].gather(1, perm).contiguous(), ts["weight"].gather(1, perm).contiguous()
        ys = lst.reshape(B, N).double().gather(1, perm).contiguous()
        cs = model["counts"].gather(2, perm[:, None, :].expand(B, E, N)).contiguous()
        scratch = torch.empty(L.call("sifsrd_fit_scratch_bytes", B, E, N), dtype=torch.uint8, device="cuda")
        thr, nl, lf = (torch.empty_like(model[k]) for k in ("thresholds", "nleaf", "leaves"))
        sr, out = torch.empty_like(nf), torch.empty_like(nf)
        m4 = torch.empty((B, h, w), dtype=torch.float64, device="cuda")

        def correct():
            L.call("sifsrd_aggregate", sr, m4, None, B, h, w, 1, S())
            L.call("sifsrd_correct", lst, sr, m4, out, B, h, w, S())

        calls = {"dms": lambda: BL.dms(lst, nf, n_estimators=E, seed=0),
                 "dms_model": lambda: BL.dms_model(lst, nf, n_estimators=E, seed=0),
                 "dms_apply": lambda: BL.dms_apply(model, lst, nf),
                 "sifsrd_fit": lambda: L.call("sifsrd_fit", xs, ys, ws, cs, ts["n_train"], scratch, thr, nl, lf, B, E, N, S()),
                 "sifsrd_predict": lambda: L.call("sifsrd_predict", nf, model["thresholds"], model["nleaf"], model["leaves"], sr,
                                                  B, E, h, w, S()),
                 "sifsrd_aggregate_correct": correct}
        t = {k: timed(f, args.runs, args.warmup) for k, f in calls.items()}
        fine = 16 * B * N * 4
        t["sifsrd_predict"]["bytes"] = 2 * fine
        t["sifsrd_predict"]["gbs"] = 2 * fine / t["sifsrd_predict"]["median_ms"] / 1e6
        t["sifsrd_aggregate_correct"]["bytes"] = 4 * fine
        t["sifsrd_aggregate_correct"]["gbs"] = 4 * fine / t["sifsrd_aggregate_correct"]["median_ms"] / 1e6
        result["cases"][name] = {"lst": [B, h, w], "fit_workgroups": B * E, "n_train_mean": float(ts["n_train"].float().mean()),
                                 "leaves_mean": float(model["nleaf"].float().mean()), "calls": t}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
