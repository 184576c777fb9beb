#!/usr/bin/env python3
"""Time the captured step and the captured granule predictors at any ratio beside the eager calls they replay.

    python tools/time_captured.py [--windows 9] [--reps 5] [--warmup 3] [--only step,adapt,predict,gaps] [--side 1200] [--out FILE.json]

Every figure is the median (with minimum and maximum) over `windows` windows of `reps` back-to-back calls between two HIP events on
the current stream, the stream synchronised before and after each window, after `warmup` calls of every variant; the variants of one
workload ALTERNATE window by window inside the one process, so that clock and cache state are shared (`tools/time_sensor.alternating`).
An eager call that synchronises with the host (`predict_granule_gaps`, `adapt_granule`) is timed with its synchronisation: the events
bracket what the stream saw, idle time included.  Profiler off.  No ratio is asserted.  Nothing is fetched; inputs are seeded.

  step      `rloss.train_step` against `rloss.GraphedTrainStep` at (64, 192), batch 8, 16 and 64, unmasked and masked (35 % of the
            cells invalid, counts formed inside)
  adapt     `rloss.adapt_granule` at (64, 192) and `adapt.adapt_granule` at x4: 20 steps x 16 tiles on a `--side`^2 granule with 35 %
            gaps, eager against graphed=True (each call pays its own three warm-up steps and its capture)
  predict   `ratio.predict_granule` against `ratio.GranulePredictor` at (64, 192) and (64, 160), at batch 256 (the captured form
            forwards a whole number of batches: 768 slots for 625 tiles) and at the largest batch that divides the tile count
            (`*_fit`: no padded slot)
  gaps      `predict_granule_gaps` against `GranulePredictor(gaps=True)` at x4 and at (64, 192), on a granule with 35 % gaps (clouds
            of tile size: about an eighth of the tiles inactive) and on a nearly full one, one granule per call and ten back to
            back; `replay_fit` as above

Timing needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_sensor import alternating  # noqa: E402

STATS = {"mean_lst": 307.2378, "std_lst": 5.5698, "mean_ndvi": 0.6452, "std_ndvi": 0.1683}
ALPHA, GAMMA = 0.5, -0.25


def new_model(sifsr, seed=0):
    torch.manual_seed(seed)
    return sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda()


def gappy_granule(side, window, hr, share, seed=0):
    """-> (lst (side, side) [K] with `share` of its pixels 0 K in square clouds of tile size, ndvi at hr / window), on the device"""
    rs = np.random.RandomState(seed)
    lst = rs.uniform(285.0, 325.0, (side, side)).astype(np.float32)
    gap = np.zeros((side, side), bool)
    while gap.mean() < share:
        y, x = rs.randint(0, side), rs.randint(0, side)
        gap[y:y + 2 * window, x:x + 2 * window] = True
    lst[gap] = 0.0
    big = side * hr // window
    ndvi = np.clip(0.5 + 0.3 * rs.standard_normal((big, big)), -1.0, 1.0).astype(np.float32)
    return torch.from_numpy(lst).cuda(), torch.from_numpy(ndvi).cuda()


def step_variants(sifsr, batch, masked, window=64, hr=192):
    from sifsr import ratio, rloss
    out = {}
    lst = torch.randn((batch, 1, window, window), device="cuda")
    up, ndvi = ratio.upsample(lst, (hr, hr)), torch.randn((batch, 1, hr, hr), device="cuda").clamp(-3, 3)
    valid = (torch.rand((batch, 1, window, window), device="cuda") > 0.35).to(torch.uint8) if masked else None
    for name in ("eager", "replay"):
        m = new_model(sifsr)
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-4, capturable=True)
        if name == "eager":
            out[name] = lambda m=m, opt=opt: rloss.train_step(m, opt, lst, up, ndvi, STATS, ALPHA, GAMMA, hr / window, valid=valid)
        else:
            g = rloss.GraphedTrainStep(m, opt, batch, STATS, ALPHA, GAMMA, window, hr, masked=masked)
            out[name] = (lambda g=g: g(lst, up, ndvi, valid)) if masked else (lambda g=g: g(lst, up, ndvi))
            for _ in range(4):
                out[name]()
            assert g.graph is not None
    return out


def adapt_variants(sifsr, side, window, hr):
    lst, ndvi = gappy_granule(side, window, hr, 0.35)
    m = new_model(sifsr).eval()
    kw = dict(steps=20, lr=1e-5, batch=16, overlap=16, cover_edges=True)
    if hr == 4 * window:
        call = lambda graphed: sifsr.adapt.adapt_granule(m, lst, ndvi, STATS, window=window, graphed=graphed, **kw).restore()
    else:
        call = lambda graphed: sifsr.rloss.adapt_granule(m, lst, ndvi, STATS, window, hr, graphed=graphed, **kw).restore()
    return {"eager": lambda: call(False), "graphed": lambda: call(True)}


def fitting_batch(n, top=256):
    """the largest batch <= top that divides the tile count: a captured predictor then has no padded slot"""
    return max(b for b in range(1, top + 1) if n % b == 0)


def predict_variants(sifsr, side, window, hr):
    lst, ndvi = gappy_granule(side, window, hr, 0.0)
    m = new_model(sifsr).eval()
    kw = dict(window=window, hr=hr, overlap=16, cover_edges=True)
    gp = sifsr.ratio.GranulePredictor(m, (side, side), STATS, batch=256, **kw)
    fit = fitting_batch(gp.tiles[0] * gp.tiles[1])
    gf = sifsr.ratio.GranulePredictor(m, (side, side), STATS, batch=fit, **kw)
    note = {"n_tiles": gp.tiles[0] * gp.tiles[1], "slots_forwarded": int(gp.x.shape[0]), "fitting_batch": fit}
    return {"eager": lambda: sifsr.ratio.predict_granule(m, lst, ndvi, STATS, batch=256, **kw), "replay": lambda: gp(lst, ndvi),
            "eager_fit": lambda: sifsr.ratio.predict_granule(m, lst, ndvi, STATS, batch=fit, **kw), "replay_fit": lambda: gf(lst, ndvi)}, note


def gaps_variants(sifsr, side, window, hr, share):
    lst, ndvi = gappy_granule(side, window, hr, share)
    m = new_model(sifsr).eval()
    kw = dict(window=window, overlap=16, cover_edges=True)
    if hr == 4 * window:
        make = lambda batch: sifsr.predict.GranulePredictor(m, (side, side), STATS, gaps=True, batch=batch, **kw)
        eager = lambda: sifsr.predict.predict_granule_gaps(m, lst, ndvi, STATS, batch=256, **kw)
    else:
        make = lambda batch: sifsr.ratio.GranulePredictor(m, (side, side), STATS, hr=hr, gaps=True, batch=batch, **kw)
        eager = lambda: sifsr.ratio.predict_granule_gaps(m, lst, ndvi, STATS, hr=hr, batch=256, **kw)
    gp = make(256)
    _, info = gp(lst, ndvi, return_info=True)
    fit = fitting_batch(info["n_tiles"])
    gf = make(fit)
    note = {"invalid_share": float((lst == 0).float().mean()), "n_active": int(info["n_active"]), "n_tiles": info["n_tiles"],
            "slots_forwarded": int(gp.x.shape[0]), "fitting_batch": fit}

    def ten(fn):
        def run():
            for _ in range(10):
                fn()
        return run

    replay, replay_fit = (lambda: gp(lst, ndvi)), (lambda: gf(lst, ndvi))
    return {"eager": eager, "replay": replay, "replay_fit": replay_fit, "eager_x10": ten(eager), "replay_x10": ten(replay),
            "replay_fit_x10": ten(replay_fit)}, note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="step,adapt,predict,gaps")
    ap.add_argument("--side", type=int, default=1200, help="side of the LST granule (a multiple of 2)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_captured.py needs a ROCm GPU"
    import sifsr
    torch.manual_seed(0)
    only = set(args.only.split(","))
    t = lambda v: alternating(v, args.windows, args.reps, args.warmup)
    result = {"device": torch.cuda.get_device_name(0), "side": args.side}

    def emit(key, value):                                       # (every workload is printed when it is done: a long run shows progress)
        result[key] = value
        print(json.dumps({key: value}), flush=True)

    if "step" in only:
        for batch in (8, 16, 64):
            for masked in (False, True):
                emit(f"step (64,192) batch {batch}{' masked' if masked else ''}", t(step_variants(sifsr, batch, masked)))
    if "adapt" in only:
        for window, hr in ((64, 192), (64, 256)):
            emit(f"adapt_granule ({window},{hr}) 20 x 16", t(adapt_variants(sifsr, args.side, window, hr)))
    if "predict" in only:
        for window, hr in ((64, 192), (64, 160)):
            variants, note = predict_variants(sifsr, args.side, window, hr)
            emit(f"predict_granule ({window},{hr})", {"case": note, "per_call": t(variants)})
    if "gaps" in only:
        for window, hr in ((64, 256), (64, 192)):
            for share in (0.35, 0.02):
                variants, note = gaps_variants(sifsr, args.side, window, hr, share)
                emit(f"predict_granule_gaps ({window},{hr}) {share:.0%} gaps", {"case": note, "per_call": t(variants)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
