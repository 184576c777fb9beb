#!/usr/bin/env python3
"""Golden vectors for the classical sharpening baselines: the reference's own TsHARP, ATPRK and AATPRK
(utils.py:854-1606) on three seeded 16x16 -> 64x64 cases.  Run in the BUILD container only (needs the reference checkout, which
never travels to the GPU box; a few minutes: the reference's nested loops take ~25 s per ATPRK and ~50 s per AATPRK call):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_baselines.py

  1. imports the reference's utils.py through make_golden.import_reference().  Two things are local to this generator: an exact
     x4 nearest `resize` on the cv2 stub (what cv2.INTER_NEAREST gives for an integer factor), and recorders around
     us.opt.curve_fit (xdata, ydata, start and result of each of the two fits per call: the reference's own Gamma_coarse and
     both fits) and around np.dot (the 16 rows of the reference's own kriging weights);
  2. runs us.TsHARP, us.ATPRK and us.AATPRK (min_T = 273, scc = 926) on float64 arrays holding float32 values;
  3. asserts its conditions: fit 2 finite and positive, every kriging output finite, and ATPRK rerun from the start
     (sill, ran) = (9, 1300) instead of (7, 1000) moves the image by less than 1e-4 K (the image does not depend on the fit path);
  4. writes inputs, outputs, Gamma_coarse, both fits and the weights to tests/golden/golden_baselines_v1.npz (data only).

Cases: 0 and 1 for all three methods (finite indices; case 0 with a 2x3 block of lst == 0), case 2 for TsHARP only (the zero
block, three coarse pixels below min_T, one NaN in ndvi_coarse, a 4x4 block of NaN in ndvi_fine).  NaN indices in the kriging
methods are not pinned.
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np
from scipy.ndimage import gaussian_filter

MIN_T, SCC = 273.0, 926.0
SEEDS = (15, 16, 13)        # screened: both fits of both kriging methods converge from either start


def make_case(us, seed, zero_block, tsharp_extras):
    rs = np.random.RandomState(seed)
    ndvi = np.clip(0.35 + 4.0 * gaussian_filter(rs.standard_normal((64, 64)), 3.0) + 0.02 * rs.standard_normal((64, 64)), -1, 1)
    ndvi = ndvi.astype(np.float32).astype(np.float64)
    ndvi_c = us.downsampling_img(ndvi, (4, 4)).astype(np.float32).astype(np.float64)
    lst = 310.0 - 12.0 * ndvi_c + 15.0 * gaussian_filter(rs.standard_normal((16, 16)), 2.0) + 0.3 * rs.standard_normal((16, 16))
    lst = lst.astype(np.float32).astype(np.float64)
    if zero_block:
        lst[5:7, 8:11] = 0.0
    if tsharp_extras:
        lst[3, 4], lst[12, 2], lst[9, 13] = 270.0, 265.5, 272.875
        ndvi_c[10, 5] = np.nan
        ndvi[21:25, 42:46] = np.nan
    return lst, ndvi_c, ndvi


def main():
    from make_golden import import_reference
    _, us = import_reference()
    cv2 = sys.modules["cv2"]
    cv2.INTER_NEAREST = 0

    def resize(img, dsize, interpolation=None):
        assert (dsize[1], dsize[0]) == (4 * img.shape[0], 4 * img.shape[1])
        return np.repeat(np.repeat(img, 4, axis=0), 4, axis=1).copy()
    cv2.resize = resize

    fits, rows = [], []
    real_fit, real_dot = us.opt.curve_fit, np.dot

    def curve_fit(f, xdata, ydata, p0, **kw):
        popt, pcov = real_fit(f, xdata, ydata, p0, **kw)
        fits.append((np.array(xdata, dtype=np.float64), np.array(ydata, dtype=np.float64), np.array(p0, dtype=np.float64),
                     np.array(popt, dtype=np.float64)))
        return popt, pcov

    def dot(a, b, *args, **kw):
        out = real_dot(a, b, *args, **kw)
        if np.shape(a) == (26, 26) and np.shape(b) == (26,):
            rows.append(np.array(out[:25], dtype=np.float64))
        return out

    def run(fn, *a, **kw):
        del fits[:], rows[:]
        us.opt.curve_fit, np.dot = curve_fit, dot
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                img = fn(*[np.array(x) for x in a], **kw)
        finally:
            us.opt.curve_fit, np.dot = real_fit, real_dot
        rec = {"image": np.asarray(img, dtype=np.float64)}
        if fits:
            assert len(fits) == 2 and len(rows) == 16
            assert np.array_equal(fits[0][1], fits[1][1]) and np.array_equal(fits[0][3], fits[1][2])
            rec.update(distances=fits[0][0], gamma=fits[0][1], fit1=fits[0][3], fit2=fits[1][3], lambdas=np.stack(rows))
            assert np.isfinite(rec["fit2"]).all() and (rec["fit2"] > 0).all(), rec["fit2"]
            assert np.isfinite(rec["image"]).all()
        return rec

    out = {"min_T": MIN_T, "scc": SCC, "seeds": np.array(SEEDS)}
    for i, seed in enumerate(SEEDS):
        lst, ndvi_c, ndvi = make_case(us, seed, zero_block=i in (0, 2), tsharp_extras=i == 2)
        out[f"c{i}_lst"], out[f"c{i}_ndvi_coarse"], out[f"c{i}_ndvi_fine"] = (a.astype(np.float32) for a in (lst, ndvi_c, ndvi))
        ts = run(us.TsHARP, lst, ndvi_c, ndvi, 4, min_T=MIN_T)
        out[f"c{i}_tsharp"] = ts["image"]
        print(f"case {i}: TsHARP done, {int(np.isnan(ts['image']).sum())} NaN pixels", flush=True)
        if i == 2:
            assert np.isnan(ts["image"]).sum() >= 32
            continue
        assert np.isfinite(ts["image"]).all()
        for name, fn in (("atprk", us.ATPRK), ("aatprk", us.AATPRK)):
            rec = run(fn, lst, ndvi_c, ndvi, 4, SCC, min_T=MIN_T)
            for k in ("image", "gamma", "fit1", "fit2", "lambdas"):
                out[f"c{i}_{name}" + ("" if k == "image" else "_" + k)] = rec[k]
            out["distances"] = rec["distances"]
            print(f"case {i}: {name} fit1 {rec['fit1']} fit2 {rec['fit2']}", flush=True)
        again = run(us.ATPRK, lst, ndvi_c, ndvi, 4, SCC, sill=9, ran=1300, min_T=MIN_T)
        moved = float(np.abs(again["image"] - out[f"c{i}_atprk"]).max())
        print(f"case {i}: ATPRK from (9, 1300): fit1 {again['fit1']} fit2 {again['fit2']}, image moved by {moved:.3e} K", flush=True)
        assert moved < 1e-4, moved
        out[f"c{i}_atprk_restart_moved"] = moved
    path = os.path.join(HERE, "golden_baselines_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
