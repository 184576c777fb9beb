#!/usr/bin/env python3
"""Golden vectors for the classical sharpening baselines at integer scales other than 4: the reference's own
TsHARP, ATPRK and AATPRK (utils.py:854-1606, `iscale` throughout) at scale 2 and scale 3 on seeded 16x16 coarse cases.  Run in the
BUILD container only (needs the reference checkout, which never travels to the GPU box; about a minute: the reference's nested
loops are s^4 per pair of block pixels, so both scales together cost less than one x4 call):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rbaselines.py            # writes the .npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rbaselines.py --screen   # prints the seeds that meet the conditions

It is tests/golden/make_golden_baselines.py with the scale as a parameter:

  1. imports the reference's utils.py through make_golden.import_reference().  Local to this generator: an exact nearest `resize`
     by an integer factor on the cv2 stub (what cv2.INTER_NEAREST gives), and recorders around us.opt.curve_fit (Gamma_coarse and
     both fits) and around np.dot (the s^2 rows of the reference's own kriging weights);
  2. runs us.TsHARP, us.ATPRK and us.AATPRK (min_T = 273, scc = 926) on float64 arrays holding float32 values;
  3. asserts the x4 generator's conditions: fit 2 finite and positive, every kriging output finite, and ATPRK rerun from the start
     (sill, ran) = (9, 1300) instead of (7, 1000) moves the image by less than 1e-4 K;
  4. writes inputs, outputs, Gamma_coarse, both fits and the weights to tests/golden/golden_rbaselines_v1.npz (data only), keys
     s<scale>_c<case>_<what>.

Cases per scale, the kinds of the x4 golden built by its recipe: 0 and 1 for all three methods (finite indices; case 0 with a 2x3
block of lst == 0), case 2 for TsHARP only (the zero block, three coarse pixels below min_T, one NaN in ndvi_coarse, an s x s
block of NaN in ndvi_fine that straddles cells and overlaps the zero block).  NaN indices in the kriging methods are not pinned.
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
SCALES = (2, 3)
# screened (--screen): both fits of both kriging methods converge from either start, by the reference alone.  They are the x4
# golden's seeds but for case 1 at scale 3: from (9, 1300) the reference's second fit on seed 16 runs off to a sill of 1e7 and
# its image moves by 6e-2 K, so the next seed that meets the conditions stands in.
SEEDS = {2: (15, 16, 13), 3: (15, 17, 13)}


def nan_block(s):
    """the s x s block of NaN fine indices of case 2: rows of cells 5 and 6, columns that reach into the zero block (cells 8..10)"""
    return slice(5 * s + 1, 6 * s + 1), slice(11 * s - 2, 12 * s - 2)


def make_case(us, s, seed, zero_block, tsharp_extras):
    n = 16 * s
    rs = np.random.RandomState(seed)
    ndvi = np.clip(0.35 + 4.0 * gaussian_filter(rs.standard_normal((n, n)), 3.0) + 0.02 * rs.standard_normal((n, n)), -1, 1)
    ndvi = ndvi.astype(np.float32).astype(np.float64)
    ndvi_c = us.downsampling_img(ndvi, (s, s)).astype(np.float32).astype(np.float64)
    lst = 310.0 - 12.0 * ndvi_c + 15.0 * gaussian_filter(rs.standard_normal((16, 16)), 2.0) + 0.3 * rs.standard_normal((16, 16))
    lst = lst.astype(np.float32).astype(np.float64)
    if zero_block:
        lst[5:7, 8:11] = 0.0
    if tsharp_extras:
        lst[3, 4], lst[12, 2], lst[9, 13] = 270.0, 265.5, 272.875
        ndvi_c[10, 5] = np.nan
        ndvi[nan_block(s)] = np.nan
    return lst, ndvi_c, ndvi


class Runner:
    def __init__(self, us):
        self.us, self.fits, self.rows = us, [], []
        self.real_fit, self.real_dot = us.opt.curve_fit, np.dot
        cv2 = sys.modules["cv2"]
        cv2.INTER_NEAREST = 0

        def resize(img, dsize, interpolation=None):
            fy, fx = dsize[1] // img.shape[0], dsize[0] // img.shape[1]
            assert fy == fx >= 1 and (dsize[1], dsize[0]) == (fy * img.shape[0], fx * img.shape[1])
            return np.repeat(np.repeat(img, fy, axis=0), fx, axis=1).copy()
        cv2.resize = resize

    def _curve_fit(self, f, xdata, ydata, p0, **kw):
        popt, pcov = self.real_fit(f, xdata, ydata, p0, **kw)
        self.fits.append((np.array(xdata, dtype=np.float64), np.array(ydata, dtype=np.float64), np.array(p0, dtype=np.float64),
                          np.array(popt, dtype=np.float64)))
        return popt, pcov

    def _dot(self, a, b, *args, **kw):
        out = self.real_dot(a, b, *args, **kw)
        if np.shape(a) == (26, 26) and np.shape(b) == (26,):
            self.rows.append(np.array(out[:25], dtype=np.float64))
        return out

    def __call__(self, fn, s, *a, **kw):
        fits, rows = self.fits, self.rows
        del fits[:], rows[:]
        self.us.opt.curve_fit, np.dot = self._curve_fit, self._dot
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                img = fn(*[np.array(x) for x in a], **kw)
        finally:
            self.us.opt.curve_fit, np.dot = self.real_fit, self.real_dot
        rec = {"image": np.asarray(img, dtype=np.float64)}
        if fits:
            assert len(fits) == 2 and len(rows) == s * s
            assert np.array_equal(fits[0][1], fits[1][1]) and np.array_equal(fits[0][3], fits[1][2])
            rec.update(distances=fits[0][0], gamma=fits[0][1], fit1=fits[0][3], fit2=fits[1][3], lambdas=np.stack(rows))
            assert np.isfinite(rec["fit2"]).all() and (rec["fit2"] > 0).all(), rec["fit2"]
            assert np.isfinite(rec["image"]).all()
        return rec


def kriging_case(run, us, s, lst, ndvi_c, ndvi):
    """-> {key suffix: array} of both kriging methods and the restart; raises where a condition of the generator fails"""
    out = {}
    for name, fn in (("atprk", us.ATPRK), ("aatprk", us.AATPRK)):
        rec = run(fn, s, lst, ndvi_c, ndvi, s, SCC, min_T=MIN_T)
        for k in ("image", "gamma", "fit1", "fit2", "lambdas"):
            out[name + ("" if k == "image" else "_" + k)] = rec[k]
        out["distances"] = rec["distances"]
        print(f"    {name} fit1 {rec['fit1']} fit2 {rec['fit2']}", flush=True)
    again = run(us.ATPRK, s, lst, ndvi_c, ndvi, s, SCC, sill=9, ran=1300, min_T=MIN_T)
    moved = float(np.abs(again["image"] - out["atprk"]).max())
    print(f"    ATPRK from (9, 1300): fit1 {again['fit1']} fit2 {again['fit2']}, image moved by {moved:.3e} K", flush=True)
    assert moved < 1e-4, moved
    out["atprk_restart_moved"] = moved
    return out


def screen(run, us, first=13, last=30):
    """per scale and case kind, the first seed from `first` on which the reference alone meets the conditions"""
    for s in SCALES:
        for zero_block in (True, False):
            for seed in range(first, last):
                lst, ndvi_c, ndvi = make_case(us, s, seed, zero_block, False)
                try:
                    kriging_case(run, us, s, lst, ndvi_c, ndvi)
                    print(f"scale {s} zero_block {zero_block}: seed {seed} PASSES", flush=True)
                    break
                except (AssertionError, RuntimeError) as e:    # a seed on which the reference does not meet the conditions
                    print(f"scale {s} zero_block {zero_block}: seed {seed} fails: {type(e).__name__} {e}", flush=True)


def main():
    from make_golden import import_reference
    _, us = import_reference()
    run = Runner(us)
    if "--screen" in sys.argv:
        return screen(run, us)
    out = {"min_T": MIN_T, "scc": SCC, "scales": np.array(SCALES)}
    for s in SCALES:
        out[f"s{s}_seeds"] = np.array(SEEDS[s])
        for i, seed in enumerate(SEEDS[s]):
            lst, ndvi_c, ndvi = make_case(us, s, seed, zero_block=i in (0, 2), tsharp_extras=i == 2)
            pre = f"s{s}_c{i}_"
            out[pre + "lst"], out[pre + "ndvi_coarse"], out[pre + "ndvi_fine"] = (a.astype(np.float32) for a in (lst, ndvi_c, ndvi))
            ts = run(us.TsHARP, s, lst, ndvi_c, ndvi, s, min_T=MIN_T)
            out[pre + "tsharp"] = ts["image"]
            print(f"scale {s} case {i}: TsHARP done, {int(np.isnan(ts['image']).sum())} NaN pixels", flush=True)
            if i == 2:
                assert np.isnan(ts["image"]).sum() >= 2 * s * s
                continue
            assert np.isfinite(ts["image"]).all()
            for k, v in kriging_case(run, us, s, lst, ndvi_c, ndvi).items():
                if k == "distances":
                    out["distances"] = v
                else:
                    out[pre + k] = v
    path = os.path.join(HERE, "golden_rbaselines_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
