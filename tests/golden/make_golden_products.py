#!/usr/bin/env python3
"""Generate tests/golden/golden_products_v1.npz: what the REFERENCE's patch extraction gives on the seeded raw inputs of
tests/products_reference.make_case.  Run in the build container only (needs the reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_products.py

  1. imports the reference's utils.py through make_golden.import_reference() and its process_modis.py beside it (stub modules
     for skimage.morphology only; matplotlib and pandas are installed);
  2. replaces us.read_LST by an array provider (the two lines of read_LST that matter, `astype(np.float32)` and `0.02 * raw`,
     utils.py:335-338, around the case's raw integers; likewise read_NIRRED's `0.0001 * raw`, :424-435) and us.save_GeoTiff by a
     recorder, then runs process_MOD21A1D and process_MOD11A1 THEMSELVES for both coverages: the recorded file names carry k,
     the recorded arrays are the accepted LST patches;
  3. runs us.split and us.split_NIRRed for the window order and the per-window counts, and the acceptance lines of
     find_corresponding_NDVI (process_modis.py:290-305, which cannot run: it globs files) around us.compute_NDVI;
  4. computes statistics.json with the literal construction of data_preparation.py:83-102 over the 'Train' rows of
     data_preparation.py:32-39;
  5. asserts that tests/products_reference.py gives the same, and writes DATA only: shapes and seeds, counts, accepted
     [k, row0, col0] lists, labels, the six statistics, and one sha256 per accepted patch."""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np

from tests import products_reference as R

REF = "/root/reference"
WS = 64
MODES = {0: "process_MOD21A1D", 1: "process_MOD11A1"}


def import_process_modis():
    from make_golden import import_reference
    _, us = import_reference()
    for name in ("skimage.morphology",):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].morphology = sys.modules["skimage.morphology"]
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    import process_modis as pm
    sys.path.remove(REF)
    assert pm.us is us
    return us, pm


def run_process(us, pm, case, mode, coverage):
    """process_MOD21A1D / process_MOD11A1 on the case: -> {k: accepted LST patch}"""
    recorded = {}

    def read_LST(hdf_name, time="day"):
        raw = case["lst_raw"].astype(np.float32)
        return 0.02 * raw, case["qc"].copy(), case["w"], case["h"], "proj", [0.0, 1.0, 0.0, 0.0, 0.0, -1.0]

    def save_GeoTiff(img, fname, projection, geotransform):
        k = int(os.path.basename(fname)[len("granule."):-len(".tiff")])
        assert k not in recorded
        recorded[k] = np.array(img)

    saved = us.read_LST, us.save_GeoTiff, pm.os.makedirs
    us.read_LST, us.save_GeoTiff, pm.os.makedirs = read_LST, save_GeoTiff, lambda *a, **k: None
    try:
        getattr(pm, MODES[mode])("x/granule.hdf", "unused", WS, coverage)
    finally:
        us.read_LST, us.save_GeoTiff, pm.os.makedirs = saved
    return recorded


def reference_windows(us, case):
    """us.split / us.split_NIRRed: [(k, row0, col0, lst window, nir window, red window)] of the full windows, and nwin"""
    lst_k = 0.02 * case["lst_raw"].astype(np.float32)
    nir, red = 0.0001 * case["nir"].astype(np.float32), 0.0001 * case["red"].astype(np.float32)
    out, cnt1 = [], 0
    fine = us.split_NIRRed(nir, red, (4 * WS, 4 * WS))
    for (x, y, ext_lst, ext_qc) in us.split(lst_k, case["qc"], (WS, WS)):
        x2, y2, ext_nir, ext_red = next(fine)
        cnt1 += 1
        assert (x2, y2) == (4 * x, 4 * y)
        if ext_lst.shape[0] == 64 and ext_lst.shape[1] == 64:
            assert ext_nir.shape == (256, 256)
            assert np.array_equal(ext_lst, lst_k[x:x + WS, y:y + WS])          # the first yielded offset is the ROW
            out.append((cnt1, x, y, ext_lst, ext_qc, ext_nir, ext_red))
    assert next(fine, None) is None
    return out, cnt1


def main():
    us, pm = import_process_modis()
    out = {"window": np.int64(WS), "coverages": np.array(R.COVERAGES), "cases": np.array(R.CASES, dtype=np.int64)}
    for ci, (seed, h, w) in enumerate(R.CASES):
        case = R.make_case(seed, h, w)
        wins, nwin = reference_windows(us, case)
        assert [(k, r, c) for k, r, c, *_ in wins] == case["full"] and nwin == len(R.windows(h, w))
        print(f"case {ci} ({h} x {w}): {nwin} windows, full {[(k, r, c) for k, r, c, *_ in wins]}")
        shas = {}
        for mode in (0, 1):
            counts = np.full((nwin, 2), -1, dtype=np.int32)
            for k, r, c, ext_lst, ext_qc, ext_nir, ext_red in wins:
                bad = ext_lst == 0.0
                if mode == 1:
                    bad = bad | np.array([[np.unpackbits(q)[-1] for q in row] for row in ext_qc], dtype=bool)
                counts[k - 1] = (bad.sum(), ((ext_nir + ext_red) == 0.0).sum())
            assert np.array_equal(counts, R.census(case["lst_raw"], case["qc"], case["nir"], case["red"], WS, mode))
            out[f"c{ci}_m{mode}_counts"] = counts
            for vi, cov in enumerate(R.COVERAGES):
                lst_ok = run_process(us, pm, case, mode, cov)                  # the reference's own LST stage
                index, lst_p, ndvi_p = [], [], []
                for k, r, c, ext_lst, ext_qc, ext_nir, ext_red in wins:
                    if k not in lst_ok:
                        continue
                    assert np.array_equal(lst_ok[k], ext_lst)
                    if 0.0 in ext_nir + ext_red:                               # process_modis.py:290: the pair is dropped
                        continue
                    ext_ndvi = us.compute_NDVI(ext_nir, ext_red)
                    ext_ndvi[ext_ndvi > 1] = 1
                    ext_ndvi[ext_ndvi < -1] = -1
                    index.append((k, r, c))
                    lst_p.append(ext_lst)
                    ndvi_p.append(ext_ndvi)
                    for name, a in (("lst", ext_lst), ("ndvi", ext_ndvi)):
                        assert a.dtype == np.float32
                        assert shas.setdefault((name, k), R.sha(a)) == R.sha(a)
                index = np.array(index, dtype=np.int32).reshape(-1, 3)
                _, r_index, r_lst, r_ndvi, _ = R.mine(case, WS, cov, mode)
                assert np.array_equal(index, r_index), (index, r_index)
                assert all(np.array_equal(a, b[0]) for a, b in zip(lst_p, r_lst))
                assert all(np.array_equal(a, b[0]) for a, b in zip(ndvi_p, r_ndvi))
                # data_preparation.py:32-39 and :83-102
                import random
                random.seed(42)
                labels = [random.choices(["Train", "Val"], [0.6, 0.4])[0] for _ in index]
                assert labels == R.assign_split(len(index)).tolist()
                liste = [p for p, s in zip(lst_p, labels) if s == "Train"]
                stats = np.full(6, np.nan)
                if liste:
                    a = np.zeros((64, 64 * len(liste)))
                    for i, mat in enumerate(liste):
                        a[:, i * 64:(i + 1) * 64] = mat
                    stats[:4] = max(np.max(i) for i in liste), min(np.min(i) for i in liste), np.mean(a), np.std(a)
                    liste = [p for p, s in zip(ndvi_p, labels) if s == "Train"]
                    a = np.zeros((256, 256 * len(liste)))
                    for i, mat in enumerate(liste):
                        a[:, i * 256:(i + 1) * 256] = mat
                    stats[4:] = np.mean(a), np.std(a)
                key = f"c{ci}_m{mode}_v{vi}"
                out[key + "_index"] = index
                out[key + "_labels"] = np.array(labels, dtype="U5")
                out[key + "_stats"] = stats                                    # maxi, mini, mean_lst, std_lst, mean_ndvi, std_ndvi
                print(f"  mode {mode} coverage {cov}: accepted k {index[:, 0].tolist()} labels {labels} stats {stats}")
        ks = sorted({k for _, k in shas})
        out[f"c{ci}_sha_k"] = np.array(ks, dtype=np.int64)
        out[f"c{ci}_sha_lst"] = np.array([shas[("lst", k)] for k in ks], dtype="U64")
        out[f"c{ci}_sha_ndvi"] = np.array([shas[("ndvi", k)] for k in ks], dtype="U64")
    path = os.path.join(HERE, "golden_products_v1.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
