#!/usr/bin/env python3
"""Golden vectors for the DMS sharpener: the reference's own DecisionTreeRegressorWithLinearLeafRegression
(data_mining_sharpener_modified.py:337-449) inside scikit-learn's BaggingRegressor(random_state=k), on the training sets that
tests/dms_reference.py builds.  Run in the BUILD container only (needs the reference checkout and scikit-learn, neither of which
travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dms.py

  1. imports the reference's module with `cv2`, `osgeo`, `numba` and `pyproj` stubbed in sys.modules (none is installed; the tree
     class needs none of them) and takes the tree class from it -- no text of the reference is copied;
  2. cases 0, 1: two real (LST 64x64, NDVI 256x256) pairs of the reference's test_data_formatted, read with an unpickler that
     constructs NumPy arrays only (every other global in the file becomes an inert placeholder: nothing from the file executes);
     cases 2, 3: seeded 16x16 ones with a NaN and a 0 K cell, a NaN NDVI pixel, a block of negative mean NDVI and
     duplicated NDVI values;
  3. fits BaggingRegressor(tree class, random_state=k) on (x, lst, w) of the restatement's training set, k the first seed for
     which the RESTATEMENT's fit is far from every tie (proxy gap >= 1e-10, frontier gap >= 1e-6, distinct leaf values);
  4. stores inputs, the bootstrap multiplicities from estimators_samples_ (scattered to row-major cell order), every tree's sorted
     thresholds and per-leaf (coef, intercept, min, max), and the ensemble's predictions of the fine NDVI (whole for the small
     cases, the [1::4, 2::4] sub-grid for the real ones) to tests/golden/golden_dms_v1.npz (data only).
"""
import importlib.util
import os
import pickle
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np

from tests import dms_reference as R

REF = os.environ.get("SIFSR_REFERENCE", "/root/reference")
E = 10
PROXY_GAP, HEAP_GAP = 1e-10, 1e-6
REAL_PAIRS = (0, 1)


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))


def reference_tree_class():
    for name in ("cv2", "osgeo", "osgeo.gdal", "numba", "pyproj"):
        sys.modules.setdefault(name, _Stub(name))
    sys.modules["osgeo"].gdal = sys.modules["osgeo.gdal"]
    spec = importlib.util.spec_from_file_location("reference_dms", os.path.join(REF, "data_mining_sharpener_modified.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.DecisionTreeRegressorWithLinearLeafRegression


class _Inert:
    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        pass

    def __call__(self, *a, **k):
        return _Inert()


class _ArraysOnly(pickle.Unpickler):
    def find_class(self, module, name):
        if module.split(".")[0] == "numpy" and name in ("_reconstruct", "ndarray", "dtype", "scalar"):
            return super().find_class(module, name)
        return _Inert


def real_pair(i):
    with open(os.path.join(REF, "test_data_formatted", "data", f"{i}_data_dict.pkl"), "rb") as f:
        d = _ArraysOnly(f).load()
    lst, ndvi = np.asarray(d["LST"]), np.asarray(d["NDVI"])
    assert lst.shape == (64, 64) and ndvi.shape == (256, 256), (lst.shape, ndvi.shape)
    return lst.astype(np.float32), ndvi.astype(np.float32)


def synthetic(seed, h, w):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:4 * h, 0:4 * w].astype(np.float64)
    p = rs.uniform(0, 1, 4)
    nf = 0.4 + 0.3 * np.sin(2 * np.pi * (yy / 37 + p[0])) * np.cos(2 * np.pi * (xx / 29 + p[1])) \
        + 0.12 * np.sin(2 * np.pi * (yy / 11 + xx / 13 + p[2])) + 0.03 * rs.standard_normal((4 * h, 4 * w))
    nf = np.clip(nf, -1, 1)
    nf[8:12, 20:24] = -0.3 + 0.05 * rs.standard_normal((4, 4))        # a block of negative mean NDVI: cv < 0, dropped
    nf[16:20, 4:8] = nf[16:20, 0:4]                                     # two cells with the same 16 values: duplicate features
    nf[24:28, 12:16] = nf[24:28, 8:12]
    nf = nf.astype(np.float32)
    mean, _ = R.aggregate(nf)
    lst = 312 - 14 * mean + 1.5 * np.sin(2 * np.pi * (np.mgrid[0:h, 0:w][0] / 7 + p[3])) + 0.4 * rs.standard_normal((h, w))
    lst = lst.astype(np.float32)
    lst[1, 2], lst[3, 0] = np.nan, 0.0
    nf[41, 7] = np.nan
    return lst, nf


def ok_fit(trees):
    for t in trees:
        if not (t["proxy_gap"] >= PROXY_GAP and t["heap_gap"] >= HEAP_GAP):
            return False
        if np.unique(t["values"]).size != t["values"].size:
            return False
    return True


def main():
    from sklearn.ensemble import BaggingRegressor
    Tree = reference_tree_class()
    cases = [real_pair(i) for i in REAL_PAIRS] + [synthetic(s, 16, 16) for s in (21, 22)]
    out = {"n_cases": len(cases), "E": E}
    for ci, (lst, nf) in enumerate(cases):
        h, w = lst.shape
        mean, std = R.aggregate(nf)
        ts = R.training_set(lst, mean, std)
        idx = np.flatnonzero(ts["good"].ravel())
        n = idx.size
        assert n == ts["n_train"] >= 10
        X = ts["x"].ravel()[idx][:, None]
        y = lst.astype(np.float64).ravel()[idx]
        sw = ts["w"].ravel()[idx]
        perm, xs, ys, ws = R.sorted_samples(ts, lst)
        for k in range(200):
            bag = BaggingRegressor(Tree(0.25, {"max_leaf_nodes": 30, "min_samples_leaf": 10}), random_state=k)
            bag.fit(X, y, sample_weight=sw)
            counts = np.zeros((E, h * w), dtype=np.int64)
            for e, s in enumerate(bag.estimators_samples_):
                counts[e, idx] = np.bincount(s, minlength=n)
            trees = R.fit(xs, ys, ws, R.cell_counts_to_sorted(counts, perm))
            if ok_fit(trees):
                break
        else:
            raise SystemExit(f"case {ci}: no seed in 0..199 keeps the fit away from a tie")
        assert len(bag.estimators_) == E and counts.max() < 256
        thr = np.full((E, 29), np.inf)
        leaves = np.zeros((E, 30, 4))
        nleaf = np.zeros(E, dtype=np.int32)
        x32 = X[:, 0].astype(np.float32).astype(np.float64)
        for e, est in enumerate(bag.estimators_):
            t = est.tree_
            th = np.sort(t.threshold[t.children_left != -1])
            L = th.size + 1
            assert L == len(est.leafParameters), "two leaves of a tree share a value"
            leaf_of = np.searchsorted(th, x32, side="left")
            plain = est.tree_.predict(X.astype(np.float32)).reshape(-1)
            for j in range(L):
                v = plain[np.flatnonzero(leaf_of == j)[0]]
                lp = est.leafParameters[v]
                rg = lp["linearRegression"]
                leaves[e, j] = float(rg.coef_[0]), float(rg.intercept_), float(lp["min"]), float(lp["max"])
            thr[e, :L - 1], nleaf[e] = th, L
        xq = np.where(np.isnan(nf), 0.0, nf.astype(np.float64)).reshape(-1, 1)
        pred = bag.predict(xq).reshape(nf.shape)
        pred[np.isnan(nf)] = np.nan
        pg, hg = min(t["proxy_gap"] for t in trees), min(t["heap_gap"] for t in trees)
        print(f"case {ci}: {h}x{w}, n_train {n}, random_state {k}, leaves {nleaf.tolist()}, worst proxy gap {pg:.2e}, "
              f"worst frontier gap {hg:.2e}", flush=True)
        out.update({f"c{ci}_lst": lst, f"c{ci}_ndvi_fine": nf, f"c{ci}_counts": counts.astype(np.uint8), f"c{ci}_seed": k,
                    f"c{ci}_thresholds": thr, f"c{ci}_leaves": leaves, f"c{ci}_nleaf": nleaf,
                    f"c{ci}_pred": pred if h * w <= 256 else pred[1::4, 2::4].copy()})
    path = os.path.join(HERE, "golden_dms_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
