"""CPU: the DMS sharpener -- what can be held without a GPU.

  * tests/dms_reference.py (the float64 restatement the GPU tests compare with) reproduces what the reference's own tree class
    gave inside scikit-learn's BaggingRegressor (tests/golden/golden_dms_v1.npz, made by tests/golden/make_golden_dms.py):
    thresholds bit-equal, leaf parameters and predictions to 1e-9 relative,
  * every fit of every fixture is far from a tie IN THE RESTATEMENT: relative proxy gap >= 1e-10, frontier priority gap >= 1e-6,
    distinct leaf values (a condition on the inputs, not a tolerance: a near-tie may flip under another summation order),
  * where scikit-learn is installed, the restatement's trees are those of a live DecisionTreeRegressor on seeded data with
    duplicate features and zero weights,
  * the pins of include/sifsr_dms.h for the `sifsrd_` entry points (the gate itself is tests/test_capi_gate.py),
  * the public interface, its refusals, and the drop-in name."""
import ast
import inspect
import os

import numpy as np
import pytest

from tests import dms_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [0, 1, 2, 3]
PROXY_GAP, HEAP_GAP = 1e-10, 1e-6


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dms_v1.npz"))


_FITS = {}


def fitted(golden, i):
    """the restatement on case i (uncorrected image, info), computed once"""
    if i not in _FITS:
        _FITS[i] = R.dms(golden[f"c{i}_lst"], golden[f"c{i}_ndvi_fine"], golden[f"c{i}_counts"].astype(np.int64), do_correct=False)
    return _FITS[i]


def golden_leaves(golden, i, e):
    """(L, 4) coef, intercept, lo, hi from the stored coef, intercept, min, max"""
    n = int(golden[f"c{i}_nleaf"][e])
    g = golden[f"c{i}_leaves"][e, :n].copy()
    r = g[:, 3] - g[:, 2]
    g[:, 2], g[:, 3] = g[:, 2] - 0.25 * r, g[:, 3] + 0.25 * r
    return g


def test_golden_holds_what_it_should(golden):
    assert int(golden["n_cases"]) == 4 and int(golden["E"]) == 10
    for i in CASES:
        lst, nf, c = golden[f"c{i}_lst"], golden[f"c{i}_ndvi_fine"], golden[f"c{i}_counts"]
        h, w = lst.shape
        assert (h, w) == ((64, 64) if i < 2 else (16, 16)) and nf.shape == (4 * h, 4 * w)
        assert lst.dtype == np.float32 and nf.dtype == np.float32 and c.shape == (10, h * w)
        _, info = fitted(golden, i)
        assert (c.sum(1) == info["ts"]["n_train"]).all()                    # a bootstrap draws n_train samples
        assert (c[:, ~info["ts"]["good"].ravel()] == 0).all()
    for i in (2, 3):
        lst, nf = golden[f"c{i}_lst"], golden[f"c{i}_ndvi_fine"]
        ts = fitted(golden, i)[1]["ts"]
        assert np.isnan(lst).sum() == 1 and (lst == 0).sum() == 1 and np.isnan(nf).sum() == 1
        assert ts["n_train"] == 253 and not ts["good"][2, 5] and ts["cv"][2, 5] < 0          # the negative-mean block
        x32 = ts["x"].astype(np.float32)
        assert x32[4, 0] == x32[4, 1] and x32[6, 2] == x32[6, 3]                             # duplicate features
        assert (ts["w"][ts["good"]] == 0).sum() == 1                                         # the least homogeneous cell


@pytest.mark.parametrize("i", CASES)
def test_restatement_vs_golden(golden, i):
    out, info = fitted(golden, i)
    assert len(info["trees"]) == 10
    worst = 0.0
    for e, t in enumerate(info["trees"]):
        n = int(golden[f"c{i}_nleaf"][e])
        assert t["leaves"].shape == (n, 4)
        assert np.array_equal(t["thresholds"], golden[f"c{i}_thresholds"][e, :n - 1])        # bit-equal
        assert np.isinf(golden[f"c{i}_thresholds"][e, n - 1:]).all()
        ref = golden_leaves(golden, i, e)
        worst = max(worst, float((np.abs(t["leaves"] - ref) / np.abs(ref)).max()))
    nf = golden[f"c{i}_ndvi_fine"]
    xq = np.where(np.isnan(nf), 0.0, nf.astype(np.float64))
    pred = sum(R.predict_tree(t, xq) for t in info["trees"]) / 10
    pred[np.isnan(nf)] = np.nan
    ref = golden[f"c{i}_pred"]
    sub = pred if ref.shape == pred.shape else pred[1::4, 2::4]
    assert np.array_equal(np.isnan(sub), np.isnan(ref))
    perr = float(np.nanmax(np.abs(sub - ref) / np.abs(ref)))
    print(f"case {i}: leaf parameters {worst:.2e}, predictions {perr:.2e} relative")
    assert worst <= 1e-9 and perr <= 1e-9
    assert np.array_equal(out, np.where(np.isnan(nf), np.nan, pred).astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("i", CASES)
def test_fixtures_are_far_from_a_tie(golden, i):
    trees = fitted(golden, i)[1]["trees"]
    pg, hg = min(t["proxy_gap"] for t in trees), min(t["heap_gap"] for t in trees)
    print(f"case {i}: worst proxy gap {pg:.2e}, worst frontier gap {hg:.2e}")
    assert pg >= PROXY_GAP and hg >= HEAP_GAP
    for t in trees:
        assert np.unique(t["values"]).size == t["values"].size


def _seeded(seed, n):
    rs = np.random.RandomState(seed)
    x = np.sort(rs.uniform(-0.2, 0.9, n).astype(np.float32))
    x[n // 3:n // 3 + 7] = x[n // 3]                                    # duplicates
    x = np.sort(x)
    y = 310 - 15 * x.astype(np.float64) + 2 * np.sin(9 * x) + rs.standard_normal(n)
    w = rs.uniform(0, 1, n) * rs.poisson(1.0, n)                        # ~37 % zero weights
    return x, y, w


# seeds screened so that the restatement's fit is far from a tie (asserted below)
LIVE = [(s, 400) for s in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11)] + [(s, 4096) for s in (2, 3, 5, 7, 8, 11, 13, 14, 15, 17)]


@pytest.mark.parametrize("seed,n", LIVE)
def test_restatement_vs_live_sklearn(seed, n):
    tree = pytest.importorskip("sklearn.tree")
    x, y, w = _seeded(seed, n)
    t = R.fit_tree(x.astype(np.float64), y, w)
    assert t["proxy_gap"] >= PROXY_GAP and t["heap_gap"] >= HEAP_GAP
    sk = tree.DecisionTreeRegressor(max_leaf_nodes=30, min_samples_leaf=10, random_state=0).fit(x[:, None], y, sample_weight=w)
    tr = sk.tree_
    inner = tr.children_left != -1
    assert np.array_equal(np.sort(tr.threshold[inner]), t["thresholds"])                     # the same partition, bit-equal
    assert tr.n_node_samples[0] == (w != 0).sum()
    first = x[t["bounds"][:-1]]
    val = sk.predict(first[:, None])
    assert (np.abs(val - t["values"]) / np.abs(val)).max() <= 1e-12


def test_percentile_is_numpys():
    rs = np.random.RandomState(5)
    for n in (10, 11, 16, 253, 4096):
        v = np.sort(rs.uniform(0.01, 3, n))
        assert R.percentile80(v) == np.percentile(v, 80)


def test_few_good_cells_give_no_model():
    rs = np.random.RandomState(2)
    nf = rs.uniform(0.1, 0.8, (16, 16)).astype(np.float32)
    lst = np.full((4, 4), np.nan, dtype=np.float32)
    lst.ravel()[:9] = 300.0
    out, info = R.dms(lst, nf, np.ones((10, 16), dtype=np.int64))
    assert info["ts"]["n_train"] == 0 and np.isnan(out).all() and out.shape == (16, 16)


# ---- the pins of include/sifsr_dms.h (the gate itself is tests/test_capi_gate.py) --------------------------------------------
def test_every_writing_dms_entry_point_has_a_contract_case(L):
    from tests import test_dms_gpu as T
    writers = L.writers("dms")
    assert len(L.declared("dms")) == 7
    assert writers == {"sifsrd_aggregate": ["mean", "std"], "sifsrd_trainset": ["x", "cv", "good"], "sifsrd_weights": ["weight"],
                       "sifsrd_fit": ["scratch", "thresholds", "nleaf", "leaves"], "sifsrd_predict": ["sr"],
                       "sifsrd_correct": ["out"]}
    assert all(len(cases) >= 3 for cases in T.CONTRACT.values())


def test_dropin_name_and_signature():
    tree = ast.parse(open(os.path.join(ROOT, "dropin", "utils.py")).read())
    fns = {n.name: [a.arg for a in n.args.args] for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
    assert fns["DMS"][:3] == ["temp_coarse", "index_fine", "scale"]
    assert "__getattr__" in fns


def test_public_interface_and_refusals():
    import sifsr
    import torch
    from sifsr import baselines as BL
    p = inspect.signature(BL.dms).parameters
    assert list(p)[:7] == ["lst", "ndvi_fine", "n_estimators", "counts", "seed", "correct", "return_model"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    assert (p["n_estimators"].default, p["counts"].default, p["seed"].default, p["correct"].default, p["return_model"].default) \
        == (10, None, 0, True, False)
    assert callable(BL.dms_model) and callable(BL.dms_apply)
    z, f = torch.zeros((1, 1, 8, 8)), torch.zeros((1, 1, 32, 32))
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        BL.dms(z, f)
    for kw in ({"moving_window_size": 30}, {"predictors": 2}, {"quality": "q.tif"}):
        with pytest.raises(NotImplementedError):
            BL.dms(z, f, **kw)
