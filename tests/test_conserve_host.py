"""CPU: conservation of the observed LST -- what can be held without a GPU.

  * the restatement tests/conserve_reference.py: it reproduces tests/golden/golden_conserve_v1.npz (written where the reference is:
    there its D was held to the reference's downscale_LST_SR_to_LR and its U to the input pipeline's bicubic), the reference's D
    recorded in that file, and its own properties -- the counted set is "3 x 3 clipped neighbourhood all valid" by brute force, D
    reads exactly that neighbourhood, a constant sr equal to a constant lst gives r = 0 to rounding, what invalid pixels hold
    changes nothing,
  * convergence, recorded: on the golden cases the RMSE falls with every one of three steps (relax 1: to below a sixth after the
    first; relax 0.5: by at least a third per step), and the bias to below 0.02 K after the first step at relax 1.  The GPU test
    asserts the fall and nothing more,
  * the pins of include/sifsr_conserve.h for the `sifsrk_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, the writing entry point has memory-contract cases in tests/test_conserve_gpu.py, the workspace size and the error codes
    through the host-only paths,
  * the public names exist with the defaults that leave every existing call as it was."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import conserve_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_conserve_v1.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def golden_case(gold, i):
    mask = gold[f"c{i}_mask"]
    return gold[f"c{i}_sr"], gold[f"c{i}_lst"], (None if mask.size == 0 else mask), float(gold[f"c{i}_relax"])


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_file(gold):
    assert list(gold["names"]) == ["9x8", "mask_block", "sr_only", "5x7_half"]
    x = gold["d_input"].astype(np.float64)
    d = np.abs(R.D(x, R.taps32()) - gold["d_reference"]).max()
    print(f"D: max |restatement - reference| = {d:.3e} K")
    assert d == float(gold["d_maxdiff"]) and d < 3 * 2.0 ** -25 * 1.375 * np.abs(x).max()     # the generator's bar, reasoned there
    for i in range(4):
        sr, lst, mask, relax = golden_case(gold, i)
        out, rows, _, c, _ = R.conserve_ref(sr, lst, mask, n_iter=3, relax=relax)
        r0 = R.residual(sr, lst, mask, R.taps32())[0]
        m = R.up(c)
        assert np.array_equal(r0, gold[f"c{i}_r0"]) and np.array_equal(out[m], gold[f"c{i}_out3"][m])
        assert np.array_equal(out[~m].astype(np.float32).view(np.uint32), sr[~m].view(np.uint32))
        assert np.array_equal(rows, gold[f"c{i}_stats"])


def test_the_generated_cases_are_the_golden_ones(gold):
    for i, (sr, lst, mask) in enumerate((R.make_case(9, 8, 21) + (None,), R.hole_case("mask_block"), R.hole_case("sr_only"),
                                         R.make_case(5, 7, 22) + (None,))):
        gsr, glst, gmask, _ = golden_case(gold, i)
        assert np.array_equal(sr.view(np.uint32), gsr.view(np.uint32)) and np.array_equal(lst.view(np.uint32), glst.view(np.uint32))
        assert (mask is None and gmask is None) or np.array_equal(mask, gmask)


def test_up4_phases_are_the_kernel_constants():
    """the four fixed x4 phases: t = 0.625, 0.875, 0.125, 0.375 from the source index floor(X / 4) - 2 + (X % 4 >= 2), dyadic
    coefficients (exact in fp32) that sum to 1 -- the table csrc/conserve.hip holds"""
    idx, coef = R.up4_axis(9)
    X = np.arange(12, 24)
    assert np.array_equal(idx[X, 0], X // 4 - 2 + (X % 4 >= 2))
    assert np.array_equal(coef[12:16], coef[16:20]) and np.array_equal(coef.astype(np.float32).astype(np.float64), coef)
    assert np.array_equal(coef.sum(axis=1), np.ones(36))
    text = open(os.path.join(ROOT, "land-surface-temperature-super-resolution-with-a-scale-invariance-free-neural-approach_amd", "csrc",
                             "conserve.hip")).read()
    table = re.search(r"UP4\[4\]\[4\] = \{(.*?)\};", text, flags=re.S).group(1)
    got = np.array([float(v) for v in re.findall(r"-?\d+\.\d+", table)]).reshape(4, 4)
    assert np.array_equal(got, coef[12:16])
    assert idx.min() == 0 and idx.max() == 8 and np.array_equal(idx[0], [0, 0, 0, 1]) and np.array_equal(idx[35], [7, 8, 8, 8])


@pytest.mark.parametrize("kind", R.HOLES)
def test_counted_set_by_brute_force(kind):
    sr, lst, mask = R.hole_case(kind)
    c = R.cell_valid(sr, lst, mask)
    n = R.counted(c)
    h, w = c.shape
    for i in range(h):
        for j in range(w):
            assert n[i, j] == c[max(0, i - 1):i + 2, max(0, j - 1):j + 2].all()
    expected = {"interior": (255, 247), "corner": (254, 248), "edge": (254, 244), "row": (240, 208), "mask_block": (235, 205),
                "sr_only": (253, 234), "nothing_valid": (0, 0), "checkerboard": (128, 0)}
    assert (int(c.sum()), int(n.sum())) == expected[kind]


def test_d_reads_exactly_the_3x3_neighbourhood():
    """moving one HR pixel moves D at the cells within one cell of it and at no other, also across the reflecting edge"""
    t = R.taps32()
    sr, _ = R.make_case(6, 7, 4)
    base = R.D(sr, t)
    for (y, x) in ((0, 0), (3, 27), (23, 0), (11, 13), (23, 27), (8, 4)):
        p = sr.astype(np.float64)
        p[y, x] += 1.0
        moved = R.D(p, t) != base
        want = np.zeros_like(moved)
        want[max(0, y // 4 - 1):y // 4 + 2, max(0, x // 4 - 1):x // 4 + 2] = True
        assert np.array_equal(moved, want), (y, x)


def test_constant_rasters_leave_no_residual():
    t = R.taps32()
    for hw in ((3, 3), (9, 8)):
        sr, lst = np.full((4 * hw[0], 4 * hw[1]), 301.25, np.float32), np.full(hw, 301.25, np.float32)
        r, n, c = R.residual(sr, lst, None, t)
        assert n.all() and c.all()
        # the fp32 taps do not sum to 1 exactly: D(const) = const * sum(t)^2
        assert np.abs(r + 301.25 * (t.sum() ** 2 - 1)).max() < 1e-12 and np.abs(r).max() < 301.25 * 9 * 2.0 ** -24
        out, rows, _, _, _ = R.conserve_ref(sr, lst, None, n_iter=2)
        assert np.abs(out - 301.25).max() < 1e-4 and rows[0, 0] == hw[0] * hw[1]


@pytest.mark.parametrize("kind", R.HOLES)
def test_invalid_pixels_are_inert_in_the_restatement(kind):
    sr, lst, mask = R.hole_case(kind)
    want = R.conserve_ref(sr, lst, mask, n_iter=2)
    m = R.up(want[3])
    for junk in (np.nan, 0.0, np.inf, 1e30):
        if junk == 1e30 and mask is None and kind != "sr_only":
            continue
        psr, plst = R.poisoned(sr, lst, mask, junk)
        assert not (np.array_equal(psr, sr, equal_nan=True) and np.array_equal(plst, lst, equal_nan=True)) or kind == "nothing_valid"
        got = R.conserve_ref(psr, plst, mask, n_iter=2)
        assert np.array_equal(got[0][m], want[0][m]) and np.array_equal(got[1], want[1], equal_nan=True)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])


def test_convergence_recorded(gold):
    for i, name in enumerate(gold["names"]):
        rows = gold[f"c{i}_stats"]
        rmse, bias = rows[:, 2], rows[:, 1]
        print(name, "RMSE", rmse.tolist(), "bias", bias.tolist())
        assert np.all(np.diff(rmse) < 0) and np.all(rows[:, 0] == rows[0, 0])
        if float(gold[f"c{i}_relax"]) == 1.0:
            assert rmse[1] < rmse[0] / 5 and abs(bias[1]) < 0.02 < abs(bias[0])
        else:
            assert np.all(rmse[1:] < rmse[:-1] * (2 / 3))
        assert np.all(rows[:, 3] >= rmse)


# ---- 2. the pins of include/sifsr_conserve.h (the gate itself is tests/test_capi_gate.py) ---------------------------------------
def test_the_writing_entry_point_has_contract_cases(L):
    from tests import test_conserve_gpu as T
    names, writers = L.declared("conserve"), L.writers("conserve")
    assert names == ["sifsrk_conserve", "sifsrk_workspace_bytes"]
    assert writers == {"sifsrk_conserve": ["out", "stats", "workspace"]}
    assert sorted(T.CONTRACT) == sorted(writers)
    assert all(len(cases) >= 3 for cases in T.CONTRACT.values())
    # with and without a mask, in place and not, the pure check
    assert {(s[3], s[4]) for s in T.CONTRACT_SHAPES} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(s[2] == 0 for s in T.CONTRACT_SHAPES) and any(s[2] >= 2 for s in T.CONTRACT_SHAPES)


def test_host_only_entry_points(L):
    """the workspace size; shape, argument and workspace errors are found before anything is launched (none needs a GPU)"""
    size = lambda *a: L.call("sifsrk_workspace_bytes", *a)
    for h, w, n in ((3, 3, 0), (9, 8, 1), (33, 41, 3), (1200, 1200, 1), (16384, 16384, 64)):
        need = size(h, w, n)
        tiles = -(-h // 8) * -(-w // 8)
        # r (fp32) and one validity byte per cell, four float64 partials per workgroup and statistics row
        assert 5 * h * w + 32 * tiles * (n + 1) <= need <= 5 * h * w + 32 * tiles * (n + 1) + 8
        assert size(h, w, n + 1 if n < 64 else n) >= need
    for h, w, n in ((2, 9, 1), (9, 2, 1), (0, 0, 0), (-1, 9, 0), (16385, 9, 0), (9, 16385, 0), (9, 9, -1), (9, 9, 65)):
        assert size(h, w, n) == 0
    one = ctypes.c_void_p(4096)
    taps = (ctypes.c_float * 9)(*[float(v) for v in R.taps32()])
    fn = L.lib().sifsrk_conserve
    args = lambda **kw: [kw.get("sr", one), kw.get("lst", one), kw.get("mask", one), kw.get("out", one), kw.get("stats", one),
                         kw.get("ws", one), kw.get("nbytes", 1 << 40), kw.get("h", 9), kw.get("w", 8), kw.get("taps", taps),
                         kw.get("relax", 1.0), kw.get("n_iter", 1), None]
    for bad in (dict(h=2), dict(w=2), dict(h=0), dict(h=16385), dict(w=16385), dict(n_iter=-1), dict(n_iter=65)):
        assert fn(*args(**bad)) == 1001, bad
    for bad in (dict(sr=None), dict(lst=None), dict(out=None), dict(stats=None), dict(ws=None), dict(taps=None),
                dict(ws=ctypes.c_void_p(4100)), dict(sr=ctypes.c_void_p(4104)), dict(out=ctypes.c_void_p(4104)),
                dict(relax=float("nan")), dict(relax=float("-inf"))):
        assert fn(*args(**bad)) == 1002, bad
    need = size(9, 8, 1)
    assert fn(*args(nbytes=need - 1)) == 1003 and fn(*args(nbytes=0)) == 1003 and fn(*args(nbytes=need - 1, mask=None)) == 1003
    assert fn(*args(nbytes=size(9, 8, 0), n_iter=1)) == 1003


# ---- 3. the public names ---------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import conserve, gaps, predict
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    assert sig(conserve.consistency) == [("sr", E_), ("lst", E_), ("mask", None), ("mtf", 0.1), ("return_residual", False)]
    assert sig(conserve.conserve) == [("sr", E_), ("lst", E_), ("mask", None), ("n_iter", 1), ("relax", 1.0), ("mtf", 0.1), ("out", None),
                                      ("return_stats", False)]
    # the existing calls are what they were, with the new option last and off
    # the two granule calls: the option is keyword-only, off by default and added around the call (conserve.granule_option); the
    # parameter list tests/test_gaps_host.py pins is what it was
    for f, last in ((predict.predict_granule, "cover_edges"), (gaps.predict_granule_gaps, "return_info")):
        assert list(inspect.signature(f).parameters)[-1] == last
        outer = inspect.signature(f, follow_wrapped=False).parameters
        assert outer["conserve"].kind is inspect.Parameter.KEYWORD_ONLY and outer["conserve"].default == 0
        assert "conserve=k" in f.__doc__
    assert predict.predict_granule_gaps is gaps.predict_granule_gaps
    with pytest.raises(sifsr.SifsrError):                                      # refused before anything runs
        predict.predict_granule(None, None, None, None, conserve=-1)
    assert sig(predict.GranulePredictor.__init__)[-2:] == [("device", None), ("conserve", 0)]
    z = torch.zeros((12, 12))
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        conserve.consistency(z, torch.zeros((3, 3)))
    with pytest.raises(sifsr.SifsrError):
        conserve.conserve(z, torch.zeros((3, 3)))
    assert os.path.samefile(sifsr._lib.header_path("conserve"), os.path.join(ROOT, "include", "sifsr_conserve.h"))
    assert sifsr.conserve is conserve and conserve.MAX_ITER == 64
