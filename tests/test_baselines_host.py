"""CPU: the classical sharpening baselines -- what can be held without a GPU.

  * tests/baselines_reference.py (the float64 restatement the GPU tests compare with at shapes the golden does not hold) reproduces
    the reference's own images and Gamma_coarse (tests/golden/golden_baselines_v1.npz) to 1e-9 when given the reference's fit 2,
  * sifsr.baselines' host side -- its own damped least squares and the kriging system -- fed the golden Gamma_coarse gives weights
    whose image, through the restatement, is within the project's parity bar (1e-4 of the image's maximum) of the reference's,
  * the pins of include/sifsr_baselines.h for the `sifsrb_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, every entry point that can write through a pointer has a memory-contract case in tests/test_baselines_gpu.py,
  * the drop-in names exist with the reference's signatures."""
import ast
import inspect
import os
import re

import numpy as np
import pytest

from tests import baselines_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KRIGING = [(i, m) for i in (0, 1) for m in ("atprk", "aatprk")]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_baselines_v1.npz"))


def _case(golden, i):
    return tuple(golden[f"c{i}_{k}"].astype(np.float64) for k in ("lst", "ndvi_coarse", "ndvi_fine"))


def test_golden_holds_what_it_should(golden):
    assert float(golden["min_T"]) == 273.0 and float(golden["scc"]) == 926.0
    assert np.allclose(golden["distances"], 926.0 * np.sqrt(np.array(R.KS, dtype=np.float64)), rtol=1e-14)
    for i in (0, 1, 2):
        lst, nc, nf = _case(golden, i)
        assert lst.shape == nc.shape == (16, 16) and nf.shape == (64, 64) and golden[f"c{i}_lst"].dtype == np.float32
        assert ((lst == 0).sum() == 6) == (i in (0, 2))                      # the 2 x 3 block of lst == 0
    lst, nc, nf = _case(golden, 2)
    assert ((lst > 0) & (lst < 273)).sum() == 3 and np.isnan(nc).sum() == 1 and np.isnan(nf).sum() == 16
    for i, m in KRIGING:
        assert np.isfinite(golden[f"c{i}_{m}_fit2"]).all() and (golden[f"c{i}_{m}_fit2"] > 0).all()
        assert golden[f"c{i}_{m}_lambdas"].shape == (16, 25) and golden[f"c{i}_{m}_gamma"].shape == (15,)
        assert np.isfinite(golden[f"c{i}_{m}"]).all()
    assert float(golden["c0_atprk_restart_moved"]) < 1e-4 and float(golden["c1_atprk_restart_moved"]) < 1e-4


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restatement_tsharp(golden, i):
    ref = golden[f"c{i}_tsharp"]
    out = R.tsharp(*_case(golden, i), min_T=273.0)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan)
    assert np.abs(out - ref)[~nan].max() <= 1e-9


@pytest.mark.parametrize("i,method", KRIGING)
def test_restatement_kriging(golden, i, method):
    """with the reference's recorded fit 2: images to 1e-9 K, Gamma_coarse to 1e-9 relative; and the regularised model the
    reference's second fit minimised is the restatement's (its residual is stationary at the recorded parameters)"""
    ref, gref, fit2 = golden[f"c{i}_{method}"], golden[f"c{i}_{method}_gamma"], golden[f"c{i}_{method}_fit2"]
    out, g = getattr(R, method)(*_case(golden, i), variogram=fit2, scc=926.0, min_T=273.0)
    err = np.abs(out - ref).max()
    print(f"restatement {method} case {i}: max |out - ref| = {err:.3e} K")
    assert err <= 1e-9
    assert np.array_equal(g == 0, gref == 0) and (np.abs(g - gref)[1:] / gref[1:]).max() <= 1e-9
    # the same image from the reference's own recorded weights, and the weights themselves
    out_l, _ = getattr(R, method)(*_case(golden, i), variogram=fit2, scc=926.0, min_T=273.0, lambdas=golden[f"c{i}_{method}_lambdas"])
    assert np.abs(out_l - ref).max() <= 1e-9
    assert np.abs(R.kriging_weights(fit2[0], fit2[1], 926.0) - golden[f"c{i}_{method}_lambdas"]).max() <= 1e-9
    cost = lambda p: float(((R.regularised_model(p[0], p[1], 926.0) - gref) ** 2).sum())
    c0 = cost(fit2)
    for ds, dr in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
        assert cost((fit2[0] * (1 + ds), fit2[1] * (1 + dr))) >= c0 * (1 - 1e-6)


@pytest.mark.parametrize("i,method", KRIGING)
def test_host_fit_gives_the_reference_image(golden, i, method):
    """sifsr.baselines.fit_variogram + kriging_weights on the golden Gamma_coarse -> image through the restatement, against the
    reference's: the project's parity bar, 1e-4 of the image's maximum.  The reference itself moves by 2.5e-8 / 1.8e-6 K (cases 0 /
    1) when its fit starts from (9, 1300); a value far above that would mean a bug, not fit noise."""
    from sifsr import baselines as BL
    ref, gref = golden[f"c{i}_{method}"], golden[f"c{i}_{method}_gamma"]
    fit1, fit2 = BL.fit_variogram(gref, 926.0, 7.0, 1000.0)
    assert np.isfinite(fit2).all() and (fit2 > 0).all()
    lam = BL.kriging_weights(fit2[0], fit2[1], 926.0)
    out, _ = getattr(R, method)(*_case(golden, i), variogram=fit2, scc=926.0, min_T=273.0, lambdas=lam)
    err = np.abs(out - ref).max()
    print(f"host fit {method} case {i}: fit1 {fit1} fit2 {fit2} (reference {golden[f'c{i}_{method}_fit1']} {golden[f'c{i}_{method}_fit2']}); "
          f"max |image - ref| = {err:.3e} K = {err / np.abs(ref).max():.3e} of the maximum")
    assert err <= 1e-4 * np.abs(ref).max()
    # the two host models are the restatement's
    assert np.abs(BL.regularised_model(fit2[0], fit2[1], 926.0) - R.regularised_model(fit2[0], fit2[1], 926.0)).max() <= 1e-9 * fit2[0]
    assert np.abs(lam - R.kriging_weights(fit2[0], fit2[1], 926.0)).max() <= 1e-9


def test_host_fit_is_capped_and_refuses_a_bad_variogram():
    from sifsr import baselines as BL
    d = 926.0 * np.sqrt(np.array(BL.KS, dtype=np.float64))
    y = 12.0 * (1 - np.exp(-3 * d / 2500.0))
    p, it = BL._damped_least_squares(lambda q: q[0] * (1 - np.exp(-3 * d / q[1])), y, (7.0, 1000.0))
    assert it <= BL.LM_MAX_ITER == 200 and abs(p[0] - 12.0) < 1e-6 and abs(p[1] - 2500.0) < 1e-3        # an exact model is recovered
    _, it = BL._damped_least_squares(lambda q: q[0] * (1 - np.exp(-3 * d / q[1])), d * 1e-3, (7.0, 1000.0), max_iter=5)
    assert it <= 5                                                                                       # a straight line: no finite range


# ---- the pins of include/sifsr_baselines.h (the gate itself is tests/test_capi_gate.py) --------------------------------------
def test_every_writing_baseline_entry_point_has_a_contract_case(L):
    from tests import test_baselines_gpu as T
    assert len(L.declared("baselines")) == 6
    writers = L.writers("baselines")
    assert writers == {"sifsrb_linfit": ["fit"], "sifsrb_linfit_window": ["coef"], "sifsrb_residual": ["delta"],
                       "sifsrb_semivariogram": ["scratch", "gamma"], "sifsrb_sharpen": ["out"]}
    assert all(len(cases) >= 3 for cases in T.CONTRACT.values())


def test_dropin_names_and_signatures():
    tree = ast.parse(open(os.path.join(ROOT, "dropin", "utils.py")).read())
    fns = {n.name: [a.arg for a in n.args.args] for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
    assert fns["TsHARP"] == ["temp_coarse", "index_coarse", "index_fine", "scale", "min_T", "path_image"]
    assert fns["ATPRK"] == ["temp_coarse", "index_coarse", "index_fine", "scale", "scc", "block_size", "sill", "ran", "min_T", "path_image"]
    assert fns["AATPRK"] == ["temp_coarse", "index_coarse", "index_fine", "scale", "scc", "b_radius", "block_size", "sill", "ran",
                             "min_T", "path_image"]
    assert "__getattr__" in fns                                               # everything else still refuses by name


def test_public_interface():
    import sifsr
    from sifsr import baselines as BL
    assert sifsr.baselines is BL
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(BL.tsharp) == ["lst", "ndvi_coarse", "ndvi_fine", "min_T"]
    assert sig(BL.atprk) == ["lst", "ndvi_coarse", "ndvi_fine", "scc", "sill", "ran", "min_T", "variogram", "return_variogram"]
    assert sig(BL.aatprk) == ["lst", "ndvi_coarse", "ndvi_fine", "scc", "b_radius", "sill", "ran", "min_T", "variogram", "return_variogram"]
    d = {k: v.default for k, v in inspect.signature(BL.aatprk).parameters.items()}
    assert (d["scc"], d["b_radius"], d["sill"], d["ran"], d["min_T"], d["variogram"], d["return_variogram"]) == (926.0, 2, 7.0, 1000.0, 285.0, None, False)
    import torch
    z = torch.zeros((1, 1, 8, 8))
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        BL.tsharp(z, z, torch.zeros((1, 1, 32, 32)))
    with pytest.raises(sifsr.SifsrError):
        BL.semivariogram(z.double())
    src = open(BL.__file__).read()
    assert "scipy" not in re.sub(r'""".*?"""', "", src, flags=re.S)           # the fits are the package's own
