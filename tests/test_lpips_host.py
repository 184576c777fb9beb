"""CPU: on-device LPIPS -- what can be held without a GPU.

  * the float64 restatement tests/lpips_reference.py against the golden file (whose maker ran the reference's own ContentLoss on
    the
    same weights), the checksum of the closed-form weights, an identical pair -> 0,
  * the planted cases: every non-identical case of the GPU value tests and of the golden file has all five layer terms >= 1e-7 in
    float64, so no layer can pass as 0 = 0,
  * the pins of include/sifsr_lpips.h for the `sifsrl_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, every entry point that can write through a pointer has at least three memory-contract cases in tests/test_lpips_gpu.py;
    sizes and error codes through the host-only paths,
  * the public interface and its errors, the drop-in without weights included."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from tests import lpips_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = R.ROOT


# ---- 1. the restatement and the generator ----------------------------------------------------------------------------------------
def test_generated_weights_checksum():
    assert R.vgg_flat().size == 14714688 and R.lin_flat().size == 1472
    assert R.weights_sha256() == R.WEIGHTS_SHA256
    vgg, lin = R.weights()
    for (ci, co), (w, b) in zip(R.CONV_CHANNELS, vgg):
        a = np.sqrt(6.0 / (9 * ci))
        assert w.shape == (co, ci, 3, 3) and np.abs(w).max() <= a and np.abs(w).max() > 0.99 * a and np.abs(b).max() <= 0.1
    assert all(v.min() > 0 and v.max() < 10.0 / c for v, c in zip(lin, R.TAP_CHANNELS))


def test_restatement_against_the_golden_file():
    gold = np.load(R.GOLDEN)
    assert str(gold["weights_sha256"]) == R.WEIGHTS_SHA256 and len(gold["kinds"]) == 5
    for i, kind in enumerate(gold["kinds"]):
        a, b = gold[f"a{i}"][None], gold[f"b{i}"][None]
        x, y, mini, maxi = R.normalise_pair(a, b)
        assert np.array_equal(np.array([mini[0], maxi[0]], np.float32), gold[f"minmax{i}"])
        for tag, got in (("pairs", R.pair_terms(a, b)), ("imagenet", R.terms(x, y))):
            want = gold[f"terms_{tag}{i}"]
            if kind == "same":
                assert (got == 0).all() and (want == 0).all()
            else:
                assert np.allclose(got[0], want, rtol=1e-12, atol=0), (i, tag, got, want)       # float64 on another host: summation order
                assert want[:5].min() >= R.FLOOR and abs(want[:5].sum() - want[5]) <= 1e-15


def test_identical_pair_is_zero_and_swap_is_symmetric():
    x, y = R.images(1, 16, 16, seed=1)
    assert (R.terms(x, x) == 0).all()
    assert np.array_equal(R.terms(x, y), R.terms(y, x))


def test_planted_cases_are_above_the_floor():
    smallest = 1.0
    for shape in R.VALUE_SHAPES:
        for _, _, want in R.value_case(shape):
            print(shape, want.tolist())
            assert want.shape == (shape[0], 6) and (want[:, :5] >= R.FLOOR).all()
            smallest = min(smallest, want[:, :5].min())
    x, y = R.images(3, 24, 40, seed=7)
    a, b = R.rasters(3, 24, 40, seed=7)
    assert (R.terms(x, y)[:, :5] >= R.FLOOR).all() and (R.pair_terms(a, b)[:, :5] >= R.FLOOR).all()
    assert R.FLOOR == 1e-7 and smallest >= R.FLOOR


# ---- 2. the pins of include/sifsr_lpips.h (the gate itself is tests/test_capi_gate.py) ------------------------------------------
def test_every_writing_lpips_entry_point_has_contract_cases(L):
    from tests import test_lpips_gpu as T
    names, writers = L.declared("lpips"), L.writers("lpips")
    assert names == ["sifsrl_lpips", "sifsrl_lpips_pairs", "sifsrl_pack", "sifsrl_pack_floats", "sifsrl_workspace_bytes"]
    assert writers == {"sifsrl_pack": ["packed"], "sifsrl_lpips": ["workspace", "out6"], "sifsrl_lpips_pairs": ["workspace", "out6"]}
    assert all(n not in writers for n in ("sifsrl_pack_floats", "sifsrl_workspace_bytes"))
    assert sorted(T.CONTRACT) == sorted(writers)
    assert all(len(cases) >= 3 for cases in T.CONTRACT.values())


def test_host_only_entry_points(L):
    """sizes; shape, argument and workspace errors are found before anything is launched (none needs a GPU)"""
    size = lambda *a: L.call("sifsrl_workspace_bytes", *a)
    weights = 9 * (16 * 64 + sum(ci * co for ci, co in R.CONV_CHANNELS[1:]))
    assert L.call("sifsrl_pack_floats") == weights + 4224 + 1472
    base = size(1, 16, 16)
    assert base >= 3 * 2 * 16 * 16 * 64 * 4
    assert size(2, 16, 16) > base and size(1, 17, 16) > base and size(1, 16, 17) > base
    for n, h, w in ((1, 41, 43), (3, 48, 80), (83, 64, 64), (16, 256, 256)):
        need = size(n, h, w)
        assert 3 * 2 * n * h * w * 256 <= need <= 3 * 2 * n * h * w * 256 + 5 * n * 128 * 8 + 12 * n + 8 * 256
    for n, h, w in ((0, 16, 16), (-1, 64, 64), (1, 15, 16), (1, 16, 15), (128, 256, 256), (1, 4096, 4096), (1, 65536, 65536), (1 << 30, 16, 16)):
        assert size(n, h, w) == 0, (n, h, w)
    assert size(127, 256, 256) > 0                                    # 2 * 127 * 256 * 256 * 64 * 4 bytes is just below 4 GiB - 4 KiB

    one = ctypes.c_void_p(4096)
    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    f3, f1 = L.lib().sifsrl_lpips, L.lib().sifsrl_lpips_pairs
    a3 = lambda **kw: [kw.get("x", one), kw.get("y", one), kw.get("N", 2), kw.get("H", 41), kw.get("W", 43), kw.get("mean", three),
                       kw.get("std", three), kw.get("packed", one), kw.get("ws", one), kw.get("nbytes", 1 << 40), kw.get("out", one), None]
    a1 = lambda **kw: [kw.get("a", one), kw.get("b", one), kw.get("N", 2), kw.get("H", 41), kw.get("W", 43), kw.get("packed", one),
                       kw.get("ws", one), kw.get("nbytes", 1 << 40), kw.get("out", one), None]
    for bad in (dict(N=0), dict(H=15), dict(W=15), dict(N=128, H=256, W=256), dict(H=65536, W=65536)):
        assert f3(*a3(**bad)) == 1001 and f1(*a1(**bad)) == 1001
    for bad in (dict(x=None), dict(y=None), dict(mean=None), dict(std=None), dict(packed=None), dict(ws=None), dict(out=None),
                dict(ws=ctypes.c_void_p(4100))):
        assert f3(*a3(**bad)) == 1002
    for bad in (dict(a=None), dict(b=None), dict(packed=None), dict(ws=None), dict(out=None)):
        assert f1(*a1(**bad)) == 1002
    need = size(2, 41, 43)
    assert f3(*a3(nbytes=need - 1)) == 1003 and f1(*a1(nbytes=need - 1)) == 1003 and f1(*a1(nbytes=0)) == 1003
    pack = L.lib().sifsrl_pack
    assert pack(None, one, one, None) == 1002 and pack(one, None, one, None) == 1002 and pack(one, one, None, None) == 1002


# ---- 3. the public names ---------------------------------------------------------------------------------------------------------
def test_public_interface_and_errors(tmp_path, monkeypatch):
    import sifsr
    from sifsr import lpips, metrics
    E_ = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    assert sig(lpips.LPIPS.__init__)[1:] == [("vgg16_weights", E_), ("lpips_weights", E_), ("mean", lpips.IMAGENET_MEAN),
                                             ("std", lpips.IMAGENET_STD), ("reduction", "mean")]
    assert sig(metrics.aster_table) == [("reference", E_), ("prediction", E_), ("lpips", E_), ("data_range", None)]
    assert sig(metrics.aster_metrics) == [("reference", E_), ("prediction", E_), ("data_range", None)]      # what it was
    assert metrics.METRIC_NAMES_WITH_LPIPS == ("PSNR", "SSIM", "RMSE", "RMSE (low grad per image)", "RMSE (mean grad per image)",
                                               "RMSE (high grad per image)", "GSSIM", "LPIPS", "RMSE_grad")
    assert metrics.METRIC_NAMES == metrics.METRIC_NAMES_WITH_LPIPS[:7] + metrics.METRIC_NAMES_WITH_LPIPS[8:] and len(metrics.METRIC_NAMES) == 8
    assert lpips.IMAGENET_MEAN == R.IMAGENET_MEAN and lpips.IMAGENET_STD == R.IMAGENET_STD
    assert lpips.N_VGG_PARAMS == 14714688 and lpips.N_LIN == 1472 and lpips.CONV_MODULES == R.CONV_MODULES
    assert os.path.samefile(sifsr._lib.header_path("lpips"), os.path.join(ROOT, "include", "sifsr_lpips.h"))

    # both key forms, piq's list, paths: the flat buffers are the generator's
    for prefix in ("features.", ""):
        sd, lin = R.state_dicts(prefix)
        assert np.array_equal(lpips.flatten_vgg16(sd).numpy(), R.vgg_flat())
    assert np.array_equal(lpips.flatten_lin(lin).numpy(), R.lin_flat())
    torch.save(lin, tmp_path / "lpips_weights.pt")
    assert np.array_equal(lpips.flatten_lin(str(tmp_path / "lpips_weights.pt")).numpy(), R.lin_flat())
    model = lpips.LPIPS(sd, lin)
    z = torch.zeros((1, 3, 16, 16))
    with pytest.raises(sifsr.SifsrError, match="no CPU path"):                 # no CPU path
        model(z, z)
    with pytest.raises(ValueError):
        lpips.LPIPS(sd, lin, reduction="median")
    # missing weights say where each file normally comes from; nothing opens a URL
    for bad in ((None, lin), (sd, None), (str(tmp_path / "absent.pth"), lin)):
        with pytest.raises(sifsr.SifsrError, match="vgg16-397923af.pth.*lpips_weights.pt"):
            lpips.LPIPS(*bad)
    part = {k: v for k, v in sd.items() if not k.startswith("28.")}
    with pytest.raises(sifsr.SifsrError, match="28.weight"):
        lpips.LPIPS(part, lin)
    with pytest.raises(sifsr.SifsrError):
        lpips.LPIPS(sd, lin[:4])
    for src in (os.path.join(ROOT, "dropin", "lpips.py"), lpips.__file__):
        text = open(src).read()
        assert "load_state_dict_from_url" not in text.replace("``torch.hub.load_state_dict_from_url``", "") and "urlopen" not in text
        assert "pretrained=True" not in text

    # the drop-in: the reference's constructor line binds; without weights it says what is missing
    spec = importlib.util.spec_from_file_location("dropin_lpips_host", os.path.join(ROOT, "dropin", "lpips.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert sig(mod.LPIPS.__init__)[1:] == [("replace_pooling", False), ("distance", "mse"), ("reduction", "mean"), ("mean", lpips.IMAGENET_MEAN),
                                           ("std", lpips.IMAGENET_STD), ("vgg16_weights", None), ("lpips_weights", None)]
    monkeypatch.delenv("SIFSR_VGG16_WEIGHTS", raising=False)
    monkeypatch.delenv("SIFSR_LPIPS_WEIGHTS", raising=False)
    with pytest.raises(sifsr.SifsrError, match="SIFSR_VGG16_WEIGHTS"):
        mod.LPIPS(distance='mse', reduction='mean', mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0])
    with pytest.raises(NotImplementedError):
        mod.LPIPS(replace_pooling=True)
    with pytest.raises(NotImplementedError):
        mod.LPIPS(distance="mae")
    torch.save(sd, tmp_path / "vgg16.pth")
    monkeypatch.setenv("SIFSR_VGG16_WEIGHTS", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("SIFSR_LPIPS_WEIGHTS", str(tmp_path / "lpips_weights.pt"))
    bound = mod.LPIPS(distance='mse', reduction='mean', mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0])
    assert list(bound._impl.mean) == [0.0, 0.0, 0.0] and list(bound._impl.std) == [1.0, 1.0, 1.0] and bound.reduction == "mean"
