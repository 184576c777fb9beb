#!/usr/bin/env python3
"""Golden vectors for on-device LPIPS, lpips.py:226-292, :351-358 as called at
model_perf_aster_formatds.py:134, :405-410.  Run in the BUILD container only (needs the reference checkout, which never travels to
the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lpips.py

  1. cuts small crops of the reference's ASTER test rasters and makes seeded predictions, as make_golden_eval.py does;
  2. stubs ``torchvision.models`` in sys.modules (the reference imports vgg16 / vgg19 from it; neither is called), imports the
     reference's lpips.py, builds an nn.Sequential with torchvision's module indices holding the closed-form weights of
     tests/lpips_reference.py, and runs the reference's OWN ContentLoss(feature_extractor=that, layers=['3','8','15','22','29'],
     weights=lin, normalize_features=True, distance='mse', reduction='none', mean, std) in float32;
  3. ASSERTS that the float64 restatement's sum equals it to fp32 rounding, for the table path (min/max-normalised, mean 0, std 1)
     and for the three-channel call with the ImageNet statistics;
  4. writes the inputs, the float64 terms and the checksum of the generated weights to tests/golden/golden_lpips_v1.npz (data only).
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np
import torch

REFERENCE = "/root/reference"
# (scene, crop h, crop w, kind): 'k' kelvin pair, 'same' identical pair
CASES = [(0, 41, 43, "k"), (102, 32, 48, "k"), (104, 16, 16, "k"), (109, 24, 17, "k"), (0, 24, 24, "same")]
FP32_BAR = 2e-5        # the reference runs in float32: CPU float32 against float64 measured <= 4e-6 per term, <= 2e-7 on the sum


def reference_module():
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvm.vgg16 = tvm.vgg19 = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("the stub is never called"))
    tv.models = tvm
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tvm)
    spec = importlib.util.spec_from_file_location("reference_lpips", os.path.join(REFERENCE, "lpips.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def vgg_features(R):
    """nn.Sequential with torchvision's vgg16().features module indices 0 .. 29"""
    seq = torch.nn.Sequential()
    idx = 0
    for l, ((ci, co), (w, b)) in enumerate(zip(R.CONV_CHANNELS, R.weights()[0])):
        conv = torch.nn.Conv2d(ci, co, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(w)); conv.bias.copy_(torch.from_numpy(b))
        assert idx == R.CONV_MODULES[l]
        seq.add_module(str(idx), conv); seq.add_module(str(idx + 1), torch.nn.ReLU()); idx += 2
        if l in R.POOL_AFTER:
            seq.add_module(str(idx), torch.nn.MaxPool2d(2, 2)); idx += 1
    assert idx == 30
    return seq


if __name__ == "__main__":
    from tests import lpips_reference as R
    from tests.golden.make_golden_eval import DATA, prediction, read_tiff_f32, valid_crop
    ref = reference_module()
    assert R.weights_sha256() == R.WEIGHTS_SHA256
    model = vgg_features(R)
    lin = [torch.from_numpy(v).view(1, -1, 1, 1) for v in R.weights()[1]]

    def content_loss(x, y, mean, std):
        loss = ref.ContentLoss(feature_extractor=model, layers=["3", "8", "15", "22", "29"], weights=lin, normalize_features=True,
                               distance="mse", reduction="none", mean=mean, std=std)
        with torch.no_grad():
            return loss(torch.from_numpy(x), torch.from_numpy(y)).double().numpy()

    out = {"names": np.array(["relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3", "LPIPS"]), "weights_sha256": np.array(R.WEIGHTS_SHA256)}
    for i, (scene, h, w, kind) in enumerate(CASES):
        img = read_tiff_f32(os.path.join(DATA, f"{scene}_aster_250m.tif")) * np.float32(0.1)
        a = valid_crop(img, h, w)
        assert a is not None, (scene, h, w)
        b = a.copy() if kind == "same" else prediction(a, 300 + i)
        x, y, mini, maxi = R.normalise_pair(a[None], b[None])
        for tag, mean, std in (("pairs", [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]), ("imagenet", R.IMAGENET_MEAN, R.IMAGENET_STD)):
            want = R.terms(x, y, mean, std)
            got = content_loss(x, y, mean, std)
            rel = abs(got[0] - want[0, 5]) / max(want[0, 5], 1e-300)
            assert (kind == "same" and got[0] == 0 and (want == 0).all()) or rel < FP32_BAR, (i, tag, got, want)
            out[f"terms_{tag}{i}"] = want[0]
            print(f"case {i} scene {scene} {a.shape} {kind} {tag}: reference {got[0]:.9g}, restatement {want[0, 5]:.9g} (rel {rel:.1e}), terms "
                  + " ".join(f"{v:.3e}" for v in want[0, :5]))
        out[f"a{i}"], out[f"b{i}"] = a, b
        out[f"minmax{i}"] = np.array([mini[0], maxi[0]], np.float32)
    out["cases"] = np.array([[c[0], c[1], c[2]] for c in CASES])
    out["kinds"] = np.array([c[3] for c in CASES])
    path = os.path.join(HERE, "golden_lpips_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
