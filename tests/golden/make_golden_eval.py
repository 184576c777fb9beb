#!/usr/bin/env python3
"""Golden vectors for the per-pair ASTER evaluation table, model_perf_aster_formatds.py:371-437.
Run in the BUILD container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py

  1. reads ASTER LST rasters of the reference's test_data_formatted/data/*_aster_250m.tif with a stdlib strip reader
     (uncompressed, 32-bit IEEE float), applies the x0.1 scale of :358 and cuts crops holding no nodata (values <= 0);
  2. makes seeded predictions: a blurred copy + noise + a bias, one z-scored pair, one identical pair;
  3. imports the reference's utils.py (stub modules as make_golden.py; skimage.util.arraycrop.crop for gssim) and ASSERTS
     that tests/eval_reference.py's gssim equals us.gssim and its get_output_ftm equals us.get_output_ftm (to float32
     rounding) on every case;
  4. writes inputs, the eight columns, q25 / q75 and the stratum counts to tests/golden/golden_eval_v1.npz (data only).
"""
import os
import struct
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np
from scipy.ndimage import gaussian_filter

DATA = "/root/reference/test_data_formatted/data"


def read_tiff_f32(path):
    """Uncompressed single-band float32 GeoTIFF -> (H, W) float32 (strips, either byte order)."""
    raw = open(path, "rb").read()
    bo = {b"II": "<", b"MM": ">"}[raw[:2]]
    assert struct.unpack(bo + "H", raw[2:4])[0] == 42, "not a classic TIFF"
    ifd = struct.unpack(bo + "I", raw[4:8])[0]
    n = struct.unpack(bo + "H", raw[ifd:ifd + 2])[0]
    sizes = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 11: 4, 12: 8, 16: 8}
    fmt = {1: "B", 2: "c", 3: "H", 4: "I", 11: "f", 12: "d", 16: "Q"}
    tags = {}
    for i in range(n):
        e = ifd + 2 + 12 * i
        tag, typ, cnt = struct.unpack(bo + "HHI", raw[e:e + 8])
        nbytes = sizes.get(typ, 1) * cnt
        off = e + 8 if nbytes <= 4 else struct.unpack(bo + "I", raw[e + 8:e + 12])[0]
        if typ in fmt and typ != 2:
            tags[tag] = struct.unpack(bo + fmt[typ] * cnt, raw[off:off + nbytes])
    W, H = tags[256][0], tags[257][0]
    assert tags.get(259, (1,))[0] == 1 and tags[258][0] == 32 and tags.get(339, (1,))[0] == 3, "not raw float32"
    assert tags.get(277, (1,))[0] == 1, "single band expected"
    data = b"".join(raw[o:o + c] for o, c in zip(tags[273], tags[279]))
    return np.frombuffer(data, dtype=bo + "f4", count=H * W).reshape(H, W).astype(np.float32)


def valid_crop(img, h, w):
    """First (row-major) h x w window with no value <= 0 (nodata); None if there is none."""
    bad = (img <= 0).astype(np.int64)
    S = np.pad(bad.cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    cnt = S[h:, w:] - S[:-h, w:] - S[h:, :-w] + S[:-h, :-w]
    ys, xs = np.nonzero(cnt == 0)
    if len(ys) == 0:
        return None
    return img[ys[0]:ys[0] + h, xs[0]:xs[0] + w].copy()


def prediction(a, seed, sigma=1.2, noise=0.35, bias=0.4):
    rs = np.random.RandomState(seed)
    return (gaussian_filter(a.astype(np.float64), sigma) + noise * rs.standard_normal(a.shape) + bias).astype(np.float32)


# (scene, crop h, crop w, kind): kind 'k' kelvin pair, 'z' z-scored pair, 'same' identical pair
CASES = [(0, 96, 112, "k"), (102, 72, 88, "k"), (104, 64, 80, "z"), (109, 41, 57, "k"), (0, 48, 56, "same")]

if __name__ == "__main__":
    import torch
    from tests import eval_reference as E
    from tests.golden.make_golden import import_reference
    _, us = import_reference()
    sk = sys.modules["skimage"]
    sk.util = types.SimpleNamespace(arraycrop=types.SimpleNamespace(crop=lambda ar, c: ar[c:ar.shape[0] - c, c:ar.shape[1] - c]))
    out = {"names": np.array(E.METRIC_NAMES)}
    for i, (scene, h, w, kind) in enumerate(CASES):
        img = read_tiff_f32(os.path.join(DATA, f"{scene}_aster_250m.tif")) * np.float32(0.1)     # :358
        a = valid_crop(img, h, w)
        assert a is not None, (scene, h, w)
        b = a.copy() if kind == "same" else prediction(a, 100 + i)
        if kind == "z":
            m, s = a.mean(), a.std()
            a, b = ((a - m) / s).astype(np.float32), ((b - m) / s).astype(np.float32)
        row, ex = E.metrics(a, b)
        # pinned by import: the reference's gssim and get_output_ftm
        ref_g = us.gssim(a, b, data_range=ex["R"])
        assert abs(ref_g - row[6]) <= 1e-12 * abs(ref_g), (ref_g, row[6])
        ftm_ref = us.get_output_ftm(torch.tensor(a).unsqueeze(0).unsqueeze(0)).numpy()[0, 0]
        ftm = E.get_output_ftm(a)
        err = np.abs(ftm_ref - ftm).max() / np.abs(ftm_ref).max()
        assert err < 2e-6, err          # an 81-tap float32 conv2d vs two 9-tap passes: a few ulps
        g = E.gradient_map(a)
        nties = g.size - np.unique(g).size
        out[f"a{i}"], out[f"b{i}"] = a, b
        out[f"metrics{i}"] = row
        out[f"q{i}"] = np.array([ex["q25"], ex["q75"]], np.float32)
        out[f"counts{i}"] = np.array(ex["counts"], np.int64)
        print(f"case {i}: scene {scene} {a.shape} {kind}: ties in g {nties}, ftm rel err {err:.1e}, "
              + ", ".join(f"{n} {v:.6g}" for n, v in zip(E.METRIC_NAMES, row)))
    out["cases"] = np.array([[c[0], c[1], c[2]] for c in CASES])
    out["kinds"] = np.array([c[3] for c in CASES])
    path = os.path.join(HERE, "golden_eval_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
