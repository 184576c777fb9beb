#!/usr/bin/env python3
"""Record what the reference's sensor model computes for tests/test_degrade_host.py and tests/test_degrade_gpu.py.
Run in the BUILD container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_degrade.py

Imports the reference's utils.py through make_golden.import_reference() (stub modules for cv2 / skimage / osgeo) and writes
tests/golden/golden_degrade_v1.npz (data only):

  * `names`, and per case of tests/degrade_reference.CASES `<name>_out`, the fp32 output of the reference function on the input that
    degrade_reference.case_input(name) regenerates from its seed, and `<name>_crc`, the CRC-32 of that input: the inputs themselves
    are not stored.  coarse -> downscale_Aster_to_coarse, fine -> downscale_Aster_to_fine, generic -> generic_downscale(hkw=3),
    lr -> downscale_LST_SR_to_LR(factor, mtf) (the cropped form);
  * `shapes`, int32 rows (side, factor id, crop, hw, output side or -1 where the reference refuses the raster): the reference's own
    output size for every side 4 .. 300 at the three factors of degrade_reference.SWEEP_FACTORS, uncropped through the first three
    functions and cropped through downscale_LST_SR_to_LR."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

from tests import degrade_reference as R


def reference_call(us, kind, x, factor, mtf, hkw):
    if kind == "coarse":
        return us.downscale_Aster_to_coarse(x)
    if kind == "fine":
        return us.downscale_Aster_to_fine(x)
    if kind == "generic":
        return us.generic_downscale(torch.from_numpy(x), factor=factor, mtf=mtf, hkw=hkw).numpy()
    return us.downscale_LST_SR_to_LR(torch.from_numpy(x), factor=factor, mtf=mtf).numpy()


def main():
    from make_golden import import_reference
    _, us = import_reference()
    out = {"names": np.array([c[0] for c in R.CASES])}
    worst = 0.0
    for name, kind, shape, factor, mtf, hkw, crop, _ in R.CASES:
        x = R.case_input(name)
        ref = np.asarray(reference_call(us, kind, x, factor, mtf, hkw), np.float32)
        mine, _ = R.degrade_ref(x, factor, mtf, hkw, crop)
        assert ref.shape == mine.shape, (name, ref.shape, mine.shape)
        d = float(np.abs(ref.astype(np.float64) - mine).max())
        worst = max(worst, d)
        print(f"{name}: {shape} -> {ref.shape}, max |reference - restatement| = {d:.3e} K")
        out[name + "_out"] = ref
        out[name + "_crc"] = np.uint32(R.checksum(x))
    print(f"largest deviation {worst:.3e} K")
    rows = []
    for side in range(4, 301):
        for fid, (factor, hkw) in enumerate(R.SWEEP_FACTORS):
            for crop in (0, 1):
                hw = R.half_width(factor, None if crop else hkw)
                x = np.full((side, max(hw + 1, 4)), 300.0, np.float32)
                try:
                    if crop:
                        got = us.downscale_LST_SR_to_LR(torch.from_numpy(x)[None, None], factor=factor, mtf=0.1).shape[-2]
                    elif fid == 2:
                        got = us.generic_downscale(torch.from_numpy(x)[None, None], factor=factor, mtf=0.1, hkw=hkw).shape[-2]
                    else:
                        got = (us.downscale_Aster_to_coarse, us.downscale_Aster_to_fine)[fid](x).shape[-2]
                except RuntimeError:
                    got = -1
                rows.append((side, fid, crop, hw, got))
    out["shapes"] = np.array(rows, np.int32)
    path = os.path.join(HERE, "golden_degrade_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
