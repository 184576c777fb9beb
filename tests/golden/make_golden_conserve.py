#!/usr/bin/env python3
"""Pin tests/conserve_reference.py to the reference and record what it computes on a few seeded cases.
Run in the BUILD container only (needs the reference checkout, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_conserve.py

  1. imports the reference's utils.py through make_golden.import_reference() (stub modules for cv2 / skimage / osgeo) and ASSERTS,
     on a seeded all-valid 36 x 44 -> 9 x 11 raster in float64, that the restatement's D is the reference's
     downscale_LST_SR_to_LR: the reference convolves with the fp32 cast of its 9 x 9 kernel, the restatement with the outer product
     of the fp32 taps.  Each of the three casts moves a coefficient by at most 2^-25 of itself and the /4 taps have an absolute sum
     of 1.375, so the two differ by at most 3 * 2^-25 * 1.375 * max |x| (1.2e-7 relative) -- the bar; what is seen is the 1e-9
     level of the separable-tap identity tests/test_host_logic.py::test_psf_taps records.  The difference is printed and stored;
  2. ASSERTS that the restatement's U is the bicubic restatement of the input pipeline (oracle.sif_oracle.prepare_tiles:
     F.interpolate bicubic, A = -0.75, half-pixel centres, edge clamp) in float64 on a 48 x 64 raster and on a 3 x 5 one, to 1e-12;
  3. writes inputs and the restatement's outputs over three steps for the cases below to tests/golden/golden_conserve_v1.npz
     (data only, ~130 KB).

Cases: LR 9 x 8 all valid; LR 16 x 16 with a masked block; LR 16 x 16 invalid through sr alone; LR 5 x 7 with relax 0.5."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

from oracle import sif_oracle as O
from tests import conserve_reference as R

CASES = [("9x8", lambda: R.make_case(9, 8, 21) + (None,), 1.0), ("mask_block", lambda: R.hole_case("mask_block"), 1.0),
         ("sr_only", lambda: R.hole_case("sr_only"), 1.0), ("5x7_half", lambda: R.make_case(5, 7, 22) + (None,), 0.5)]


def main():
    from make_golden import import_reference
    _, us = import_reference()
    out = {}
    # 1. D against the reference
    rs = np.random.RandomState(5)
    x = (300.0 + 8.0 * rs.standard_normal((36, 44))).astype(np.float32).astype(np.float64)
    ref = us.downscale_LST_SR_to_LR(torch.from_numpy(x)[None, None]).numpy()[0, 0]
    mine = R.D(x, R.taps32())
    assert ref.dtype == np.float64 and ref.shape == mine.shape == (9, 11)
    d = float(np.abs(ref - mine).max())
    print(f"D: max |restatement - reference| = {d:.3e} K on values near 300 K ({d / 300:.2e} relative)")
    assert d < 3 * 2.0 ** -25 * 1.375 * np.abs(x).max()
    out["d_input"], out["d_reference"], out["d_maxdiff"] = x.astype(np.float32), ref, np.float64(d)
    # 2. U against the pipeline's restatement
    for hw in ((48, 64), (3, 5)):
        r = rs.standard_normal(hw)
        want = O.prepare_tiles(torch.from_numpy(r)[None, None], torch.zeros((1, 1, 4 * hw[0], 4 * hw[1]), dtype=torch.float64))[0, 0].numpy()
        du = float(np.abs(R.U(r) - want).max())
        print(f"U {hw}: max |restatement - F.interpolate bicubic| = {du:.3e}")
        assert du < 1e-12
    # 3. the cases
    out["names"] = np.array([c[0] for c in CASES])
    for i, (name, make, relax) in enumerate(CASES):
        sr, lst, mask = make()
        o, rows, r, c, n = R.conserve_ref(sr, lst, mask, n_iter=3, relax=relax)
        r0 = R.residual(sr, lst, mask, R.taps32())[0]
        out[f"c{i}_sr"], out[f"c{i}_lst"] = sr, lst
        out[f"c{i}_mask"] = np.zeros((0, 0), np.uint8) if mask is None else mask
        out[f"c{i}_relax"] = np.float64(relax)
        out[f"c{i}_r0"], out[f"c{i}_out3"], out[f"c{i}_stats"] = r0, o, rows
        print(f"{name}: counted {int(rows[0, 0])}, RMSE over three steps {rows[:, 2]}")
    path = os.path.join(HERE, "golden_conserve_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
