#!/usr/bin/env python3
"""Record what the reference's sensor model computes and what torch autograd gives as its gradient for
tests/test_sensor_host.py and tests/test_sensor_gpu.py.  Run in the BUILD container only (needs the reference checkout, which never
travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sensor.py

Imports the reference's utils.py through make_golden.import_reference() and writes tests/golden/golden_sensor_v1.npz (data only):
`names`, and per case of tests/sensor_reference.CASES (five factors on three shapes)

  * `<name>_down` / `<name>_down_grad`: the fp32 output of downscale_LST_SR_to_LR(x, factor=f, mtf=0.1) and its autograd gradient
    with respect to x for the cotangent d_down,
  * `<name>_low` / `<name>_low_grad`: the same for get_output_ftm(x, factor=f, mtf=0.25) and the cotangent d_low,
  * `<name>_crc`: the CRC-32 of (x, d_down, d_low), which sensor_reference.case_input(name) regenerates from the seed: the inputs
    and cotangents themselves are not stored.

Prints the largest deviation of the float64 restatement (tests/sensor_reference.py) from each kind of recording: the bars of
tests/test_sensor_host.py are twice these."""
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
from tests import sensor_reference as SR


def main():
    from make_golden import import_reference
    _, us = import_reference()
    out = {"names": np.array([c[0] for c in SR.CASES])}
    worst = {"down": 0.0, "down_grad": 0.0, "low": 0.0, "low_grad": 0.0}
    for name, shape, factor, _ in SR.CASES:
        x, d_down, d_low = SR.case_input(name)
        xt = torch.from_numpy(x).requires_grad_(True)
        down = us.downscale_LST_SR_to_LR(xt, factor=factor, mtf=SR.DOWN_MTF)
        assert tuple(down.shape) == d_down.shape, (name, tuple(down.shape), d_down.shape)
        (down_grad,) = torch.autograd.grad(down, xt, torch.from_numpy(d_down))
        low = us.get_output_ftm(xt, factor=factor, mtf=SR.LOWPASS_MTF)
        assert tuple(low.shape) == shape
        (low_grad,) = torch.autograd.grad(low, xt, torch.from_numpy(d_low))
        rec = {"down": down.detach().numpy(), "down_grad": down_grad.numpy(), "low": low.detach().numpy(), "low_grad": low_grad.numpy()}
        mine = {"down": SR.downscale_ref(x, factor, SR.DOWN_MTF),
                "down_grad": SR.downscale_bwd_ref(d_down, shape[-2:], factor, SR.DOWN_MTF),
                "low": SR.lowpass_ref(x, factor, SR.LOWPASS_MTF), "low_grad": SR.lowpass_bwd_ref(d_low, factor, SR.LOWPASS_MTF)}
        line = []
        for k, v in rec.items():
            assert v.dtype == np.float32 and v.shape == mine[k].shape, (name, k)
            d = float(np.abs(v.astype(np.float64) - mine[k]).max())
            worst[k] = max(worst[k], d)
            line.append(f"{k} {d:.3e}")
            out[f"{name}_{k}"] = v
        out[name + "_crc"] = np.uint32(SR.checksum(x, d_down, d_low))
        print(f"{name}: {shape} -> {tuple(down.shape)}: max |reference - restatement|: " + ", ".join(line))
    print("largest deviations: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    path = os.path.join(HERE, "golden_sensor_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
