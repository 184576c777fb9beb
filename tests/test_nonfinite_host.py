"""CPU: what the reference (the oracle and torch) does with one NaN or infinity -- the facts tests/test_nonfinite_gpu.py holds the
library to through the helpers of tests/nonfinite_reference.py.  No kernel runs here.

  * eval forward: the non-finite outputs form a box of up to 140 x 140 around the pixel, clipped at the image edge, in the poisoned
    image alone; everything outside it is bit-equal to the run on the repaired input (the precondition of rule R)
  * a poisoned parameter or running statistic: every pixel of every image
  * training forward + loss + backward: no gradient element is finite, for a NaN in ndvi, lst_up, lst or a conv weight
  * nn.HuberLoss, relu, skimage's PSNR / SSIM
  * the float64 restatements of the masked losses (tests/masked_reference.py, tests/rloss_reference.py) carry a NaN residual at a
    VALID pixel into value and gradient"""
import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import masked_reference as MR
from tests import nonfinite_reference as N
from tests import rloss_reference as RR


@pytest.mark.parametrize("case", N.EVAL_CASES, ids=lambda c: f"{c[0]}-{c[2]}")
def test_eval_footprint_is_a_clipped_box(case):
    shape, b, pixel, ch, value = case
    mask = N.eval_footprint(*case)                       # (asserts independence outside the mask)
    box, full = N.box_of(mask)
    assert full, "the reference's non-finite pixels are not a box"
    assert box[0][1] - box[0][0] < 140 and box[1][1] - box[1][0] < 140
    key = (shape[1:], pixel)
    if key in N.FOOTPRINTS:
        assert box == N.FOOTPRINTS[key]
    if shape[1:] == (40, 72):
        assert int(mask.sum()) == 2800
    if shape[1] <= 64 and shape[2] <= 64:
        assert bool(mask.all())


@pytest.mark.parametrize("value", [N.NAN, N.PINF, N.NINF])
def test_eval_whole_image_at_64_and_the_others_untouched(value):
    shape = (3, 64, 64)
    x = N.eval_input(shape)
    with torch.inference_mode():
        clean = O.modelb2_forward(N.state(), x, False)
        for pixel, ch in (((0, 0), 0), ((31, 37), 1), ((63, 63), 0)):
            bad = O.modelb2_forward(N.state(), N.poisoned(x, 1, pixel, ch, value), False)
            N.all_nonfinite(bad[1], "reference sr[1]")
            assert N.bit_equal(bad[0], clean[0]) and N.bit_equal(bad[2], clean[2])


@pytest.mark.parametrize("key,index", N.STATE_POISONS)
def test_eval_poisoned_state_poisons_every_pixel(key, index):
    x = N.eval_input((2, 24, 24))
    with torch.inference_mode():
        N.all_nonfinite(O.modelb2_forward(N.poison_state(N.state(), key, index), x, False), key)


@pytest.mark.parametrize("where", N.TRAIN_POISONS)
@pytest.mark.parametrize("kind", N.TRAIN_KINDS)
@pytest.mark.parametrize("hr", N.TRAIN_SHAPES)
def test_training_step_has_no_finite_gradient(hr, kind, where):
    f = N.train_facts(hr, kind, where)
    assert f["finite_grads"] == 0 and not f["ds"] and not f["loss"]
    if where == "lst":                                   # the network never sees lst: sr and the perceptual term stay finite
        assert f["sr_finite"] == f["sr_numel"] and f["pl"]
    else:
        assert f["sr_finite"] == 0 and not f["pl"]


def test_huber_relu_psnr_ssim():
    a = torch.linspace(-3, 3, 255)
    b = torch.zeros(255)
    a[17] = N.NAN
    v, g = N.huber_ref(a, b)
    assert torch.isnan(v) and torch.isnan(g[17])
    keep = torch.ones(255, dtype=torch.bool)
    keep[17] = False
    # (clamp(e) * (1 / n) or clamp(e) / n: one float64 rounding apart)
    assert torch.allclose(g[keep], (a.double().clamp(-1, 1) / 255)[keep], rtol=2.0 ** -51, atol=0.0)
    assert torch.isnan(torch.relu(torch.tensor(N.NAN)))
    rs = np.random.RandomState(0)
    t = torch.from_numpy(rs.standard_normal((2, 1, 32, 32)).astype(np.float32))
    p = t + 0.1 * torch.from_numpy(rs.standard_normal((2, 1, 32, 32)).astype(np.float32))
    p[1, 0, 9, 20] = N.NAN
    assert np.isnan(float(O.psnr_skimage(p, t))) and np.isnan(float(O.ssim_skimage(p, t)))


def _residual_nan_reaches_gradient(loss, sr, lst, valid_flat):
    """poison lst at a valid LR pixel: value and gradient of the restatement must be NaN; at an invalid one nothing changes"""
    i_valid, i_invalid = int(torch.nonzero(valid_flat)[0]), int(torch.nonzero(valid_flat == 0)[0])
    out = {}
    for tag, i in (("clean", None), ("valid", i_valid), ("invalid", i_invalid)):
        l = lst.clone()
        if i is not None:
            l.view(-1)[i] = N.NAN
        s = sr.double().clone().requires_grad_(True)
        val = loss(s, l)
        (g,) = torch.autograd.grad(val[2], s)
        out[tag] = (val, g)
    assert torch.isnan(out["valid"][0][0]) and torch.isnan(out["valid"][0][2]) and bool(torch.isnan(out["valid"][1]).any())
    assert torch.equal(out["invalid"][1], out["clean"][1]) and float(out["invalid"][0][2].detach()) == float(out["clean"][0][2].detach())


@pytest.mark.parametrize("kind,alpha,gamma", MR.KINDS[:2])
def test_masked_restatement_propagates_a_valid_nan(kind, alpha, gamma):
    hw = MR.SHAPES[0]
    sr, lst, ndvi = MR.loss_inputs(hw)
    valid = MR.loss_mask(hw, "random30")
    _residual_nan_reaches_gradient(lambda s, l: MR.masked_loss_ref(kind, s, l, valid, ndvi, MR.MEAN, MR.STD, alpha, gamma), sr, lst,
                                   valid.reshape(-1))


@pytest.mark.parametrize("shape", [RR.SHAPES[0], RR.SHAPES[1]])
@pytest.mark.parametrize("kind,alpha,gamma", RR.KINDS[:2])
def test_rloss_restatement_propagates_a_valid_nan(shape, kind, alpha, gamma):
    sr, lst, ndvi = RR.loss_inputs(shape)
    valid = RR.loss_mask(shape, "blobs30")
    _residual_nan_reaches_gradient(lambda s, l: RR.loss_ref(kind, s, l, valid, ndvi, shape[2], RR.MEAN, RR.STD, alpha, gamma), sr, lst,
                                   valid.reshape(-1))
