"""GPU: the differentiable sensor model at any ratio (include/sifsr_sensor.h, sifsr/sensor.py) against the float64
NumPy restatement tests/sensor_reference.py (held to the reference's recorded outputs and autograd gradients by
tests/test_sensor_host.py), against those recordings themselves (tests/golden/golden_sensor_v1.npz), against the /4 kernels, and,
for the loss and the training step, against the float64 oracle.

Bars.  Gradients, device against restatement, per element: 2^-23 |ref| + 1e-10 max|dout| -- the one rounding to fp32 plus the
reordering of a float64 sum of at most K^2 terms of 1e-16 relative each.  Low-pass forward on 300 K fields: TOL = 2e-4 K, the bar
of tests/test_degrade_gpu.py.  Against the reference's recordings: the host bar of tests/test_sensor_host.py plus the device bar.
Against the /4 kernels (fp32 taps and fp32 accumulation, 18 of each per pixel, each <= 2^-24 max|x|): 4e-6 max|x|.  Loss values,
d loss / d sr and the 53 parameter gradients of a step: 1e-4 relative, the project's parity bar.

Measured on an MI355X over every case of this file (printed by each test): gradients 0.27 - 0.49 of the per-element bar, low-pass
forward <= 1.53e-5 K, against the reference's recorded gradients <= 8.9e-8 (downscale) and 1.8e-7 (low-pass), against the /4 kernels
9.2e-5 K forward and 3.0e-8 in the gradient (low-pass 6.1e-5 K and 6.0e-8), loss scalars <= 2.1e-7 and d loss / d sr <= 2.0e-6
relative, the parameter gradients of the factor-3 step <= 4.9e-6.

Shapes, the smallest at which each part can go wrong: 4 x 4 at 231.656 / 90 (n = hw + 1: every pixel mirrored twice), 12 x 12 and
12 x 40 at 926.25 / 90 (3 outputs, 1 with the crop), input widths 63 / 64 / 65 / 129 and heights BY - 1 / BY / BY + 1 / 2 BY + 1 for
the passes' tiling (BX = 64 lanes, BY = 4 rows per workgroup, read from csrc/degrade.hip), 37 x 37 at factor 1.5 with hkw 16 (34
outputs over one input pixel: longer than any window), the 4 x 3415 strip on which the fp32 source coordinate first floors
differently from the float64 one, and the three cropped cases on 40 x 52."""
import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import adapt_reference as A
from tests import degrade_reference as R
from tests import sensor_reference as SR
from tests.conftest import rel_err
from tests.contract import L, S, bits, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal
from tests.test_degrade_gpu import BX, BY
from tests.test_sensor_host import GOLDEN, HOST_BAR

pytestmark = pytest.mark.gpu
TOL = 2e-4
PARITY = 1e-4
MEAN, STD = A.MEAN, A.STD
ALPHA, GAMMA = 0.5, -0.25


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grad_bar(ref, dout):
    return 2.0 ** -23 * np.abs(ref) + 1e-10 * float(np.abs(dout).max())


def within(tag, got, ref, dout):
    """got fp32 (numpy) against ref float64 under the per-element gradient bar; prints the worst ratio"""
    assert got.shape == ref.shape and got.dtype == np.float32, tag
    ratio = float((np.abs(got.astype(np.float64) - ref) / grad_bar(ref, dout)).max())
    print(f"{tag}: max |device - restatement| = {float(np.abs(got - ref).max()):.3e}, {ratio:.3f} of the bar")
    assert ratio <= 1.0, tag


def downscale_grad(sifsr, x, dout, factor, mtf=0.1, hkw=None, crop=True, valid=None):
    """-> (out, out_valid or None, dx) on the device through autograd"""
    xs = dev(x).requires_grad_(True)
    got = sifsr.sensor.downscale(xs, factor, mtf=mtf, hkw=hkw, crop=crop, valid=dev(valid), fill_value=-1.0, return_valid=valid is not None)
    out, ov = got if valid is not None else (got, None)
    (dx,) = torch.autograd.grad(out, xs, dev(dout))
    torch.cuda.synchronize()
    return out.detach(), ov, dx


def cotangent(shape, factor, hkw, crop, seed):
    oh, ow = R.out_side(shape[-2], factor, hkw, crop), R.out_side(shape[-1], factor, hkw, crop)
    return np.random.RandomState(seed).standard_normal(shape[:-2] + (oh, ow)).astype(np.float32)


# (tag, shape, factor, hkw, crop)
BWD_CASES = [
    ("fine 4x4", (4, 4), R.FINE, None, False),
    ("coarse 12x12", (12, 12), R.COARSE, None, False),
    ("coarse 12x12 crop", (12, 12), R.COARSE, None, True),
    ("coarse 12x40", (2, 12, 40), R.COARSE, None, False),
    ("coarse 12x40 crop", (12, 40), R.COARSE, None, True),
    (f"f2 hkw2 {BY - 1}x{BX - 1}", (BY - 1, BX - 1), 2.0, 2, False),
    (f"f2 hkw2 {BY}x{BX}", (2, 1, BY, BX), 2.0, 2, False),
    (f"f2 hkw2 {BY + 1}x{BX + 1}", (BY + 1, BX + 1), 2.0, 2, False),
    (f"f2 hkw2 {2 * BY + 1}x{2 * BX + 1}", (2 * BY + 1, 2 * BX + 1), 2.0, 2, False),
    (f"fine {2 * BY + 1}x{BX + 1}", (3, 2 * BY + 1, BX + 1), R.FINE, None, False),
    ("f1.5 hkw16 37x37", (37, 37), 1.5, 16, False),
    ("fine 4x3415", (4, 3415), R.FINE, None, False),
    ("lr f2 40x52", (1, 1, 40, 52), 2.0, None, True),
    ("lr f3 40x52", (2, 1, 40, 52), 3.0, None, True),
    ("lr f4 40x52", (1, 1, 40, 52), 4.0, None, True),
    ("lr f2.5 24x32", (24, 32), 2.5, None, True),
]


# ---- 1. the operator and its adjoint ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c[0])
def test_forward_bits_and_backward_against_the_restatement(sifsr, case):
    tag, shape, factor, hkw, crop = case
    x = R.make_field(shape, 7 + shape[-2] + shape[-1])
    dout = cotangent(shape, factor, hkw, crop, 11 + shape[-1])
    out, _, dx = downscale_grad(sifsr, x, dout, factor, 0.1, hkw, crop)
    assert bit_equal(out, sifsr.degrade.degrade(dev(x), factor, mtf=0.1, hkw=hkw, crop=crop))
    ref = SR.downscale_bwd_ref(dout, shape[-2:], factor, 0.1, hkw, crop)
    within(tag, dx.cpu().numpy(), ref, dout)
    # <out, d> = <x, dx>, in float64 from the fp32 results
    o64, x64, d64, g64 = (np.asarray(a, np.float64) for a in (out.cpu().numpy(), x, dout, dx.cpu().numpy()))
    lhs, rhs = float((o64 * d64).sum()), float((x64 * g64).sum())
    slack = 2.0 ** -23 * (float(np.abs(o64 * d64).sum()) + float(np.abs(x64 * g64).sum()))
    print(f"{tag}: <out, d> - <x, dx> = {lhs - rhs:.3e}, allowed {slack:.3e}")
    assert abs(lhs - rhs) <= slack


@pytest.mark.parametrize("case", SR.CASES, ids=lambda c: c[0])
def test_golden_gradients_and_lowpass(sifsr, gold, case):
    """the device against the reference's recorded autograd gradients and low-pass outputs: host bar + device bar"""
    name, shape, factor, _ = case
    x, d_down, d_low = SR.case_input(name)
    out, _, dx = downscale_grad(sifsr, x, d_down, factor, SR.DOWN_MTF)
    ref = gold[name + "_down_grad"].astype(np.float64)
    err = np.abs(dx.cpu().numpy() - ref)
    assert (err <= HOST_BAR["down_grad"] + grad_bar(ref, d_down)).all(), float(err.max())
    assert float(np.abs(out.cpu().numpy() - gold[name + "_down"].astype(np.float64)).max()) <= HOST_BAR["down"] + TOL
    xs = dev(x).requires_grad_(True)
    low = sifsr.sensor.lowpass(xs, factor, SR.LOWPASS_MTF)
    (dlow,) = torch.autograd.grad(low, xs, dev(d_low))
    e_low = float(np.abs(low.detach().cpu().numpy() - gold[name + "_low"].astype(np.float64)).max())
    ref = gold[name + "_low_grad"].astype(np.float64)
    err = np.abs(dlow.cpu().numpy() - ref)
    print(f"{name}: max |device - reference|: downscale gradient {float(np.abs(dx.cpu().numpy() - gold[name + '_down_grad']).max()):.3e}, "
          f"low-pass {e_low:.3e} K, low-pass gradient {float(err.max()):.3e}")
    assert e_low <= HOST_BAR["low"] + TOL
    assert (err <= HOST_BAR["low_grad"] + grad_bar(ref, d_low)).all(), float(err.max())


# ---- 2. validity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(R.FINE, None, False), (3.0, None, True), (2.0, 3, False)], ids=lambda c: f"f{c[0]:.3g}_crop{int(c[2])}")
def test_validity(sifsr, cfg):
    """outputs that hold the fill value pass no gradient: dx is exactly 0 at every invalid pixel, and NaN in dout at the invalid
    outputs or in x at the invalid pixels changes no bit of dx"""
    factor, hkw, crop = cfg
    shape = (2, 40, 52)
    x = R.make_field(shape, 3)
    valid = np.stack([R.quad_valid(40, 52), np.roll(R.quad_valid(40, 52), 5, axis=1)])
    dout = cotangent(shape, factor, hkw, crop, 19)
    out, ov, dx = downscale_grad(sifsr, x, dout, factor, 0.1, hkw, crop, valid)
    want, wv = sifsr.degrade.degrade(dev(x), factor, hkw=hkw, crop=crop, valid=dev(valid), fill_value=-1.0, return_valid=True)
    assert bit_equal(out, want) and bit_equal(ov, wv) and not ov.requires_grad
    ovn = ov.cpu().numpy()
    assert 0 < ovn.sum() < ovn.size
    got = dx.cpu().numpy()
    assert (got[valid == 0] == 0).all() and np.abs(got[valid == 1]).max() > 0
    for b in range(2):
        _, rv = R.degrade_ref(x[b], factor, 0.1, hkw, crop, valid[b])
        assert np.array_equal(ovn[b].astype(bool), rv)
        within(f"map {b}", got[b], SR.downscale_bwd_ref(dout[b], (40, 52), factor, 0.1, hkw, crop, out_valid=rv), dout)
    xn, dn = x.copy(), dout.copy()
    xn[valid == 0] = np.nan
    dn[ovn == 0] = np.nan
    _, ov2, dx2 = downscale_grad(sifsr, xn, dn, factor, 0.1, hkw, crop, valid)
    assert bit_equal(ov2, ov) and bit_equal(dx2, dx) and not torch.isnan(dx2).any()
    # without a map every output counts, the darkened ring included
    _, _, free = downscale_grad(sifsr, x, dout, factor, 0.1, hkw, crop)
    within("no map", free.cpu().numpy(), SR.downscale_bwd_ref(dout, (40, 52), factor, 0.1, hkw, crop), dout)


# ---- 3. the low-pass ---------------------------------------------------------------------------------------------------------------
LOWPASS_CASES = [(hw + 1, 63, hw) for hw in (1, 2, 4, 16)] + [(65, hw + 1, hw) for hw in (1, 2, 4, 16)] + [(17, 17, 16), (2, 2, 1)]


@pytest.mark.parametrize("case", LOWPASS_CASES, ids=lambda c: f"{c[0]}x{c[1]}_hw{c[2]}")
def test_lowpass_forward_and_backward(sifsr, case):
    h, w, hw = case
    factor = 2.5
    x, d = R.make_field((2, h, w), 30 + h + w), np.random.RandomState(h * w).standard_normal((2, h, w)).astype(np.float32)
    xs = dev(x).requires_grad_(True)
    out = sifsr.sensor.lowpass(xs, factor, 0.25, hkw=hw)
    (dx,) = torch.autograd.grad(out, xs, dev(d))
    e = float(np.abs(out.detach().cpu().numpy() - SR.lowpass_ref(x, factor, 0.25, hw)).max())
    print(f"{h}x{w} hw {hw}: max |device - restatement| = {e:.3e} K")
    assert out.shape == xs.shape and e <= TOL
    within(f"{h}x{w} hw {hw} backward", dx.cpu().numpy(), SR.lowpass_bwd_ref(d, factor, 0.25, hw), d)


def test_lowpass_against_the_9_tap_kernels(sifsr):
    x = dev(R.make_field((2, 1, 40, 52), 44)).requires_grad_(True)
    d = torch.from_numpy(np.random.RandomState(45).standard_normal((2, 1, 40, 52)).astype(np.float32)).cuda()
    a = sifsr.sensor.lowpass(x, 4, 0.25)
    b = sifsr.get_output_ftm(x, mtf=0.25)
    (ga,), (gb,) = torch.autograd.grad(a, x, d), torch.autograd.grad(b, x, d)
    ef, eb = float((a.detach().double() - b.detach().double()).abs().max()), float((ga.double() - gb.double()).abs().max())
    print(f"lowpass(4, 0.25) against get_output_ftm: forward {ef:.3e} K, backward {eb:.3e}")
    assert ef <= 4e-6 * float(x.detach().abs().max()) and eb <= 4e-6 * float(d.abs().max())


def test_consistent_with_the_div4_kernels(sifsr):
    x = dev(R.make_field((2, 1, 40, 52), 92)).requires_grad_(True)
    d = torch.from_numpy(np.random.RandomState(93).standard_normal((2, 1, 10, 13)).astype(np.float32)).cuda()
    a = sifsr.sensor.downscale(x, 4)
    b = sifsr.downscale_LST_SR_to_LR(x)
    (ga,), (gb,) = torch.autograd.grad(a, x, d), torch.autograd.grad(b, x, d)
    ef, eb = float((a.detach().double() - b.detach().double()).abs().max()), float((ga.double() - gb.double()).abs().max())
    print(f"downscale(4) against downscale_LST_SR_to_LR: forward {ef:.3e} K, gradient {eb:.3e}")
    assert a.shape == b.shape and ef <= TOL
    assert eb <= 4e-6 * float(d.abs().max())


# ---- 4. the loss and the step -------------------------------------------------------------------------------------------------------
def loss_inputs(seed, factor, B=2, H=24, W=32):
    rs = np.random.RandomState(seed)
    h, w = R.out_side(H, factor, None, True), R.out_side(W, factor, None, True)
    sr, ndvi = rs.standard_normal((B, 1, H, W)), np.clip(rs.standard_normal((B, 1, H, W)), -3, 3)
    lst = rs.standard_normal((B, 1, h, w))
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (sr, lst, ndvi))


@pytest.mark.parametrize("factor", [3.0, 2.5])
@pytest.mark.parametrize("kind", ["sr2", "sr1"])
def test_sif_loss_against_the_float64_oracle(sifsr, kind, factor):
    sr, lst, ndvi = loss_inputs(200 + int(10 * factor), factor)
    assert tuple(lst.shape[-2:]) == ((8, 10) if factor == 3.0 else (10, 13))
    s = sr.cuda().requires_grad_(True)
    ds, pl, loss = sifsr.sensor.sif_loss(kind, s, lst.cuda(), ndvi.cuda(), factor, MEAN, STD, ALPHA, GAMMA)
    assert not ds.requires_grad and not pl.requires_grad and loss.requires_grad and ds.dim() == pl.dim() == loss.dim() == 0
    loss.backward()
    s64 = sr.double().requires_grad_(True)
    ref = SR.loss_ref(kind, s64, lst.double(), ndvi.double(), factor, MEAN, STD, ALPHA, GAMMA)
    (g64,) = torch.autograd.grad(ref[2], s64)
    for name, a, b in zip(("ds", "pl", "loss"), (ds, pl, loss.detach()), (r.detach() for r in ref)):
        print(f"[{kind} x{factor}] {name}: {float(a):.8f} | float64 {float(b):.8f}")
        assert abs(float(a) - float(b)) <= PARITY * abs(float(b)), name
    e = rel_err(s.grad, g64)
    print(f"[{kind} x{factor}] d loss / d sr: rel err {e:.2e}")
    assert e <= PARITY


@pytest.mark.parametrize("kind", ["sr2", "sr1"])
def test_sif_loss_at_factor_4_agrees_with_the_fused_loss(sifsr, kind):
    sr, lst, ndvi = loss_inputs(240, 4.0, H=32, W=40)
    a, b = sr.cuda().requires_grad_(True), sr.cuda().requires_grad_(True)
    got = sifsr.sensor.sif_loss(kind, a, lst.cuda(), ndvi.cuda(), 4, MEAN, STD, ALPHA, GAMMA)
    want = sifsr.sif_loss(kind, b, lst.cuda(), ndvi.cuda(), MEAN, STD, ALPHA, GAMMA)
    got[2].backward()
    want[2].backward()
    for name, x, y in zip(("ds", "pl", "loss"), got, want):
        assert abs(float(x) - float(y)) <= PARITY * abs(float(y)), name
    assert rel_err(a.grad, b.grad) <= PARITY


def test_train_step_at_factor_3_against_the_oracle(sifsr, L):
    """one step on B = 2, HR 24 x 32, LR 8 x 10: the 53 parameter gradients against float64 at the ReLU masks the device took,
    parameters move; with bn_frozen the BatchNorm buffers keep their bits"""
    from tests.test_adapt_gpu import hip_run, named
    from tests.test_model_gpu import make_model
    factor, kind, B, H, W = 3.0, "sr2", 2, 24, 32
    sd = O.synthetic_state(71)
    x, _, _ = A.network_inputs(72, B, H, W)
    lst = torch.from_numpy(np.random.RandomState(73).standard_normal((B, 1, 8, 10)).astype(np.float32))
    ndvi = x[:, 1:2].contiguous()

    def upstream(sr):
        s = sr.detach().clone().requires_grad_(True)
        sifsr.sensor.sif_loss(kind, s, lst.cuda(), ndvi.cuda(), factor, MEAN, STD, ALPHA, GAMMA)[2].backward()
        return s.grad

    r = hip_run(L, sd, x, upstream, frozen=0, want_dx=False)
    ref = lambda sr: SR.loss_ref(kind, sr, lst.double(), ndvi.double(), factor, MEAN, STD, ALPHA, GAMMA)
    sr_ref, _, g_ref, losses_ref = A.network_ref(sd, x, ref, training=True, masks=r["masks"])
    assert rel_err(r["sr"], sr_ref) < PARITY
    g = named(r["grads"])
    errs = {n: rel_err(g[n], g_ref[n]) for n in g}
    worst = max(errs, key=errs.get)
    print(f"[factor 3 step] worst rel err of {len(g)} parameter gradients vs float64 at equal masks: {errs[worst]:.2e} ({worst})")
    assert len(g) == 53 and all(e < PARITY for e in errs.values()), errs
    # the step itself: the same gradients through the module, the losses, parameters move
    m = make_model(sifsr, sd)
    opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
    p0 = m.flat_parameters().detach().clone()
    ds, pl, loss, sr = sifsr.sensor.train_step(m, opt, lst.cuda(), x[:, 0:1].cuda().contiguous(), ndvi.cuda(), A.STATS, ALPHA, GAMMA, factor,
                                               kind=kind, return_sr=True)
    for a, b in zip((ds, pl, loss), losses_ref):
        assert abs(float(a) - float(b)) <= PARITY * abs(float(b))
    assert m.training and not loss.requires_grad and rel_err(sr, sr_ref) < PARITY
    gm = named(m.flat_grad().detach())
    assert all(rel_err(gm[n], g_ref[n]) < PARITY for n in gm)
    assert not torch.equal(m.flat_parameters(), p0)
    # frozen BatchNorm: the buffers keep their bits, the parameters still move
    m2 = make_model(sifsr, sd)
    m2.bn_frozen = True
    opt2 = sifsr.FlatAdam(m2.parameters(), lr=1e-3)
    buffers = {k: v.clone() for k, v in m2.state_dict().items() if "running" in k or "num_batches" in k}
    out = sifsr.sensor.train_step(m2, opt2, lst.cuda(), x[:, 0:1].cuda().contiguous(), ndvi.cuda(), A.STATS, ALPHA, GAMMA, factor, kind="sr1")
    assert len(out) == 3 and all(torch.isfinite(v) for v in out) and not torch.equal(m2.flat_parameters(), p0)
    for k, v in m2.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k


# ---- 5. robustness -------------------------------------------------------------------------------------------------------------------
def test_batch_independence_and_determinism(sifsr):
    x = R.make_field((5, 37, 70), 9)
    valid = np.stack([np.roll(R.quad_valid(37, 70), 3 * b, axis=1) for b in range(5)])
    for factor, hkw, crop in ((2.5, None, True), (R.FINE, None, False)):
        dout = cotangent((5, 37, 70), factor, hkw, crop, 10)
        a = downscale_grad(sifsr, x, dout, factor, 0.1, hkw, crop, valid)
        b = downscale_grad(sifsr, x, dout, factor, 0.1, hkw, crop, valid)
        assert bit_equal(a[2], b[2]) and bit_equal(a[0], b[0])
        for i in range(5):
            one = downscale_grad(sifsr, x[i], dout[i], factor, 0.1, hkw, crop, valid[i])
            assert bit_equal(one[2], a[2][i]) and bit_equal(one[0], a[0][i]), i
        four = downscale_grad(sifsr, x[:, None], dout[:, None], factor, 0.1, hkw, crop)        # (B,C,H,W)
        assert four[2].shape == (5, 1, 37, 70) and bit_equal(four[2][:, 0], downscale_grad(sifsr, x, dout, factor, 0.1, hkw, crop)[2])
    d = np.random.RandomState(4).standard_normal((5, 37, 70)).astype(np.float32)
    xs = dev(x).requires_grad_(True)
    g = torch.autograd.grad(sifsr.sensor.lowpass(xs, 3.0, 0.25), xs, dev(d))[0]
    for i in (0, 4):
        xi = dev(x[i]).requires_grad_(True)
        oi = sifsr.sensor.lowpass(xi, 3.0, 0.25)
        assert bit_equal(oi.detach(), sifsr.sensor.lowpass(dev(x), 3.0, 0.25)[i]) and bit_equal(torch.autograd.grad(oi, xi, dev(d[i]))[0], g[i])


def test_graph_capture_of_forward_and_backward(sifsr):
    """forward plus backward captured once and replayed on new data gives the eager bits: the entry points only enqueue"""
    shape, factor = (2, 1, 24, 32), 3.0
    xs = torch.zeros(shape, device="cuda").requires_grad_(True)
    ds = torch.zeros((2, 1, 8, 10), device="cuda")

    def run():
        out = sifsr.sensor.downscale(xs, factor)
        low = sifsr.sensor.lowpass(xs, factor, 0.25)
        (g,) = torch.autograd.grad([out, low], xs, [ds, xs.detach()])
        return out.detach(), g

    def load(seed):
        with torch.no_grad():
            xs.copy_(dev(R.make_field(shape, seed)))
            ds.copy_(dev(cotangent(shape, factor, None, True, seed)))

    load(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, grad_g = run()
    load(2)
    graph.replay()
    torch.cuda.synchronize()
    out_e, grad_e = run()
    torch.cuda.synchronize()
    assert bit_equal(out_g, out_e) and bit_equal(grad_g, grad_e) and float(grad_e.abs().max()) > 0


# ---- 6. the C entry points: memory contract, errors ---------------------------------------------------------------------------------
# (B, h, w, factor, hkw, crop, with out_valid, NaN in dout under the invalid outputs)
DEGRADE_CONTRACT_SHAPES = [(1, 4, 4, R.FINE, 0, False, False, False), (1, 12, 12, R.COARSE, 0, True, False, False),
                           (2, 40, 52, 2.0, 3, False, True, True), (3, 9, 65, R.FINE, 0, False, False, False),
                           (2, 33, 70, 3.0, 0, True, True, False), (1, 37, 37, 1.5, 16, False, False, False)]
# (B, h, w, factor, hkw)
LOWPASS_CONTRACT_SHAPES = [(1, 2, 2, 1.5, 1), (2, 17, 63, 3.0, 16), (3, 5, 65, 4.0, 0), (1, 40, 52, 2.5, 0)]


def degrade_contract_inputs(i):
    B, h, w, factor, hkw, crop, with_ov, nan = DEGRADE_CONTRACT_SHAPES[i]
    dout = cotangent((B, h, w), factor, hkw or None, crop, 600 + i)
    ov = None
    if with_ov:
        ov = np.stack([R.degrade_ref(np.zeros((h, w)), factor, 0.1, hkw or None, crop, np.roll(R.quad_valid(h, w), b, axis=0))[1]
                       for b in range(B)]).astype(np.uint8)
        if nan:
            dout[ov == 0] = np.nan
    return dout, ov


def degrade_bwd_case(i):
    def make(k):
        B, h, w, factor, hkw, crop, with_ov, _ = DEGRADE_CONTRACT_SHAPES[i]
        dout_np, ov_np = degrade_contract_inputs(i)
        dout = k.t("dout", torch.from_numpy(dout_np))
        ov = k.t("out_valid", torch.from_numpy(ov_np)) if with_ov else None
        dx = k.o("dx", B, h, w)
        need = k.L.call("sifsrt_degrade_bwd_workspace_bytes", B, h, w, factor, hkw, int(crop))
        ws = k.A.scratch(need, "workspace")                       # poisoned scratch: nothing of it may reach the output
        return (lambda: k.L.call("sifsrt_degrade_bwd", dout, ov, dx, ws, need, B, h, w, factor, 0.1, hkw, int(crop), S())), {"dx": dx}
    return make


def lowpass_case(i, name):
    def make(k):
        B, h, w, factor, hkw = LOWPASS_CONTRACT_SHAPES[i]
        src = k.t("x" if name.endswith("fwd") else "dout", torch.from_numpy(R.make_field((B, h, w), 700 + i)))
        dst = k.o("out" if name.endswith("fwd") else "dx", B, h, w)
        need = k.L.call("sifsrt_lowpass_workspace_bytes", B, h, w, factor, hkw)
        ws = k.A.scratch(need, "workspace")
        return (lambda: k.L.call(name, src, dst, ws, need, B, h, w, factor, 0.25, hkw, S())), {"result": dst}
    return make


CONTRACT = {"sifsrt_degrade_bwd": [degrade_bwd_case(i) for i in range(len(DEGRADE_CONTRACT_SHAPES))],
            "sifsrt_lowpass_fwd": [lowpass_case(i, "sifsrt_lowpass_fwd") for i in range(len(LOWPASS_CONTRACT_SHAPES))],
            "sifsrt_lowpass_bwd": [lowpass_case(i, "sifsrt_lowpass_bwd") for i in range(len(LOWPASS_CONTRACT_SHAPES))]}


@pytest.mark.parametrize("idx", range(len(DEGRADE_CONTRACT_SHAPES)))
def test_memory_contract_degrade_bwd(L, idx):
    """dx written in full and nowhere else -- bit-identical and NaN-free under every poison of the output and of the workspace (no
    workspace byte is read before it is written; the NaNs under the invalid outputs reach nothing) --, dout and out_valid untouched,
    nothing outside the buffers and the stated workspace bytes written, the same bits on ordinary allocations, and the result is the
    restatement's"""
    first = run_contract(L, CONTRACT["sifsrt_degrade_bwd"][idx], seed=531 + idx, capacity=64 << 20)
    B, h, w, factor, hkw, crop, with_ov, _ = DEGRADE_CONTRACT_SHAPES[idx]
    dout, ov = degrade_contract_inputs(idx)
    got = first["dx"].cpu().numpy()
    clean = np.nan_to_num(dout)
    for b in range(B):
        ref = SR.downscale_bwd_ref(clean[b], (h, w), factor, 0.1, hkw or None, crop, None if ov is None else ov[b])
        within(f"contract {idx} image {b}", got[b], ref, clean)


@pytest.mark.parametrize("name", ["sifsrt_lowpass_fwd", "sifsrt_lowpass_bwd"])
@pytest.mark.parametrize("idx", range(len(LOWPASS_CONTRACT_SHAPES)))
def test_memory_contract_lowpass(L, idx, name):
    first = run_contract(L, CONTRACT[name][idx], seed=631 + idx, capacity=64 << 20)
    B, h, w, factor, hkw = LOWPASS_CONTRACT_SHAPES[idx]
    src = R.make_field((B, h, w), 700 + idx)
    got = first["result"].cpu().numpy()
    if name.endswith("fwd"):
        assert np.abs(got - SR.lowpass_ref(src, factor, 0.25, hkw or None)).max() <= TOL
    else:
        within(f"contract {idx}", got, SR.lowpass_bwd_ref(src, factor, 0.25, hkw or None), src)


def test_errors_launch_nothing(sifsr, L):
    N = sifsr.sensor
    x = dev(R.make_field((40, 52), 1))
    E = sifsr.SifsrError
    for bad in (lambda: N.downscale(x.cpu(), 2.0), lambda: N.downscale(x[:11].contiguous(), R.COARSE), lambda: N.downscale(x, 1.0),
                lambda: N.downscale(x, 16.5), lambda: N.downscale(x, 2.0, hkw=17), lambda: N.downscale(x, 2.0, mtf=1.0),
                lambda: N.downscale(x.double(), 2.0), lambda: N.downscale(x[:, ::2], 2.0), lambda: N.downscale(x[None, None, None], 2.0),
                lambda: N.lowpass(x.cpu(), 2.0), lambda: N.lowpass(x[:2].contiguous(), 3.0), lambda: N.lowpass(x, 1.0), lambda: N.lowpass(x, 16.5),
                lambda: N.lowpass(x, 2.0, hkw=0), lambda: N.lowpass(x, 2.0, mtf=0.0), lambda: N.lowpass(x.double(), 2.0),
                lambda: N.lowpass(x[:, ::2], 2.0), lambda: N.sif_loss("sr2", x[None, None], x[None, None, :10, :13].contiguous(), x[None, None], 3.0, MEAN, STD, 0.5, 1.0)):
        with pytest.raises(E):
            bad()
    with pytest.raises(NotImplementedError):                                              # what existed keeps its refusals
        sifsr.degrade.degrade(x.clone().requires_grad_(), 2.0)
    # the C entry points: every error returns before a launch
    h, w, B = 40, 52, 2
    lib = L.lib()
    dneed, lneed = lib.sifsrt_degrade_bwd_workspace_bytes(B, h, w, 2.0, 3, 0), lib.sifsrt_lowpass_workspace_bytes(B, h, w, 2.0, 3)
    big, small = torch.full((B, h, w), 77.0, device="cuda"), torch.full((B, 23, 29), 77.0, device="cuda")
    ov = torch.full((B, 23, 29), 77, dtype=torch.uint8, device="cuda")
    ws = torch.full((max(dneed, lneed) + 16,), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    dargs = lambda **kw: [kw.get("dout", p(small)), kw.get("ov", p(ov)), kw.get("dx", p(big)), kw.get("ws", p(ws)), kw.get("nbytes", dneed),
                          kw.get("B", B), kw.get("h", h), kw.get("w", w), kw.get("factor", 2.0), kw.get("mtf", 0.1), kw.get("hkw", 3),
                          kw.get("crop", 0), S()]
    src = torch.full((B, h, w), 77.0, device="cuda")
    largs = lambda **kw: [kw.get("dout", p(src)), kw.get("dx", p(big)), kw.get("ws", p(ws)), kw.get("nbytes", lneed), kw.get("B", B),
                          kw.get("h", h), kw.get("w", w), kw.get("factor", 2.0), kw.get("mtf", 0.25), kw.get("hkw", 3), S()]
    limits = (dict(h=3), dict(w=3), dict(h=16385), dict(factor=1.0), dict(factor=16.5), dict(hkw=17), dict(hkw=-1), dict(mtf=0.0), dict(mtf=1.0),
              dict(B=0), dict(B=65536))
    for fn, args, more in ((lib.sifsrt_degrade_bwd, dargs, (dict(crop=2),)), (lib.sifsrt_lowpass_fwd, largs, ()), (lib.sifsrt_lowpass_bwd, largs, ())):
        for bad in limits + more:
            assert fn(*args(**bad)) == 1001, bad
        for bad in (dict(dout=None), dict(dx=None), dict(ws=None), dict(ws=p(ws) + 8), dict(dout=p(small) + 2), dict(dx=p(big) + 1)):
            assert fn(*args(**bad)) == 1002, bad
        for bad in (dict(nbytes=(dneed if fn is lib.sifsrt_degrade_bwd else lneed) - 1), dict(nbytes=0)):
            assert fn(*args(**bad)) == 1003, bad
    torch.cuda.synchronize()
    for t in (big, small, ov, ws, src):
        assert (t == 77).all()
    assert lib.sifsrt_degrade_bwd(*dargs(ov=None)) == 0
    torch.cuda.synchronize()
    assert (small == 77).all() and (ov == 77).all() and (ws[dneed:] == 77).all() and (big != 77).all()
    big.fill_(77.0)
    assert lib.sifsrt_lowpass_fwd(*largs()) == 0
    torch.cuda.synchronize()
    assert (src == 77).all() and (ws[max(dneed, lneed):] == 77).all() and (big - 77).abs().max() < 1e-4     # a constant stays one
