"""GPU: the model, the SIF losses, Huber, Adam and PSNR / SSIM on data that is not finite, held to the reference by rule R
(tests/nonfinite_reference.py; include/sifsr_hip.h, "Non-finite data").  Every expectation comes from the CPU oracle and float64
torch through that module, none from the library.

R: run a call on an input with one poisoned element and again with that element repaired (set to 0).  Where the reference's output
element is non-finite, ours is; where ours is finite, it has the bits of the repaired call.  On top of R: in eval mode and with
frozen BatchNorm the other images of the batch keep their bits; in training mode the whole batch is non-finite; a poisoned parameter
or running statistic poisons every pixel; after a poisoned training step every gradient, parameter and Adam moment is non-finite;
a clean call after a poisoned one gives the clean bits, eagerly and on replay of one captured graph.

Out of scope: finite inputs that overflow inside the network; the exact footprint (the library may poison the whole image); the
sharpening, gaps, conserve, scores and LPIPS families, which have contracts of their own; train.GraphedTrainStep after a poisoned
step (its parameters are NaN by contract).

Addresses: none of the kernels run here indexes memory by a data value -- the model's, the loss, Adam and PSNR / SSIM kernels
compute every index from thread / workgroup ids, shapes and host-built tables, and the flag words the model keeps in its workspace
are compared with zero, never used as an offset --, so a NaN cannot move a load or a store."""
import pytest
import torch

from oracle import sif_oracle as O
from tests import masked_reference as MR
from tests import nonfinite_reference as N
from tests import rloss_reference as RR
from tests.contract import L, S, sifsr  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
STATS = {"mean_lst": N.MEAN, "std_lst": N.STD}


def make_model(pkg, sd, mode="eval", compute="fp32"):
    m = pkg.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1)
    m.load_state_dict(sd)
    m = m.cuda()
    m.compute_dtype = compute
    if mode == "eval":
        m.eval()
    else:
        m.train()
        m.bn_frozen = mode == "frozen"
    return m


def run_eval(m, x):
    with torch.inference_mode():
        return m(x.cuda()).cpu()


# ---- eval, fp32 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_model(sifsr):
    return make_model(sifsr, N.state())


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_eval_64_poisoned_image_only(sifsr, compute):
    m = make_model(sifsr, N.state(), compute=compute)
    x = N.eval_input((3, 64, 64))
    clean = run_eval(m, x)
    assert bool(torch.isfinite(clean).all())
    for (pixel, ch), value in zip((((0, 0), 0), ((31, 37), 1), ((63, 63), 0)), (N.NAN, N.PINF, N.NINF)):
        sr = run_eval(m, N.poisoned(x, 1, pixel, ch, value))
        N.all_nonfinite(sr[1], f"sr[1], {value} at {pixel}")               # (at 64 x 64 this IS the reference's footprint)
        assert N.bit_equal(sr[0], clean[0]) and N.bit_equal(sr[2], clean[2]), "a clean image of the batch changed"
    assert N.bit_equal(run_eval(m, x), clean), "a clean call after poisoned ones"


@pytest.mark.parametrize("case", N.EVAL_CASES, ids=lambda c: f"{c[0]}-{c[2]}")
def test_eval_rule_against_the_footprint(eval_model, case):
    shape, b, pixel, ch, value = case
    x = N.eval_input(shape)
    mask = N.eval_footprint(*case)
    sr = run_eval(eval_model, N.poisoned(x, b, pixel, ch, value))
    repaired = run_eval(eval_model, N.poisoned(x, b, pixel, ch, 0.0))
    ref = torch.zeros(sr.shape, dtype=torch.bool)
    ref[b, 0] = mask
    N.check_rule(sr, repaired, ref, "sr")
    for o in range(shape[0]):
        if o != b:
            assert N.bit_equal(sr[o], repaired[o]), "a clean image of the batch changed"


@pytest.mark.parametrize("key,index", N.STATE_POISONS)
def test_eval_poisoned_state(sifsr, key, index):
    x = N.eval_input((2, 24, 24))
    N.all_nonfinite(run_eval(make_model(sifsr, N.poison_state(N.state(), key, index)), x), key)


@pytest.mark.parametrize("key,index", [N.STATE_POISONS[0], N.STATE_POISONS[3]])
def test_train_forward_poisoned_state(sifsr, key, index):
    m = make_model(sifsr, N.poison_state(N.state(), key, index), mode="train")
    with torch.no_grad():
        N.all_nonfinite(m(N.eval_input((2, 24, 24)).cuda()), key)


# ---- frozen BatchNorm, input gradient ----------------------------------------------------------------------------------------------
def test_frozen_bn_with_input_gradient(sifsr):
    xp, xr, lst, sr_mask, dx_mask, finite_grads = N.frozen_facts()
    assert finite_grads == 0 and bool(sr_mask[1].all()) and not bool(sr_mask[0].any()) and not bool(dx_mask[0].any())
    out = {}
    for tag, x in (("poisoned", xp), ("repaired", xr)):
        m = make_model(sifsr, N.state(), mode="frozen")
        xx = x.cuda().requires_grad_(True)
        sr = m(xx)
        _, _, _, dsr = sifsr.sif_ops.sif_loss_with_grad("sr2", sr, lst.cuda(), xx[:, 1:2].detach(), N.MEAN, N.STD, N.ALPHA, N.GAMMA)
        sr.backward(dsr)
        out[tag] = (sr.detach().cpu(), xx.grad.cpu(), m.flat_grad().cpu())
    N.check_rule(out["poisoned"][0], out["repaired"][0], sr_mask, "sr")
    assert N.bit_equal(out["poisoned"][0][0], out["repaired"][0][0]), "the clean image's prediction changed"
    N.check_rule(out["poisoned"][1], out["repaired"][1], dx_mask, "dx")
    N.all_nonfinite(out["poisoned"][2], "flat_grad")


# ---- training ------------------------------------------------------------------------------------------------------------------------
def train_once(pkg, hr, kind, where, value, capturable, compute="fp32", masked=False):
    sd, lst, lst_up, ndvi = N.train_case(hr, where, value)
    m = make_model(pkg, sd, mode="train", compute=compute)
    opt = pkg.FlatAdam(m.parameters(), lr=1e-4, capturable=capturable)
    kw = {}
    if masked:
        valid = torch.ones((2, 1, hr // 4, hr // 4), dtype=torch.uint8)
        valid[0, 0, 0, :2] = 0
        kw = {"valid": valid.cuda(), "n_valid": torch.tensor(int(valid.sum()), dtype=torch.int64).cuda()}
    ds, pl, loss, sr = pkg.train.train_step(m, opt, lst.cuda(), lst_up.cuda(), ndvi.cuda(), STATS, N.ALPHA, N.GAMMA, kind,
                                            return_sr=True, **kw)
    torch.cuda.synchronize()
    return {"sr": sr.cpu(), "ds": ds.cpu(), "pl": pl.cpu(), "loss": loss.cpu(), "grad": m.flat_grad().cpu(),
            "p": m.flat_parameters().detach().cpu(), "m": opt._m.cpu(), "v": opt._v.cpu()}


def check_poisoned_step(pkg, hr, kind, where, facts, **kw):
    for capturable in (False, True):
        got = train_once(pkg, hr, kind, where, N.NAN, capturable, **kw)
        fixed = train_once(pkg, hr, kind, where, 0.0, capturable, **kw)
        assert all(bool(torch.isfinite(v).all()) for v in fixed.values()), "the repaired step is not finite"
        N.check_rule(got["sr"], fixed["sr"], facts["sr_finite"] == 0, "sr")
        if facts["sr_finite"] == 0:
            N.all_nonfinite(got["sr"], "sr: training mode poisons the whole batch")
        for k in ("ds", "pl", "loss"):
            N.check_rule(got[k], fixed[k], not facts[k], k)
        assert facts["finite_grads"] == 0
        for k, what in (("grad", "flat_grad()"), ("p", "parameters after FlatAdam.step()"), ("m", "exp_avg"), ("v", "exp_avg_sq")):
            N.all_nonfinite(got[k], f"{what}, capturable={capturable}")


@pytest.mark.parametrize("where", N.TRAIN_POISONS)
@pytest.mark.parametrize("kind", N.TRAIN_KINDS)
@pytest.mark.parametrize("hr", N.TRAIN_SHAPES)
def test_poisoned_training_step(sifsr, hr, kind, where):
    check_poisoned_step(sifsr, hr, kind, where, N.train_facts(hr, kind, where))


def test_poisoned_training_step_bf16(sifsr):
    check_poisoned_step(sifsr, 64, "sr2", "ndvi", N.train_facts(64, "sr2", "ndvi"), compute="bf16")


@pytest.mark.parametrize("kind", N.TRAIN_KINDS)
def test_poisoned_masked_training_step(sifsr, kind):
    """the masked loss with the NaN at a VALID LR pixel (lst[1, 0, 3, 2] of 24 x 24; the mask drops lst[0, 0, 0, :2]): as the plain
    loss -- sr and the perceptual term are finite, the consistency term, the loss and every gradient are not"""
    check_poisoned_step(sifsr, 24, kind, "lst", N.train_facts(24, kind, "lst"), masked=True)


# ---- order and capture -------------------------------------------------------------------------------------------------------------
def test_clean_step_after_a_poisoned_forward(sifsr):
    """eager: torch hands the poisoned call's workspace block back to the next call"""
    sd, lst, lst_up, ndvi = N.train_case(24, "ndvi", 0.0)
    x_bad = torch.cat((lst_up, N.train_case(24, "ndvi", N.NAN)[3]), 1).cuda()

    def step(poison_first):
        m = make_model(sifsr, sd, mode="train")
        if poison_first:
            with torch.no_grad():
                N.all_nonfinite(m(x_bad), "sr")
            m.load_state_dict(sd)                                   # (the poisoned forward left NaN running statistics)
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-4)
        out = sifsr.train.train_step(m, opt, lst.cuda(), lst_up.cuda(), ndvi.cuda(), STATS, N.ALPHA, N.GAMMA, "sr2", return_sr=True)
        return [t.cpu() for t in out] + [m.flat_grad().cpu(), m.flat_parameters().detach().cpu()]
    for a, b in zip(step(False), step(True)):
        assert bool(torch.isfinite(a).all()) and N.bit_equal(a, b)


def test_replay_poisoned_then_clean(sifsr):
    m = make_model(sifsr, N.state())
    x = N.eval_input((3, 64, 64))
    eager = run_eval(m, x) * N.STD + N.MEAN
    g = sifsr.predict.GraphedPredictor(m, 3, STATS, hr=64)
    xb = N.poisoned(x, 2, (5, 60), 1, N.NAN).cuda()
    bad = g(xb[:, 0:1], xb[:, 1:2]).cpu()
    N.all_nonfinite(bad[2], "replay on a poisoned buffer")
    assert N.bit_equal(bad[:2], eager[:2])
    xc = x.cuda()
    assert N.bit_equal(g(xc[:, 0:1], xc[:, 1:2]).cpu(), eager), "the replay after a poisoned one"


# ---- operators through the C ABI, against float64 torch ------------------------------------------------------------------------------
def rule_on_operator(ours, ref_fn, args, which, index, value, names, masks=None):
    """ours(*args) -> tuple of device tensors; ref_fn(*args) -> the same outputs in float64 on the host"""
    masks = N.rule_masks(ref_fn, args, which, index, value) if masks is None else masks

    def run(v):
        a = [t.clone() for t in args]
        a[which].view(-1)[index] = v
        return [o.cpu() for o in ours(*[t.cuda() for t in a])]
    for o, r, mk, name in zip(run(value), run(0.0), masks, names):
        N.check_rule(o, r, mk, name)


@pytest.mark.parametrize("n", [1, 255, 4097])
def test_huber(L, n):
    rs = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=rs) * 1.5, torch.randn(n, generator=rs)

    def ours(a, b):
        part = torch.empty(L.call("sifsr_huber_partial_blocks", n), dtype=torch.float32, device="cuda")
        out, ga = torch.empty(1, device="cuda"), torch.empty(n, device="cuda")
        L.call("sifsr_huber_fwd", a, b, 1.0, n, part, out, S())
        L.call("sifsr_huber_bwd", a, b, 1.0, torch.ones(1, device="cuda"), n, ga, S())
        return out, ga

    def ref(a, b):
        v, g = N.huber_ref(a, b)
        return v.reshape(1), g
    for which in (0, 1):
        rule_on_operator(ours, ref, [a, b], which, n // 2, N.NAN, ("huber value", "huber gradient"))
    # an infinite residual is outside R (the reference's gradient THERE is the clamp's +-1 / n, not the repaired call's): directly
    for value in (N.PINF, N.NINF):
        ai = a.clone()
        ai[n // 2] = value
        (v, g), (rv, rg) = [o.cpu() for o in ours(ai.cuda(), b.cuda())], ref(ai, b)
        assert not bool(torch.isfinite(rv).any()) and not bool(torch.isfinite(v).any())
        assert bool(torch.isfinite(rg).all()) and torch.allclose(g.double(), rg, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("which,name", [(0, "sr"), (1, "lst"), (2, "ndvi")])
@pytest.mark.parametrize("hw", [(32, 32), (40, 56)])
@pytest.mark.parametrize("kind", ["sr2", "sr1"])
def test_sif_loss(sifsr, kind, hw, which, name):
    H, W = hw
    rs = torch.Generator().manual_seed(H + W)
    args = [torch.randn(2, 1, H, W, generator=rs) * 1.3, torch.randn(2, 1, H // 4, W // 4, generator=rs),
            torch.randn(2, 1, H, W, generator=rs).clamp(-3, 3)]

    def ours(sr, lst, ndvi):
        ds, pl, loss, dsr = sifsr.sif_ops.sif_loss_with_grad(kind, sr, lst, ndvi, N.MEAN, N.STD, N.ALPHA, N.GAMMA)
        return torch.stack((ds, pl, loss)), dsr

    def ref(sr, lst, ndvi):
        out, g = N.sif_loss_ref(kind, sr, lst, ndvi)
        return torch.stack(out), g
    rule_on_operator(ours, ref, args, which, args[which][1].numel() + args[which].shape[-1] * 5 + 3, N.NAN, ("losses", "dsr"))


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("kind", ["sr2", "sr1"])
def test_masked_sif_loss_valid_pixel(sifsr, kind, which):
    hw = MR.SHAPES[0]
    args = list(MR.loss_inputs(hw))
    valid = MR.loss_mask(hw, "random30")
    n = int((valid != 0).sum())
    # an LR pixel that is valid (poison in lst), or an HR pixel under it (poison in sr / ndvi)
    i = int(torch.nonzero(valid.reshape(-1))[5])
    w = hw[1] // 4
    b, r, c = i // (valid[0].numel()), (i % valid[0].numel()) // w, i % w
    index = i if which == 1 else (b * hw[0] + 4 * r + 1) * hw[1] + 4 * c + 2

    def ours(sr, lst, ndvi):
        ds, pl, loss, dsr = sifsr.sif_ops.masked_sif_loss_with_grad(kind, sr, lst, valid.cuda(), n, ndvi, MR.MEAN, MR.STD, N.ALPHA, N.GAMMA)
        return torch.stack((ds, pl, loss)), dsr

    def ref(sr, lst, ndvi):
        s = sr.double().clone().requires_grad_(True)
        out = MR.masked_loss_ref(kind, s, lst, valid, ndvi, MR.MEAN, MR.STD, N.ALPHA, N.GAMMA)
        (g,) = torch.autograd.grad(out[2], s)
        return torch.stack([o.detach() for o in out]), g
    rule_on_operator(ours, ref, args, which, index, N.NAN, ("losses", "dsr"))


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("shape", [RR.SHAPES[0], RR.SHAPES[1]], ids=["x3", "x2.5"])
@pytest.mark.parametrize("kind", ["sr2", "sr1"])
def test_ratio_sif_loss(sifsr, kind, shape, which):
    args = list(RR.loss_inputs(shape))

    def ours(sr, lst, ndvi):
        return sifsr.rloss.sif_loss_with_grad(kind, sr, lst, ndvi, shape[2], RR.MEAN, RR.STD, N.ALPHA, N.GAMMA)

    def ref(sr, lst, ndvi):
        s = sr.double().clone().requires_grad_(True)
        out = RR.loss_ref(kind, s, lst, None, ndvi, shape[2], RR.MEAN, RR.STD, N.ALPHA, N.GAMMA)
        (g,) = torch.autograd.grad(out[2], s)
        return torch.stack([o.detach() for o in out]), g
    index = args[which][1].numel() + args[which].shape[-1] * 3 + 4
    rule_on_operator(ours, ref, args, which, index, N.NAN, ("losses", "dsr"), masks=N.ratio_loss_masks(kind, shape, args, which, index, ref))


@pytest.mark.parametrize("dev_step", [False, True])
def test_adam_flat(L, dev_step):
    n = 1000
    rs = torch.Generator().manual_seed(3)
    p, g = torch.randn(n, generator=rs), torch.randn(n, generator=rs) * 1e-2
    m, v = torch.randn(n, generator=rs) * 1e-3, torch.rand(n, generator=rs) * 1e-4

    def run(gg):
        pp, mm, vv, gd = p.cuda(), m.cuda(), v.cuda(), gg.cuda()
        if dev_step:
            step, coef = torch.full((1,), 4, dtype=torch.int64, device="cuda"), torch.zeros(2, device="cuda")
            L.call("sifsr_adam_flat_dev", pp, gd, mm, vv, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, coef, 1.0, S())
        else:
            L.call("sifsr_adam_flat", pp, gd, mm, vv, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 5, 1.0, S())
        return pp.cpu(), mm.cpu(), vv.cpu()
    bad = g.clone()
    bad[17], bad[640] = N.NAN, N.PINF
    ref = N.adam_ref(p, bad, m, v, 1e-3, 5)
    clean, got = run(g), run(bad)
    keep = torch.ones(n, dtype=torch.bool)
    keep[17] = keep[640] = False
    for o, c, r, name in zip(got, clean, ref, ("p", "exp_avg", "exp_avg_sq")):
        assert not bool(torch.isfinite(r[~keep]).any()) and bool(torch.isfinite(r[keep]).all())      # the reference
        N.all_nonfinite(o[~keep], name)
        assert N.bit_equal(o[keep], c[keep]), name


def test_psnr_ssim(sifsr):
    rs = torch.Generator().manual_seed(0)
    t = torch.randn(2, 1, 32, 32, generator=rs)
    p = t + 0.1 * torch.randn(2, 1, 32, 32, generator=rs)
    ps, ss = sifsr.metrics.psnr_ssim(p.cuda(), t.cuda())
    assert abs(float(ps) - float(O.psnr_skimage(p, t))) < 1e-3 and abs(float(ss) - float(O.ssim_skimage(p, t))) < 1e-4
    p[1, 0, 9, 20] = N.NAN
    assert torch.isnan(torch.as_tensor(float(O.psnr_skimage(p, t)))) and torch.isnan(torch.as_tensor(float(O.ssim_skimage(p, t))))
    ps, ss = sifsr.metrics.psnr_ssim(p.cuda(), t.cuda())
    assert torch.isnan(ps.cpu()).all() and torch.isnan(ss.cpu()).all()
    # a NaN in the TARGET makes skimage's data range NaN, and with it both values
    t2 = t.clone()
    t2[0, 0, 3, 3] = N.NAN
    p[1, 0, 9, 20] = 0.0
    assert torch.isnan(torch.as_tensor(float(O.psnr_skimage(p, t2)))) and torch.isnan(torch.as_tensor(float(O.ssim_skimage(p, t2))))
    ps, ss = sifsr.metrics.psnr_ssim(p.cuda(), t2.cuda())
    assert torch.isnan(ps.cpu()).all() and torch.isnan(ss.cpu()).all()
