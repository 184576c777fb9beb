"""What the reference does with data that is not finite, and rule R (include/sifsr_hip.h, "Non-finite data") -- shared by
tests/test_nonfinite_host.py, which pins these facts, and tests/test_nonfinite_gpu.py, which holds the library to them.  Everything
here is the CPU oracle (oracle/sif_oracle.py) and torch; nothing is taken from the library.

Rule R, for every output element of a call run on an input with ONE poisoned element and again on the same input "repaired" (that
element set to 0.0):
  1. where the reference's element is non-finite, ours is non-finite;
  2. where ours is finite, it is bit-equal to our own result on the repaired input -- and the reference's element there does not
     depend on the poison either, which every helper below asserts before it hands out a mask.
A superset is allowed (a whole image may be NaN where the reference's footprint is a 140 x 140 box).

Out of scope: finite inputs that overflow inside the network; the exact footprint; the sharpening, gaps, conserve, scores and LPIPS
families, which define their own behaviour."""
import copy
import functools

import numpy as np
import torch

from oracle import sif_oracle as O

STATE_SEED = 23
MEAN, STD, ALPHA, GAMMA = 307.2378, 5.5698, 0.5, -0.25
NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
NPARAMS = 282705
# eval cases checked against the footprint: (B, H, W), poisoned image, (row, col), channel, value
EVAL_CASES = [((2, 256, 256), 1, (128, 128), 0, NAN), ((2, 256, 256), 0, (100, 201), 1, PINF), ((2, 256, 256), 1, (0, 0), 0, NINF),
              ((1, 40, 72), 0, (0, 0), 1, NAN), ((1, 24, 24), 0, (23, 23), 0, NAN)]
# the issue's table: shape, pixel -> the reference's non-finite box (rows, cols: first, last) of the poisoned image
FOOTPRINTS = {((256, 256), (128, 128)): ((58, 197), (58, 197)), ((256, 256), (100, 201)): ((34, 173), (130, 255)),
              ((256, 256), (0, 0)): ((0, 69), (0, 69))}
TRAIN_SHAPES = [24, 64]
TRAIN_KINDS = ["sr2", "sr1"]
TRAIN_POISONS = ["ndvi", "lst_up", "lst", "weight"]
# parameters / buffers poisoned one at a time in eval mode: state_dict key, flat index
STATE_POISONS = [("db2.lastconv.1.running_mean", 5), ("ub1.convbloc.bloc.4.running_var", 0), ("db1.resblock.doubleconv.bloc.1.weight", 3),
                 ("db3.resblock.doubleconv.bloc.0.weight", 64 * 9 * 7 + 11), ("inbloc.bloc.0.weight", 20), ("outlay.bias", 0)]
TRAIN_WEIGHT = ("db2.resblock.doubleconv.bloc.3.weight", 100)


def state():
    """a fresh copy of the synthetic state every fact here was measured with"""
    return copy.deepcopy(_state())


@functools.lru_cache(maxsize=None)
def _state():
    return O.synthetic_state(STATE_SEED)


@functools.lru_cache(maxsize=None)
def eval_input(shape):
    """seeded x = cat(lst_up, ndvi) of any (B, H, W), float32; read-only"""
    B, H, W = shape
    rs = np.random.RandomState(1000 + 7 * B + 3 * H + W)
    return torch.from_numpy(rs.standard_normal((B, 2, H, W)).astype(np.float32))


def poisoned(x, b, pixel, ch, value):
    y = x.clone()
    y[b, ch, pixel[0], pixel[1]] = value
    return y


def poison_state(sd, key, index, value=NAN):
    sd = copy.deepcopy(sd)
    sd[key] = sd[key].clone()
    sd[key].view(-1)[index] = value
    return sd


def bit_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def eval_footprint(shape, b, pixel, ch, value):
    """-> bool (H, W): where the reference's eval-mode output of image b is non-finite.  Asserts the precondition of rule R: outside
    that mask the reference is bit-equal to its output on the repaired input.  (Images of a batch are independent in eval mode --
    test_nonfinite_host checks that once --, so the reference runs on image b alone.)"""
    x = eval_input(shape)[b:b + 1]
    with torch.inference_mode():
        bad = O.modelb2_forward(state(), poisoned(x, 0, pixel, ch, value), False)[0, 0]
        good = O.modelb2_forward(state(), poisoned(x, 0, pixel, ch, 0.0), False)[0, 0]
    mask = ~torch.isfinite(bad)
    assert bool(torch.isfinite(good).all())
    assert bit_equal(bad[~mask], good[~mask]), "the reference's finite pixels depend on the poison: rule R has no precondition"
    assert bool(mask[pixel[0], pixel[1]])
    return mask


def box_of(mask):
    """-> ((row first, last), (col first, last)) of a boolean mask and whether the mask is exactly that box"""
    r, c = torch.where(mask.any(1))[0], torch.where(mask.any(0))[0]
    box = ((int(r[0]), int(r[-1])), (int(c[0]), int(c[-1])))
    full = int(mask.sum()) == (box[0][1] - box[0][0] + 1) * (box[1][1] - box[1][0] + 1)
    return box, full


def check_rule(ours, repaired, ref_nonfinite, what=""):
    """rule R on one output tensor; ref_nonfinite: bool, broadcastable to it"""
    ours, repaired = ours.detach().cpu(), repaired.detach().cpu()
    nf = ~torch.isfinite(ours)
    ref = torch.as_tensor(ref_nonfinite).expand_as(ours)
    miss = ref & ~nf
    assert not bool(miss.any()), f"{what}: {int(miss.sum())} of {int(ref.sum())} elements are finite where the reference's are not"
    assert bool(torch.isfinite(repaired).all()), f"{what}: the repaired call is not finite"
    assert bit_equal(ours[~nf], repaired[~nf]), f"{what}: finite elements differ from the call on the repaired input"


def all_nonfinite(t, what=""):
    t = t.detach().cpu()
    n = int(torch.isfinite(t).sum())
    assert n == 0, f"{what}: {n} of {t.numel()} elements are finite"


# ---- training --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def train_batch(hr):
    """(lst, lst_up, ndvi) of batch 2; read-only"""
    return O.synthetic_batch(40 + hr, 2, hr)


def train_case(hr, where, value=NAN):
    """-> (sd, lst, lst_up, ndvi) with one element poisoned: `where` in TRAIN_POISONS"""
    sd = state()
    lst, lst_up, ndvi = (t.clone() for t in train_batch(hr))
    if where == "ndvi":
        ndvi[1, 0, hr // 2, 3] = value
    elif where == "lst_up":
        lst_up[0, 0, 5, hr - 1] = value
    elif where == "lst":
        lst[1, 0, hr // 8, 2] = value
    else:
        assert where == "weight", where
        sd = poison_state(sd, *TRAIN_WEIGHT, value)
    return sd, lst, lst_up, ndvi


@functools.lru_cache(maxsize=None)
def train_facts(hr, kind, where):
    """What the reference's training forward + loss + backward gives: {sr_finite, ds, pl, loss (is each finite?), finite_grads}"""
    sd, lst, lst_up, ndvi = train_case(hr, where)
    sr, (ds, pl, loss), grads = O.forward_backward(sd, lst, lst_up, ndvi, MEAN, STD, ALPHA, GAMMA, kind)
    n = sum(int(g.numel()) for g in grads.values())
    assert n == NPARAMS
    return {"sr_finite": int(torch.isfinite(sr).sum()), "sr_numel": sr.numel(), "ds": bool(torch.isfinite(ds)),
            "pl": bool(torch.isfinite(pl)), "loss": bool(torch.isfinite(loss)),
            "finite_grads": sum(int(torch.isfinite(g).sum()) for g in grads.values())}


# ---- single operators ------------------------------------------------------------------------------------------------------------
def huber_ref(a, b):
    """float64 nn.HuberLoss(mean, delta 1) -> (value, d value / d a)"""
    a = a.double().clone().requires_grad_(True)
    v = torch.nn.functional.huber_loss(a, b.double(), reduction="mean", delta=1.0)
    (g,) = torch.autograd.grad(v, a)
    return v.detach(), g


def sif_loss_ref(kind, sr, lst, ndvi, alpha=ALPHA, gamma=GAMMA):
    """float64 oracle loss -> ((ds, pl, loss), d loss / d sr)"""
    s = sr.double().clone().requires_grad_(True)
    out = O.LOSSES[kind](s, lst.double(), ndvi.double(), MEAN, STD, alpha, gamma)
    (g,) = torch.autograd.grad(out[2], s)
    return tuple(o.detach() for o in out), g


def adam_ref(p, g, m, v, lr, step):
    """float64 single-tensor Adam (betas 0.9 / 0.999, eps 1e-8) -> (p, m, v)"""
    p, g, m, v = (t.double().clone() for t in (p, g, m, v))
    m = m + (1 - 0.9) * (g - m)
    v = 0.999 * v + (1 - 0.999) * g * g
    bc1, bc2 = 1 - 0.9 ** step, 1 - 0.999 ** step
    return p - (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + 1e-8)), m, v


def rule_masks(fn, args, which, index, value):
    """The reference side of rule R for an operator: fn(*args) -> tuple of float64 tensors; args[which].view(-1)[index] is poisoned
    with `value`, then repaired with 0.  -> tuple of bool masks (where the reference is non-finite), after asserting that its
    finite elements are those of the repaired call (compared at float64 rounding: summation order aside they are the same sums)."""
    def run(v):
        a = [t.clone() for t in args]
        a[which].view(-1)[index] = v
        return fn(*a)
    bad, good = run(value), run(0.0)
    masks = []
    for b, g in zip(bad, good):
        m = ~torch.isfinite(b)
        assert bool(torch.isfinite(g).all())
        assert torch.allclose(b[~m], g[~m], rtol=1e-12, atol=0.0), "the reference's finite elements depend on the poison"
        masks.append(m)
    return tuple(masks)


@functools.lru_cache(maxsize=None)
def frozen_facts(hr=32):
    """Fine-tuning with frozen BatchNorm (running statistics, forward and backward) on (2, hr, hr) with image 1 poisoned, SR2 loss:
    -> (x poisoned, x repaired, lst, sr mask, dx mask (bool: where the reference is non-finite), the number of finite parameter
    gradients).  In the reference sr[1] and dx[1] are non-finite throughout, sr[0] and dx[0] do not depend on the poison."""
    lst, lst_up, ndvi = O.synthetic_batch(77, 2, hr)
    x = torch.cat((lst_up, ndvi), 1)

    def run(xv):
        sd = state()
        names = O.param_names()
        leaves = {n: sd[n].detach().clone().requires_grad_(True) for n in names}
        work = {k: leaves.get(k, v) for k, v in sd.items()}
        xx = xv.clone().requires_grad_(True)
        sr = O.modelb2_forward(work, xx, training=False)
        loss = O.sr2_loss(sr, lst, xv[:, 1:2].detach(), MEAN, STD, ALPHA, GAMMA)[2]
        g = torch.autograd.grad(loss, [xx] + [leaves[n] for n in names])
        return sr.detach(), g[0], g[1:]
    xp, xr = poisoned(x, 1, (hr // 2, 7), 0, NAN), poisoned(x, 1, (hr // 2, 7), 0, 0.0)
    sr_p, dx_p, gp = run(xp)
    sr_r, dx_r, _ = run(xr)
    sr_mask, dx_mask = ~torch.isfinite(sr_p), ~torch.isfinite(dx_p)
    assert bit_equal(sr_p[~sr_mask], sr_r[~sr_mask])
    # (the loss is a mean over the batch: the clean image's gradient is the same sum in both runs)
    assert torch.allclose(dx_p[~dx_mask], dx_r[~dx_mask], rtol=1e-5, atol=0.0)
    return xp, xr, lst, sr_mask, dx_mask, sum(int(torch.isfinite(t).sum()) for t in gp)


def ratio_loss_masks(kind, shape, args, which, index, loss_fn):
    """Rule R's reference side for the any-ratio loss.  tests/rloss_reference.py applies the sensor operators as DENSE matrices, and
    a dense product multiplies the NaN by the operator's structural zeros too: its non-finite set is whole rows and columns, an
    artefact no convolution has.  So the masks are propagated through the operators' SUPPORT (R != 0, L != 0; the Sobel bank's 3 x 3
    window, zero taps included, as F.conv2d multiplies them) and their adjoints, and the precondition is checked on the dense
    float64 restatement `loss_fn(sr, lst, ndvi) -> (losses (3,), dsr)` with two FINITE values in place of the poison: outside the
    masks nothing may move.  -> (losses mask (3,), dsr mask)"""
    from tests import rloss_reference as RR
    H, W, factor = shape
    (Ry, Ly), (Rx, Lx) = RR.operators(H, factor), RR.operators(W, factor)
    nf = [torch.zeros(a.shape, dtype=torch.bool) for a in args]
    nf[which].view(-1)[index] = True
    n_sr, n_lst, n_ndvi = nf
    through = lambda m, A, B: ((A != 0).double() @ m.double() @ (B != 0).double().T) > 0
    box3 = lambda m: torch.nn.functional.max_pool2d(m.float(), 3, 1, 1) > 0
    e1 = through(n_sr, Ry, Rx) | n_lst
    if kind == "sr2":
        e2 = n_sr | through(n_sr, Ly, Lx) | n_ndvi | through(n_ndvi, Ly, Lx)
        g2 = e2 | through(e2, Ly.T, Lx.T)
    else:
        e2 = box3(n_sr) | box3(n_ndvi)
        g2 = box3(e2)
    dsr = through(e1, Ry.T, Rx.T) | g2
    losses = torch.tensor([bool(e1.any()), bool(e2.any()), bool(e1.any() or e2.any())])
    outs = []
    for v in (0.0, 2.5):
        a = [t.clone() for t in args]
        a[which].view(-1)[index] = v
        outs.append(loss_fn(*a))
    assert torch.equal(outs[0][1][~dsr], outs[1][1][~dsr]) and torch.equal(outs[0][0][~losses], outs[1][0][~losses]), \
        "the reference depends on the poisoned element outside the propagated support"
    assert not torch.equal(outs[0][1][dsr], outs[1][1][dsr])
    return losses, dsr
