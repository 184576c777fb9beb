"""Float64 restatements of include/sifsr_adapt.h, on top of oracle/ and the other *_reference files, and the
seeded inputs tests/test_adapt_host.py and tests/test_adapt_gpu.py share.

  * network_ref: O.modelb2_forward with the parameters AND the input as autograd leaves -- training=False is the frozen network
    (running statistics forward and backward), training=True the batch-statistics one; `masks` imposes the ReLU masks a device
    forward took (O.RELU_MASKS), as tests/test_model_gpu.test_train_forward_backward does for the parameter gradients,
  * conv_in_dgrad_ref: autograd through F.conv2d(F.pad(x, replicate), w) -- the adjoint of the padding is torch's, not restated,
  * tile_targets_ref: plain indexing of gaps_reference's filled raster,
  * masked_step_ref: the first optimisation step of adapt_granule: masked_reference's loss through the frozen network + O.AdamState.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sif_oracle as O
from tests import gaps_reference as G
from tests import masked_reference as MR
from tests.test_mosaic_gpu import origins

MEAN, STD = 307.2378, 5.5698
STATS = {"mean_lst": MEAN, "std_lst": STD, "mean_ndvi": 0.4, "std_ndvi": 0.25}
SHAPES = [(1, 24, 24), (2, 40, 56), (2, 32, 48), (3, 64, 96)]     # smallest; odd levels; fused 16->16 at level 0; at levels 0 and 1
OP_SHAPES = [(3, 3), (3, 17), (17, 3), (16, 16), (17, 33), (24, 40), (56, 72)]


# ---- the network ---------------------------------------------------------------------------------------------------------------
def network_inputs(seed, B, H, W):
    """x (B,2,H,W) ~ N(0,1) with the NDVI plane clipped to +-3, lst (B,1,H/4,W/4) ~ N(0,1), dsr (B,1,H,W) ~ N(0,1); numpy stream"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, 2, H, W))
    x[:, 1] = np.clip(x[:, 1], -3, 3)
    lst = rs.standard_normal((B, 1, H // 4, W // 4))
    dsr = rs.standard_normal((B, 1, H, W))
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (x, lst, dsr))


def network_ref(sd, x, upstream, training=False, masks=None, dtype=torch.float64):
    """-> (sr, dx, {name: grad}, value): `upstream` is dsr (a tensor: the gradient of <sr, dsr>) or a function sr -> scalar loss
    (or a tuple whose LAST item is the loss; `value` is then what it returned, detached).  `sd` is not modified."""
    names = O.param_names()
    leaves = {n: sd[n].detach().to(dtype).clone().requires_grad_(True) for n in names}
    work = OrderedDict((k, leaves[k] if k in leaves else (v.to(dtype) if v.is_floating_point() else v.clone())) for k, v in sd.items())
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    prev, O.RELU_MASKS = O.RELU_MASKS, masks
    try:
        sr = O.modelb2_forward(work, xl, training=training)
        if callable(upstream):
            out = upstream(sr)
            loss = out[-1] if isinstance(out, (tuple, list)) else out
            value = tuple(o.detach() for o in out) if isinstance(out, (tuple, list)) else out.detach()
        else:
            loss, value = (sr * upstream.to(dtype)).sum(), None
        g = torch.autograd.grad(loss, [xl] + [leaves[n] for n in names])
    finally:
        O.RELU_MASKS = prev
    return sr.detach(), g[0], dict(zip(names, g[1:])), value


# ---- the first convolution's input gradient ------------------------------------------------------------------------------------
def op_inputs(seed, B, H, W):
    """g, y (B,H,W,16) fp32, scale, shift (16,) fp32, coef (48,) float64 [scale | k1 | k0] with k1, k0 != 0, w (16,2,3,3) fp32"""
    rs = np.random.RandomState(seed)
    g = rs.standard_normal((B, H, W, 16)).astype(np.float32)
    y = rs.standard_normal((B, H, W, 16)).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, 16).astype(np.float32) * np.where(np.arange(16) % 5 == 0, -1, 1).astype(np.float32)
    shift = (0.3 * rs.standard_normal(16)).astype(np.float32)
    coef = np.concatenate([scale.astype(np.float64), 0.05 * rs.standard_normal(16), 0.05 * rs.standard_normal(16)])
    w = (rs.standard_normal((16, 2, 3, 3)) / 3).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (g, y, scale, shift, coef, w))


def conv_in_dgrad_ref(g, y, scale, shift, coef, w):
    """float64 dx (B,2,H,W).  The ReLU mask is the sign of the kernels' fmaf(y, scale, shift): y*scale is exact in float64."""
    g, y, sc, sh, w = (t.double() for t in (g, y, scale, shift, w))
    dz = torch.where(y * sc + sh > 0, g, torch.zeros_like(g))
    dy = (coef[:16] * dz + (coef[16:32] * y + coef[32:48])).permute(0, 3, 1, 2)
    B, _, H, W = dy.shape
    x = torch.zeros((B, 2, H, W), dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w), x, dy)
    return dx


def regions(H, W):
    """{name: bool (H,W)}: corners, edges (without the corners), interior"""
    yy, xx = np.mgrid[0:H, 0:W]
    by, bx = (yy == 0) | (yy == H - 1), (xx == 0) | (xx == W - 1)
    return {"corners": torch.from_numpy(by & bx), "edges": torch.from_numpy(by ^ bx), "interior": torch.from_numpy(~by & ~bx)}


# ---- tile targets ----------------------------------------------------------------------------------------------------------------
GRANULE_HW, WIN = (24, 32), 8


def make_granule(seed=11):
    """-> (lst (24,32) fp32 [K], ndvi (96,128) fp32): with window 8 and no overlap tile (0,0) has no valid pixel, tile (0,1) is half
    cloud, tile (2,3) is gap-free, and a 4 % sprinkle of 0 K pixels covers the rest"""
    rs = np.random.RandomState(seed)
    h, w = GRANULE_HW
    lst = rs.uniform(290.0, 325.0, (h, w)).astype(np.float32)
    lst[rs.uniform(size=(h, w)) < 0.04] = 0.0
    lst[0:8, 0:8] = 0.0
    lst[0:8, 8:12] = np.nan
    lst[16:24, 24:32] = rs.uniform(290.0, 325.0, (8, 8)).astype(np.float32)
    ndvi = np.clip(0.4 + 0.3 * rs.standard_normal((4 * h, 4 * w)), -1.2, 1.2).astype(np.float32)
    return lst, ndvi


def tile_kinds(valid, win, overlap, cover):
    """number of (empty, partly valid, fully valid) tiles of the layout"""
    h, w = valid.shape
    n = [int((valid[y:y + win, x:x + win] != 0).sum()) for y in origins(h, win, overlap, cover) for x in origins(w, win, overlap, cover)]
    return sum(c == 0 for c in n), sum(0 < c < win * win for c in n), sum(c == win * win for c in n)


def tile_targets_ref(filled, valid, active, first, count, win, overlap, cover, mean, std):
    """-> (lst (count,1,win,win) fp32, valid (count,1,win,win) uint8, n_valid int): tile i is active[(first + i) % len(active)];
    lst = (filled - mean) * (1 / std) in fp32 arithmetic, the expression of the input pipeline (mosaic.h)"""
    h, w = filled.shape
    oy, ox = origins(h, win, overlap, cover), origins(w, win, overlap, cover)
    lst = np.zeros((count, 1, win, win), np.float32)
    vt = np.zeros((count, 1, win, win), np.uint8)
    istd = np.float32(1.0) / np.float32(std)
    for i in range(count if len(active) else 0):
        t = int(active[(first + i) % len(active)])
        y, x = oy[t // len(ox)], ox[t % len(ox)]
        lst[i, 0] = (filled[y:y + win, x:x + win].astype(np.float32) - np.float32(mean)) * istd
        vt[i, 0] = valid[y:y + win, x:x + win] != 0
    return lst, vt, int(vt.sum())


def granule_reference(win=WIN, overlap=0, cover=False):
    """the granule through gaps_reference: (lst, ndvi, filled, valid, active)"""
    lst, ndvi = make_granule()
    filled, valid = G.fill_ref(lst)
    _, active, _ = G.select_ref(valid, win, overlap, cover)
    return lst, ndvi, filled, valid, active


# ---- the first adaptation step -------------------------------------------------------------------------------------------------
def calibrated_state(sd, x, iters=40):
    """`sd` with the running statistics of every BatchNorm layer moved onto the statistics of the batch `x` (`iters` training-mode
    forwards of the oracle at momentum 0.1: 1 - 0.9^40 = 98.5 % of the way) -- what a TRAINED model's buffers are for the data it is
    adapted to.  With the raw N(0, 0.1) / U(0.5, 1.5) statistics of O.synthetic_state half of the units are dead on these tiles
    and 62 % of the gradient elements lie below the significance threshold of oracle.checks (its own precondition asks for fewer
    than half); calibrated, 10 % do.  num_batches_tracked stays 0."""
    import copy
    sd = copy.deepcopy(sd)
    with torch.no_grad():
        for _ in range(iters):
            O.modelb2_forward(sd, x, training=True)
    for k in sd:
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.int64)
    return sd


def masked_step_ref(sd, x, lst, valid, kind, alpha, gamma, lr, masks=None):
    """One frozen-statistics step in float64: -> ((ds, pl, loss), grads, update (flat, parameters() order), params after (flat))"""
    ndvi = x[:, 1:2].double()
    loss_fn = lambda sr: MR.masked_loss_ref(kind, sr, lst, valid, ndvi, MEAN, STD, alpha, gamma)
    _, _, grads, losses = network_ref(sd, x, loss_fn, training=False, masks=masks)
    names = O.param_names()
    work = {n: sd[n].double().clone() for n in names}
    before = torch.cat([work[n].reshape(-1) for n in names])
    O.AdamState(names, lr).step(work, grads)
    after = torch.cat([work[n].reshape(-1) for n in names])
    return tuple(float(v) for v in losses), grads, after - before, after
