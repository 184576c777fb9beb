"""Float64 torch restatement of include/sifsr_rloss.h and the seeded inputs tests/test_rloss_host.py and
tests/test_rloss_gpu.py share.  The operators are those of tests/sensor_reference.py -- R = axis_operator(n, factor, 0.1, None,
crop=True) and L = lowpass_operator(n, factor, 0.25), which tests/test_sensor_host.py holds to the reference's recorded outputs and
autograd gradients (tests/golden/golden_sensor_v1.npz) -- applied as dense matrices; the Sobel bank is the oracle's; masks are
applied as the header defines them; the gradient comes from autograd.

    cells(N, n)                the LR cell of every HR index: (Y n) // N, in integers
    counts_ref(valid, H, W)    (n1, n2) by brute force
    residuals_ref              e1 (B,1,h,w) and e2 (B,F,H,W), the arguments of the two Huber terms
    loss_ref                   (ds, pl, loss), differentiable with respect to sr
    loss_inputs / loss_mask / loss_reference    one (shape, kind, alpha, gamma, mask) case, computed once and shared, read-only"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sif_oracle as O
from tests import degrade_reference as R
from tests import sensor_reference as SR

MEAN, STD = 307.2378, 5.5698
B = 2
MAX_FACTOR = 8.0
# (H, W, factor): integer factor; cells of 2 and 3 pixels and the half-pixel phase; a non-terminating ratio; hw = 2; the x4 operator;
# several tiles per image with ragged last tiles in both axes (twice); the largest accepted factor (the LDS-limit instantiation:
# LR tiles of 8 x 8 cells, two per axis, ragged)
SHAPES = [(24, 24, 3.0), (40, 56, 2.5), (32, 48, 8.0 / 3.0), (48, 32, 2.0), (64, 64, 4.0), (96, 120, 3.0), (80, 200, 2.5),
          (80, 104, MAX_FACTOR)]
# the (kind, alpha, gamma) of tests/test_ops_gpu.test_fused_sif_loss, then each term's adjoint alone
KINDS = [("sr2", 0.5, -0.25), ("sr1", 0.99, -0.5), ("sr2", 0.1, -0.4), ("sr2", 1.0, -0.25), ("sr1", 1.0, -0.5), ("sr2", 0.0, -0.25),
         ("sr1", 0.0, -0.5)]
MASKS = ["all", "blobs30", "image0", "single", "none"]


def lr_shape(H, W, factor):
    return R.out_side(H, factor, None, True), R.out_side(W, factor, None, True)


def cells(N, n):
    """-> int array (N,): the LR cell of every HR index"""
    return (np.arange(N, dtype=np.int64) * n) // N


def hr_mask(valid, H, W):
    """valid (..., h, w) -> (..., H, W) bool: is the cell of the pixel valid"""
    v = np.asarray(valid) != 0
    return v[..., cells(H, v.shape[-2])[:, None], cells(W, v.shape[-1])[None, :]]


def counts_ref(valid, H, W):
    """-> (n1, n2) by counting"""
    return int((np.asarray(valid) != 0).sum()), int(hr_mask(valid, H, W).sum())


@functools.lru_cache(maxsize=None)
def operators(n, factor):
    """-> (R (count, n), L (n, n)) float64 torch"""
    return (torch.from_numpy(SR.axis_operator(n, factor, SR.DOWN_MTF, None, True)["R"]),
            torch.from_numpy(SR.lowpass_operator(n, factor, SR.LOWPASS_MTF)))


def residuals_ref(kind, sr, lst, ndvi, factor, mean, std, gamma):
    """float64 torch (B,1,H,W) / (B,1,h,w) -> (e1 (B,1,h,w), e2 (B,F,H,W))"""
    H, W = sr.shape[-2:]
    (Ry, Ly), (Rx, Lx) = operators(H, factor), operators(W, factor)
    dn = (Ry @ (sr * std + mean) @ Rx.T - mean) / std
    if kind == "sr2":
        e2 = (sr - Ly @ sr @ Lx.T) - gamma * (ndvi - Ly @ ndvi @ Lx.T)
    else:
        e2 = O.sobel_bank(sr) - gamma * O.sobel_bank(ndvi)
    return dn - lst, e2


def _huber(e):
    return F.huber_loss(e, torch.zeros_like(e), reduction="none", delta=1.0)


def loss_ref(kind, sr, lst, valid, ndvi, factor, mean, std, alpha, gamma, counts=None):
    """-> (ds, pl, loss) float64 0-d tensors.  valid (B,1,h,w) or None (every cell counts); counts: the (n1, n2) the kernel is told
    (default: the mask's own).  lst under an invalid cell is replaced before it is used; a count <= 0: zeros."""
    sr, lst, ndvi = sr.double(), lst.double(), ndvi.double()
    H, W = sr.shape[-2:]
    v = torch.ones(lst.shape, dtype=torch.bool) if valid is None else (torch.as_tensor(np.asarray(valid)) != 0).reshape(lst.shape)
    n1, n2 = counts_ref(v.numpy(), H, W) if counts is None else (int(c) for c in counts)
    if n1 <= 0 or n2 <= 0:
        z = sr.sum() * 0.0
        return z, z, z
    lst = torch.where(v, lst, torch.zeros_like(lst))
    e1, e2 = residuals_ref(kind, sr, lst, ndvi, factor, mean, std, gamma)
    vh = torch.from_numpy(hr_mask(v.numpy(), H, W))
    ds = (_huber(e1) * v).sum() / n1
    pl = (_huber(e2) * vh).sum() / (e2.shape[1] * n2)
    return ds, pl, alpha * ds + (1 - alpha) * pl


def composed_ref(kind, sr, lst, ndvi, factor, mean, std, alpha, gamma):
    """the unmasked composition, as sensor.sif_loss writes it: plain means of the two Huber terms"""
    e1, e2 = residuals_ref(kind, sr.double(), lst.double(), ndvi.double(), factor, mean, std, gamma)
    ds, pl = _huber(e1).mean(), _huber(e2).mean()
    return ds, pl, alpha * ds + (1 - alpha) * pl


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_inputs(shape, batch=B):
    """(sr, lst, ndvi) float32, the recipe of tests/test_ops_gpu.test_fused_sif_loss: sr ~ 1.3 N(0,1), so |e| > 1 on a fraction"""
    H, W, factor = shape
    h, w = lr_shape(H, W, factor)
    rs = np.random.RandomState(19 + H + 3 * W)
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    return rnd(batch, 1, H, W) * 1.3, rnd(batch, 1, h, w), rnd(batch, 1, H, W).clamp(-3, 3)


def blobs(h, w, rs, share=0.3):
    """(h, w) uint8, about `share` invalid in square blobs of 1 .. 4 cells a side; valid bytes of any non-zero value"""
    v = rs.randint(1, 256, (h, w)).astype(np.uint8)
    while (v == 0).mean() < share:
        s = rs.randint(1, 5)
        y, x = rs.randint(0, h), rs.randint(0, w)
        v[y:y + s, x:x + s] = 0
    return v


@functools.lru_cache(maxsize=None)
def loss_mask(shape, mask):
    """valid (B,1,h,w) uint8.  all: ones; blobs30: about 30 % invalid in seeded blobs; image0: image 0 wholly invalid, image 1
    valid; single: ONE valid cell, in image 1 -- the one whose consistency residual is largest: it lies in the linear Huber branch,
    because the relative error of a one-element Huber mean in the quadratic branch is 2 d / |e| (d the absolute error of e), so a
    small |e| would measure that conditioning and not the masking; none: zeros."""
    H, W, factor = shape
    h, w = lr_shape(H, W, factor)
    if mask == "all":
        return torch.ones((B, 1, h, w), dtype=torch.uint8)
    if mask == "blobs30":
        rs = np.random.RandomState(H * W)
        return torch.from_numpy(np.stack([blobs(h, w, rs) for _ in range(B)])[:, None])
    v = torch.zeros((B, 1, h, w), dtype=torch.uint8)
    if mask == "image0":
        v[1] = 1
    elif mask == "single":
        sr, lst, ndvi = loss_inputs(shape)
        e1, _ = residuals_ref("sr1", sr.double(), lst.double(), ndvi.double(), factor, MEAN, STD, 0.0)
        v[1].view(-1)[int(e1[1].abs().argmax())] = 1
    else:
        assert mask == "none", mask
    return v


@functools.lru_cache(maxsize=None)
def loss_reference(shape, kind, alpha, gamma, mask):
    """-> (sr, lst, ndvi, valid, (n1, n2), (ds, pl, loss) floats, d loss / d sr float64), computed once and shared"""
    sr, lst, ndvi = loss_inputs(shape)
    valid = loss_mask(shape, mask)
    s = sr.double().requires_grad_(True)
    out = loss_ref(kind, s, lst, valid, ndvi, shape[2], MEAN, STD, alpha, gamma)
    (g,) = torch.autograd.grad(out[2], s)
    return sr, lst, ndvi, valid, counts_ref(valid.numpy(), shape[0], shape[1]), tuple(float(o.detach()) for o in out), g
