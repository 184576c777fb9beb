"""Restatement of include/sifsr_masked.h and the seeded inputs tests/test_masked_host.py and
tests/test_masked_gpu.py share.

  * fill_patches_ref: tests/gaps_reference.fill_ref applied per patch, plus NumPy float64 moments of the valid pixels.  The patches
    hold temperatures in [250, 350] K -- multiples of 2^-15 below 2^9, at most 4096 of them --, so every float64 sum is exact and
    `filled`, `count`, `mean`, `min`, `max` are bit-defined; only M2 depends on the order of summation.
  * masked_loss_ref: the masked SIF loss in float64 torch, built from the oracle's operators (downscale_LST_SR_to_LR,
    get_output_ftm, sobel_bank) and the element-wise Huber with the masked mean; the gradient comes from autograd.
  * loss_inputs / loss_mask / loss_reference: the inputs and the reference of one (shape, kind, mask) case, computed once, and
    residuals_ref: the arguments of the two Huber terms, for the
    condition that both branches are reached."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sif_oracle as O
from tests import gaps_reference as G

MEAN, STD = 307.2378, 5.5698


# ---- per-patch fill and moments ------------------------------------------------------------------------------------------------
def moments_ref(lst, valid):
    """[count, mean, M2, min, max] over the valid pixels of one patch, float64; none: [0, 0, 0, +inf, -inf]"""
    v = lst[valid != 0].astype(np.float64)
    if v.size == 0:
        return np.array([0.0, 0.0, 0.0, np.inf, -np.inf])
    mean = v.sum() / np.float64(v.size)
    return np.array([v.size, mean, ((v - mean) ** 2).sum(), v.min(), v.max()], np.float64)


def fill_patches_ref(lst):
    """lst (N,w,w) float32 -> (filled (N,w,w) float32, valid (N,w,w) uint8, moments (N,5) float64): fill_ref per patch"""
    lst = np.asarray(lst, np.float32)
    filled, valid = zip(*(G.fill_ref(p) for p in lst))
    filled, valid = np.stack(filled), np.stack(valid)
    return filled, valid, np.stack([moments_ref(p, v) for p, v in zip(lst, valid)])


def make_patches(w, seed=0):
    """(4,w,w) float32 in [250, 350] K: all valid; none valid; one valid pixel (the last one: its fill is the top level); a hole of
    about a third of the side that holds whole 2 x 2 blocks and ends at odd coordinates, 5 % scattered zeros, one NaN and one +inf"""
    rs = np.random.RandomState(1000 * w + seed)
    p = rs.uniform(250.0, 350.0, (4, w, w)).astype(np.float32)
    p[1] = 0.0
    one = p[2, w - 1, w - 1]
    p[2] = 0.0
    p[2, w - 1, w - 1] = one
    a = 2 * (w // 8)
    b = a + max(3, w // 3)
    p[3, a:b, a:b + 1] = 0.0
    p[3][rs.uniform(size=(w, w)) < 0.05] = 0.0
    p[3, 0, w - 1], p[3, w - 1, 0] = np.nan, np.inf
    return p


def holes_10_percent(n, w, seed=0):
    """(n,1,w,w) float32: valid values drawn from [290, 310] K and EXACTLY 10 % of all pixels set to 0 (n w w must be a multiple
    of 10), spread unevenly over the patches"""
    rs = np.random.RandomState(seed)
    p = rs.uniform(290.0, 310.0, (n, 1, w, w)).astype(np.float32)
    assert p.size % 10 == 0
    flat = p.reshape(-1)
    flat[rs.permutation(flat.size)[:flat.size // 10]] = 0.0
    return p


def gather_moments(lst, ndvi):
    """the (N,8) rows sifsrp_gather leaves, restated: [count, mean, M2, min, max] of ALL LST pixels, [mean, M2] of NDVI, 0"""
    rows = []
    for a, b in zip(np.asarray(lst, np.float64).reshape(len(lst), -1), np.asarray(ndvi, np.float64).reshape(len(ndvi), -1)):
        rows.append([a.size, a.mean(), ((a - a.mean()) ** 2).sum(), a.min(), a.max(), b.mean(), ((b - b.mean()) ** 2).sum(), 0.0])
    return np.array(rows, np.float64)


# ---- masked loss ---------------------------------------------------------------------------------------------------------------
def residuals_ref(kind, sr, lst, ndvi, mean, std, gamma):
    """the arguments of the two Huber terms: e1 (B,1,H/4,W/4) = dn - lst and e2 (B,F,H,W), exactly what O.LOSSES[kind] forms"""
    down = (O.downscale_LST_SR_to_LR(sr * std + mean) - mean) / std
    if kind == "sr2":
        e2 = (sr - O.get_output_ftm(sr, mtf=0.25)) - gamma * (ndvi - O.get_output_ftm(ndvi, mtf=0.25))
    else:
        e2 = O.sobel_bank(sr) - gamma * O.sobel_bank(ndvi)
    return down - lst, e2


def _huber(e):
    return F.huber_loss(e, torch.zeros_like(e), reduction="none", delta=1.0)


def masked_loss_ref(kind, sr, lst, valid, ndvi, mean, std, alpha, gamma, n=None):
    """-> (ds, pl, loss) float64 0-d tensors.  valid (B,1,H/4,W/4), any non-zero = valid; n: the count the kernel is told (default:
    the mask's own).  lst at invalid pixels is replaced before it is used, so a NaN there reaches nothing; n == 0: zeros."""
    sr, lst, ndvi = sr.double(), lst.double(), ndvi.double()
    v = (torch.as_tensor(valid) != 0).reshape(lst.shape)
    n = int(v.sum()) if n is None else int(n)
    if n == 0:
        z = sr.sum() * 0.0
        return z, z, z
    lst = torch.where(v, lst, torch.zeros_like(lst))
    e1, e2 = residuals_ref(kind, sr, lst, ndvi, mean, std, gamma)
    vh = v.repeat_interleave(4, 2).repeat_interleave(4, 3)
    ds = (_huber(e1) * v).sum() / n
    pl = (_huber(e2) * vh).sum() / (16 * e2.shape[1] * n)
    return ds, pl, alpha * ds + (1 - alpha) * pl


SHAPES = [(40, 24), (64, 64), (100, 36)]                      # partial 32 x 32 tiles; the last row of tiles holds partial LR blocks
KINDS = [("sr2", 0.5, -0.25), ("sr1", 0.99, -0.5), ("sr2", 0.1, -0.4)]     # the (alpha, gamma) pairs of test_fused_sif_loss
MASKS = ["random30", "image0", "single"]
B = 2


@functools.lru_cache(maxsize=None)
def loss_inputs(hw):
    """(sr, lst, ndvi) float32, the recipe of tests/test_ops_gpu.test_fused_sif_loss: sr ~ 1.3 N(0,1), so |e| > 1 on a fraction"""
    H, W = hw
    rs = np.random.RandomState(6 + H)
    rnd = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    return rnd(B, 1, H, W) * 1.3, rnd(B, 1, H // 4, W // 4), rnd(B, 1, H, W).clamp(-3, 3)


@functools.lru_cache(maxsize=None)
def loss_mask(hw, mask):
    """valid (B,1,H/4,W/4) uint8.  random30: about 30 % invalid, seeded, valid bytes of any non-zero value; image0: image 0 invalid,
    image 1 valid; single: ONE valid pixel, in image 1 -- the one whose consistency residual is largest, because the relative
    error of a one-element Huber mean in the quadratic branch is 2 d / |e| (d, a few 1e-6, is the fp32 error of the de-normalised
    blur at 307 K), so a small |e| would measure that conditioning and not the masking."""
    H, W = hw
    h, w = H // 4, W // 4
    if mask == "random30":
        rs = np.random.RandomState(H * W)
        return torch.from_numpy(((rs.uniform(size=(B, 1, h, w)) > 0.3) * rs.randint(1, 256, (B, 1, h, w))).astype(np.uint8))
    v = torch.zeros((B, 1, h, w), dtype=torch.uint8)
    if mask == "image0":
        v[1] = 1
    else:
        sr, lst, ndvi = loss_inputs(hw)
        e1, _ = residuals_ref("sr2", sr.double(), lst.double(), ndvi.double(), MEAN, STD, 0.0)      # (e1 is the same for both kinds)
        v[1].view(-1)[int(e1[1].abs().argmax())] = 1
    return v


@functools.lru_cache(maxsize=None)
def loss_reference(hw, kind, alpha, gamma, mask):
    """-> (sr, lst, ndvi, valid, n, (ds, pl, loss) floats, d loss / d sr float64), computed once and shared"""
    sr, lst, ndvi = loss_inputs(hw)
    valid = loss_mask(hw, mask)
    s = sr.double().requires_grad_(True)
    out = masked_loss_ref(kind, s, lst, valid, ndvi, MEAN, STD, alpha, gamma)
    (g,) = torch.autograd.grad(out[2], s)
    return sr, lst, ndvi, valid, int((valid != 0).sum()), tuple(float(o.detach()) for o in out), g
