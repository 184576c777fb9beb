"""NumPy restatement of include/sifsr_gaps.h, what tests/test_gaps_gpu.py compares the kernels with bit for bit,
and the seeded rasters both test files use.

  * fill_ref, written two ways -- the push-pull pyramid recurrence of the header (`fill_ref`) and its closed form, pixel by pixel
    (`fill_ref_closed`); tests/test_gaps_host.py holds them to each other,
  * select_ref: the active tiles of a layout,
  * blend_gaps_ref: the float64 blend of tests/test_mosaic_gpu.blend_ref over the active tiles, masked.

Float64 sums of these rasters are exact (values in [250, 350] K are multiples of 2^-15 below 2^9, at most 15 000 of them), so
np.sum's own order does not matter and the two forms -- and any kernel -- must agree to the bit."""
import numpy as np

from tests.test_mosaic_gpu import blend_ref, origins


# ---- validity and fill -------------------------------------------------------------------------------------------------------
def valid_ref(lst, mask=None):
    v = np.isfinite(lst) & (lst != 0)
    if mask is not None:
        v &= np.asarray(mask) != 0
    return v.astype(np.uint8)


def _mean32(S, c):
    """(float)(S / c) where c > 0, float64 division, one rounding; 0 elsewhere"""
    q = np.zeros(S.shape, np.float64)
    np.divide(S, c.astype(np.float64), out=q, where=c > 0)
    return q.astype(np.float32)


def pyramid_ref(lst, valid):
    """[(S float64, c int64)] for level 0, 1, ..., top (1 x 1; a 1 x 1 raster has one level above it)"""
    S = np.where(valid != 0, lst.astype(np.float64), 0.0)        # (np.where: a NaN / inf pixel contributes nothing)
    c = (valid != 0).astype(np.int64)
    levels = [(S, c)]
    while True:
        h, w = S.shape
        H, W = (h + 1) // 2, (w + 1) // 2
        Sp, cp = np.zeros((2 * H, 2 * W)), np.zeros((2 * H, 2 * W), np.int64)     # children past the ragged edge: nothing
        Sp[:h, :w], cp[:h, :w] = S, c
        S = Sp.reshape(H, 2, W, 2).sum(axis=(1, 3))
        c = cp.reshape(H, 2, W, 2).sum(axis=(1, 3))
        levels.append((S, c))
        if H == 1 and W == 1:
            return levels


def fill_ref(lst, mask=None, return_level=False):
    """the recurrence: F_l = (float)(S_l / c_l) where c_l > 0, else F_{l+1} of the parent; filled = lst where valid, else F_1 of
    the parent.  -> (filled float32, valid uint8[, the level each pixel's value comes from: 0 = itself, -1 = nothing valid])"""
    lst = np.asarray(lst, np.float32)
    valid = valid_ref(lst, mask)
    levels = pyramid_ref(lst, valid)
    top = len(levels) - 1
    F = _mean32(*levels[top])                                       # nothing valid anywhere: 0
    src = np.where(levels[top][1] > 0, top, -1)
    for l in range(top - 1, -1, -1):
        S, c = levels[l]
        h, w = S.shape
        parent = np.repeat(np.repeat(F, 2, 0), 2, 1)[:h, :w]
        psrc = np.repeat(np.repeat(src, 2, 0), 2, 1)[:h, :w]
        if l == 0:
            F, src = np.where(valid != 0, lst, parent), np.where(valid != 0, 0, psrc)
        else:
            F, src = np.where(c > 0, _mean32(S, c), parent), np.where(c > 0, l, psrc)
    F = F.astype(np.float32)
    return (F, valid, src) if return_level else (F, valid)


def fill_ref_closed(lst, mask=None):
    """the closed form: an invalid pixel gets the mean of the valid pixels of the smallest aligned dyadic block around it that
    holds one (float64 sum, one division, one rounding); none anywhere: 0"""
    lst = np.asarray(lst, np.float32)
    valid = valid_ref(lst, mask)
    h, w = lst.shape
    filled = lst.copy()
    for y, x in zip(*np.nonzero(valid == 0)):
        filled[y, x] = 0.0
        l = 1
        while True:
            y0, x0 = (y >> l) << l, (x >> l) << l
            v = valid[y0:y0 + (1 << l), x0:x0 + (1 << l)] != 0          # (slices clip at the ragged edge)
            if v.any():
                block = lst[y0:y0 + (1 << l), x0:x0 + (1 << l)]
                filled[y, x] = np.float32(block[v].astype(np.float64).sum() / np.float64(v.sum()))
                break
            if (1 << l) >= h and (1 << l) >= w:
                break
            l += 1
    return filled, valid


# ---- select ------------------------------------------------------------------------------------------------------------------
def select_ref(valid, win, overlap, cover):
    """-> (slot (T,) int32, active (n,) int32, n): a tile is active iff its window holds a valid pixel"""
    h, w = valid.shape
    oy, ox = origins(h, win, overlap, cover), origins(w, win, overlap, cover)
    on = np.array([(valid[y:y + win, x:x + win] != 0).any() for y in oy for x in ox])
    active = np.nonzero(on)[0].astype(np.int32)
    slot = np.full(len(on), -1, np.int32)
    slot[active] = np.arange(len(active), dtype=np.int32)
    return slot, active, len(active)


def upsampled(valid):
    """the (h, w) mask on the (4h, 4w) output grid, bool"""
    return np.repeat(np.repeat(np.asarray(valid) != 0, 4, 0), 4, 1)


def blend_gaps_ref(sr, slot, valid, win, overlap, cover, mean, std, fill_value):
    """sr (>= n,1,4win,4win) compact -> (out float64 (4h,4w), covered mask): blend_ref's formula over the active tiles (a skipped
    tile touches invalid pixels only), fill_value where the LST pixel is invalid, 0 where valid and uncovered"""
    sr = np.asarray(sr, np.float64)
    full = np.zeros((len(slot),) + sr.shape[1:])
    full[slot >= 0] = sr[slot[slot >= 0]]
    out, m = blend_ref(full, valid.shape, win, overlap, cover, mean, std)
    return np.where(upsampled(valid), out, fill_value), m


# ---- the rasters -------------------------------------------------------------------------------------------------------------
def _lst(seed, h, w):
    return np.random.RandomState(seed).uniform(250.0, 350.0, (h, w)).astype(np.float32)


def _sparse_mask(seed, h, w):
    return (np.random.RandomState(seed).uniform(size=(h, w)) > 0.03).astype(np.uint8)


def make_rasters():
    """{name: (lst float32 (h,w), mask uint8 (h,w))}: LST in [250, 350] K with the planted gaps of the table in
    tests/test_gaps_gpu.py; the mask (a 3 % sprinkle of zeros, on 150x100 also a stripe) is for the runs `with mask`."""
    r = {}
    a = _lst(1, 37, 50)
    for y, x in ((0, 0), (36, 49), (0, 17), (20, 0), (20, 23)):          # corners, edges, interior
        a[y, x] = 0.0
    r["37x50"] = (a, _sparse_mask(11, 37, 50))
    a = _lst(2, 45, 61)
    a[0:16, 16:32] = 0.0                                                # one whole tile of window 16
    a[30:35, 27:36] = 0.0                                               # 5 x 9 across the 32-boundary of both axes
    r["45x61"] = (a, _sparse_mask(12, 45, 61))
    a = _lst(3, 150, 100)
    a[60:130, 20:100] = 0.0                                             # 70 x 80: holds the whole 64-block (1, 1) = rows 64.., cols 64..99
    a[5, 5], a[10, 90] = np.nan, np.inf
    m = _sparse_mask(13, 150, 100)
    m[140:143, :] = 0
    r["150x100"] = (a, m)
    r["64x64"] = (_lst(4, 64, 64), _sparse_mask(14, 64, 64))
    r["40x40"] = (np.zeros((40, 40), np.float32), _sparse_mask(15, 40, 40))
    a = np.zeros((33, 33), np.float32)
    a[32, 32] = 301.25
    r["33x33"] = (a, np.ones((33, 33), np.uint8))
    return r


def min_chebyshev_distance_mask(valid, d):
    """the valid pixels at least d pixels (Chebyshev, hence also Euclidean) from every invalid one"""
    bad = np.asarray(valid) == 0
    h, w = bad.shape
    near = np.zeros_like(bad)
    for dy in range(-(d - 1), d):
        for dx in range(-(d - 1), d):
            ys, xs = slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx))
            yd, xd = slice(max(0, -dy), h + min(0, -dy)), slice(max(0, -dx), w + min(0, -dx))
            near[yd, xd] |= bad[ys, xs]
    return ~near
