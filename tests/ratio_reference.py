"""float64 NumPy restatement of include/sifsr_ratio.h: the integer-phase bicubic resampling matrix per axis,
the per-tile input pipeline, the tile layout mapped through p / q, the feathered blend and the validity mapping.  Held to torch's
float64 ``F.interpolate`` and to the library's host entry points by tests/test_ratio_host.py; the yardstick of tests/test_ratio_gpu.py."""
from math import gcd

import numpy as np

A = -0.75
MAX_LST_SIDE = 16384


# ---- the resampler ------------------------------------------------------------------------------------------------------------------
def phases(n, N):
    """output d of an axis n -> N reads source coordinate ((2d + 1) n - N) / (2N): -> (floor, remainder, 2N), all integers"""
    d = np.arange(N, dtype=np.int64)
    num, den = (2 * d + 1) * n - N, 2 * N
    i = np.floor_divide(num, den)
    return i, num - i * den, den


def cubic_weights(t):
    """the four weights of taps i - 1 .. i + 2 at fraction t (ATen upsample_bicubic2d / OpenCV INTER_CUBIC, A = -0.75)"""
    near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], axis=-1)


def axis_matrix(n, N):
    """(N, n) float64: the resampling operator of one axis, indices clamped to the raster"""
    assert 1 <= n <= N
    i, r, den = phases(n, N)
    w = cubic_weights(r.astype(np.float64) / den)
    M = np.zeros((N, n))
    for j in range(4):
        np.add.at(M, (np.arange(N), np.clip(i - 1 + j, 0, n - 1)), w[:, j])
    return M


def upsample_ref(x, size):
    """x (..., h, w) -> (..., H, W) float64"""
    x = np.asarray(x, dtype=np.float64)
    H, W = size
    return axis_matrix(x.shape[-2], H) @ x @ axis_matrix(x.shape[-1], W).T


# ---- the geometry -------------------------------------------------------------------------------------------------------------------
def origins(n, win, overlap, cover):
    """the layout of csrc/mosaic.h along one axis (tests/test_mosaic_gpu.origins)"""
    o = list(range(0, n - win + 1, win - overlap))
    if cover and o[-1] + win < n:
        o.append(n - win)
    return o


def geometry_ref(lst_shape, win, hr, overlap=0, cover=0):
    """-> (p, q, (Ty, Tx), (H, W)), or None where include/sifsr_ratio.h says 1001"""
    h, w = lst_shape
    if not (1 <= win <= 64) or hr % 8 or not (24 <= hr <= 256) or not (win < hr <= 16 * win):
        return None
    d = gcd(hr, win)
    p, q = hr // d, win // d
    for n in (h, w):
        if n < win or n > MAX_LST_SIDE or n % q:
            return None
    if overlap < 0 or 2 * overlap > win or overlap % q:
        return None
    return p, q, (len(origins(h, win, overlap, cover)), len(origins(w, win, overlap, cover))), (h * p // q, w * p // q)


# ---- prepare --------------------------------------------------------------------------------------------------------------------
def prepare_ref(lst, ndvi, stats, win, hr, overlap=0, cover=0, clip_ndvi=True):
    """lst (h, w), ndvi (H, W) -> x (T, 2, hr, hr) float64: per tile the z-score of the block, the resampler clamped at the tile,
    NDVI clip + z-score"""
    lst, ndvi = np.asarray(lst, dtype=np.float64), np.asarray(ndvi, dtype=np.float64)
    p, q, _, hr_shape = geometry_ref(lst.shape, win, hr, overlap, cover)
    assert ndvi.shape == hr_shape
    out = []
    for oy in origins(lst.shape[0], win, overlap, cover):
        for ox in origins(lst.shape[1], win, overlap, cover):
            z = (lst[oy:oy + win, ox:ox + win] - stats["mean_lst"]) / stats["std_lst"]
            nv = ndvi[oy * p // q:oy * p // q + hr, ox * p // q:ox * p // q + hr]
            if clip_ndvi:
                nv = np.clip(nv, -1.0, 1.0)
            out.append(np.stack([upsample_ref(z, (hr, hr)), (nv - stats["mean_ndvi"]) / stats["std_ndvi"]]))
    return np.stack(out)


# ---- blend ----------------------------------------------------------------------------------------------------------------------
def cell_of(n_hr, p, q):
    """the LST cell of every HR pixel along one axis: floor(Y q / p)"""
    return np.arange(n_hr, dtype=np.int64) * q // p


def upsampled(valid, p, q):
    """valid (h, w) -> bool (H, W): is the LST cell of the output pixel valid"""
    valid = np.asarray(valid) != 0
    h, w = valid.shape
    return valid[np.ix_(cell_of(h * p // q, p, q), cell_of(w * p // q, p, q))]


def blend_ref(sr, lst_shape, win, hr, overlap, cover, mean, std, slot=None, valid=None, fill_value=np.nan):
    """sr (T or n_active, 1, hr, hr) -> (out (H, W) float64, covered bool (H, W)).  Weight t(q) of include/sifsr_mosaic.h with
    W = hr and R = overlap p / q; with `slot` tile k is read at sr[slot[k]] and skipped when slot[k] < 0; with `valid` the pixels
    of invalid cells hold fill_value.  covered: some tile of the layout lies over the pixel (whatever `slot` says)."""
    p, q, (ty, tx), (H, W) = geometry_ref(lst_shape, win, hr, overlap, cover)
    R = overlap * p // q
    assert R * q == overlap * p
    c = np.arange(hr, dtype=np.float64)
    t = np.ones(hr) if R == 0 else np.minimum(1.0, np.minimum((c + 0.5) / R, (hr - c - 0.5) / R))
    wgt = t[:, None] * t[None, :]
    oy, ox = origins(lst_shape[0], win, overlap, cover), origins(lst_shape[1], win, overlap, cover)
    sr = np.asarray(sr, dtype=np.float64)
    num, den, covered = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), dtype=bool)
    for a, y0 in enumerate(oy):
        for b, x0 in enumerate(ox):
            Y0, X0 = y0 * p // q, x0 * p // q
            assert Y0 * q == y0 * p and X0 * q == x0 * p
            covered[Y0:Y0 + hr, X0:X0 + hr] = True
            k = a * len(ox) + b
            if slot is not None:
                k = int(slot[k])
                if k < 0:
                    continue
            num[Y0:Y0 + hr, X0:X0 + hr] += wgt * sr[k, 0]
            den[Y0:Y0 + hr, X0:X0 + hr] += wgt
    out = np.zeros((H, W))
    m = den > 0
    out[m] = num[m] / den[m] * std + mean
    if valid is not None:
        out[~upsampled(valid, p, q)] = fill_value
    return out, covered
