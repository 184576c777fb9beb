"""Float64 NumPy restatement of include/sifsr_conserve.h -- D, U, the validity rule, one correction step and the
statistics -- and the seeded rasters tests/test_conserve_host.py, tests/test_conserve_gpu.py and
tests/golden/make_golden_conserve.py share.

D is pinned to the reference's own downscale_LST_SR_to_LR and U to the bicubic restatement of the input pipeline
(oracle.sif_oracle.prepare_tiles) by tests/golden/make_golden_conserve.py; tests/golden/golden_conserve_v1.npz pins this file to
what it computed then.  Everything here is exact arithmetic on the fp32 taps up to float64 rounding (1e-13 K at 300 K)."""
import math

import numpy as np

from oracle import sif_oracle as O

K4 = np.array([-3.0, 19.0, 19.0, -3.0]) / 32.0
A = -0.75


def taps32(mtf=0.1):
    """the nine fp32 taps the library is handed (sif_ops._taps_c), as float64"""
    return O.psf_taps_1d(mtf).astype(np.float32).astype(np.float64)


# ---- D ---------------------------------------------------------------------------------------------------------------------------
def blur(x, t):
    """separable 9-tap correlation with reflect border (index -k -> k, n-1+k -> n-1-k)"""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    p = np.pad(x, 4, mode="reflect")
    g = sum(t[k] * p[:, k:k + W] for k in range(9))
    return sum(t[k] * g[k:k + H, :] for k in range(9))


def D(x, t):
    """(4h, 4w) -> (h, w): blur, then the bicubic /4 taps K4 at rows / columns 4i .. 4i + 3"""
    g = blur(x, t)
    g = sum(K4[a] * g[a::4, :] for a in range(4))
    return sum(K4[b] * g[:, b::4] for b in range(4))


# ---- U ---------------------------------------------------------------------------------------------------------------------------
def _k1(x):
    return ((A + 2) * x - (A + 3)) * x * x + 1


def _k2(x):
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A


def up4_axis(n):
    """-> (idx (4n, 4) int, coef (4n, 4) float64): output X reads the clamped sources idx[X] with coef[X] (half-pixel centres)"""
    X = np.arange(4 * n)
    s = (X + 0.5) / 4 - 0.5
    i = np.floor(s).astype(np.int64)
    t = s - i
    coef = np.stack([_k2(t + 1), _k1(t), _k1(1 - t), _k2(2 - t)], axis=1)
    idx = np.clip(i[:, None] - 1 + np.arange(4)[None, :], 0, n - 1)
    return idx, coef


def U(r):
    """(h, w) -> (4h, 4w): cv2.resize INTER_CUBIC x4 with the indices clamped at the raster edge"""
    r = np.asarray(r, np.float64)
    h, w = r.shape
    iy, cy = up4_axis(h)
    ix, cx = up4_axis(w)
    rows = sum(cy[:, a, None] * r[iy[:, a], :] for a in range(4))
    return sum(cx[None, :, b] * rows[:, ix[:, b]] for b in range(4))


# ---- validity, residual, step, statistics ------------------------------------------------------------------------------------------
def up(c):
    return np.repeat(np.repeat(np.asarray(c), 4, 0), 4, 1)


def cell_valid(sr, lst, mask=None):
    sr, lst = np.asarray(sr), np.asarray(lst)
    h, w = lst.shape
    c = np.isfinite(lst) & (lst != 0)
    if mask is not None:
        c &= np.asarray(mask) != 0
    return c & (np.isfinite(sr) & (sr != 0)).reshape(h, 4, w, 4).all(axis=(1, 3))


def counted(c):
    """c on the whole 3 x 3 neighbourhood clipped to the raster"""
    h, w = c.shape
    p = np.ones((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = c
    out = np.ones((h, w), bool)
    for a in range(3):
        for b in range(3):
            out &= p[a:a + h, b:b + w]
    return out


def residual(sr, lst, mask, t):
    """-> (r float64 (h, w), 0 where not counted; counted; c).  Invalid cells are zeroed before D: a counted cell never reads them."""
    c = cell_valid(sr, lst, mask)
    n = counted(c)
    srz = np.where(up(c), np.asarray(sr, np.float64), 0.0)
    lstz = np.where(c, np.asarray(lst, np.float64), 0.0)
    return np.where(n, lstz - D(srz, t), 0.0), n, c


def stats_row(r, n):
    k = int(n.sum())
    if k == 0:
        return np.array([0.0, np.nan, np.nan, np.nan])
    v = np.asarray(r, np.float64)[n]
    return np.array([float(k), math.fsum(v) / k, math.sqrt(math.fsum(v * v) / k), float(np.abs(v).max())])


def conserve_ref(sr, lst, mask=None, n_iter=1, relax=1.0, mtf=0.1):
    """-> (out float64 (4h, 4w), stats (n_iter+1, 4), r of the last row, c of the last row, counted of the last row).  Pixels of
    cells without c are never assigned: they keep what `sr` held."""
    t = taps32(mtf)
    out = np.array(sr, np.float64)
    rows = []
    for it in range(n_iter + 1):
        r, n, c = residual(out, lst, mask, t)
        rows.append(stats_row(r, n))
        if it == n_iter:
            break
        m = up(c)
        out[m] = out[m] + relax * U(r)[m]
    return out, np.stack(rows), r, c, n


# ---- the rasters -------------------------------------------------------------------------------------------------------------------
# LR shapes of tests/test_conserve_gpu.py: the minimum (both reflect zones in one tile), ragged non-square, exactly one workgroup,
# partial workgroup tiles on both axes with stencils across tile seams
SHAPES = [(3, 3), (5, 7), (9, 8), (8, 8), (33, 41)]
HOLES = ["interior", "corner", "edge", "row", "mask_block", "sr_only", "nothing_valid", "checkerboard"]


def make_case(h, w, seed):
    """-> (sr (4h,4w) fp32, lst (h,w) fp32): a smooth field with texture near 300 K as the prediction; the observation is D of a
    field that differs from it by a 0.3 K offset, a smooth 1 K term and 0.2 K of texture, plus 0.05 K of sensor noise -- residuals
    of some tenths of a kelvin with a bias that is a robust share of them."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:4 * h, 0:4 * w].astype(np.float64)
    ph = rs.uniform(0, 2 * np.pi, 4)
    field = 300.0 + 6.0 * np.sin(2 * np.pi * y / 53.0 + ph[0]) * np.cos(2 * np.pi * x / 37.0 + ph[1]) + 3.0 * np.cos(2 * np.pi * (x + y) / 19.0 + ph[2])
    sr = (field + 0.8 * rs.standard_normal(field.shape)).astype(np.float32)
    truth = sr.astype(np.float64) + 0.3 + 1.0 * np.sin(2 * np.pi * (y - x) / 29.0 + ph[3]) + 0.2 * rs.standard_normal(field.shape)
    lst = (D(truth, taps32()) + 0.05 * rs.standard_normal((h, w))).astype(np.float32)
    return sr, lst


def hole_case(kind, seed=7, h=16, w=16):
    """-> (sr, lst, mask or None) on an LR 16 x 16 raster with the planted gap `kind` (HOLES)"""
    sr, lst = make_case(h, w, seed)
    mask = None
    if kind == "interior":
        lst[7, 9] = 0.0
    elif kind == "corner":
        lst[0, 0] = 0.0
        lst[h - 1, w - 1] = np.nan
    elif kind == "edge":
        lst[0, 6] = 0.0
        lst[9, w - 1] = np.inf
    elif kind == "row":
        lst[5, :] = 0.0
    elif kind == "mask_block":
        mask = np.ones((h, w), np.uint8)
        mask[3:7, 8:13] = 0
        mask[12, 2] = 0
        mask[mask != 0] = 200                                       # any non-zero byte keeps
    elif kind == "sr_only":
        sr[4 * 6 + 1, 4 * 4 + 2] = np.nan                           # one pixel of cell (6, 4)
        sr[4 * 11:4 * 11 + 4, 4 * 12:4 * 12 + 4] = 0.0              # the whole cell (11, 12): an uncovered patch
        sr[3, 4 * 15 + 3] = np.inf                                  # cell (0, 15), on the corner
    elif kind == "nothing_valid":
        lst[:] = 0.0
    elif kind == "checkerboard":
        lst[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 1] = 0.0
    else:
        raise KeyError(kind)
    return sr, lst, mask


def poisoned(sr, lst, mask, junk, seed=3):
    """the same case with other contents in every pixel of a cell without c: lst stays invalid where it made the cell invalid (it
    takes NaN / 0 / inf, or anything at all under mask == 0), the sr pixels of the cell take `junk`, and lst of a cell that is
    invalid through sr alone takes another valid temperature"""
    rs = np.random.RandomState(seed)
    c = cell_valid(sr, lst, mask)
    lst_ok = np.isfinite(lst) & (lst != 0)
    sr2, lst2 = sr.copy(), lst.copy()
    inv = ~c
    bad_lst = inv & ~lst_ok
    lst2[bad_lst] = np.float32(junk) if (not np.isfinite(junk) or junk == 0) else np.float32(0.0)
    if mask is not None:
        m0 = np.asarray(mask) == 0
        lst2[m0] = np.float32(junk)
    only_sr = inv & lst_ok & (np.ones_like(c) if mask is None else np.asarray(mask) != 0)
    lst2[only_sr] = (lst[only_sr] + rs.uniform(1.0, 5.0, int(only_sr.sum()))).astype(np.float32)
    # sr pixels of invalid cells: where the cell is invalid through sr alone at least one pixel must stay non-finite or 0
    fill = np.full(sr.shape, np.float32(junk))
    keep_bad = up(only_sr) & ~(np.isfinite(sr) & (sr != 0))
    if np.isfinite(junk) and junk != 0:
        fill[keep_bad] = sr[keep_bad]
    sr2[up(inv)] = fill[up(inv)]
    assert np.array_equal(cell_valid(sr2, lst2, mask), c)
    return sr2, lst2
