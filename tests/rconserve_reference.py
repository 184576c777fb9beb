"""Float64 NumPy restatement of include/sifsr_rconserve.h -- D, U, the cell rule, the validity rule, one
correction step and the statistics at any ratio -- and the seeded rasters tests/test_rconserve_host.py and
tests/test_rconserve_gpu.py share.

D is tests/degrade_reference.axis_operator(..., crop=True), which tests/test_degrade_host.py holds to the reference's recorded
outputs; validity comes from its `ring` and the non-zero pattern of its rows; U is the float64 operator of
tests/ratio_reference.py, which tests/test_ratio_host.py holds to torch's float64 F.interpolate.  The residual is rounded to fp32
before U and sr after every step, as the device rounds them, so the trajectory is the device's."""
import functools
import math

import numpy as np

from tests import degrade_reference as DR
from tests import ratio_reference as RR
from tests.conserve_reference import stats_row  # noqa: F401  (the statistics are f12's)

MAX_FACTOR = 8.0
# the tile of csrc/rconserve.hip: at most CAP staged rows / columns, at most TL cells per side
CAP, TL = 80, 16


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def hr_shape(lst_shape, p, q):
    h, w = lst_shape
    assert h % q == 0 and w % q == 0
    return h * p // q, w * p // q


def accepted(lst_shape, sr_shape):
    """what include/sifsr_rconserve.h accepts (n_iter and mtf aside)"""
    (h, w), (H, W) = lst_shape, sr_shape
    if min(h, w, H, W) < 1 or max(h, w, H, W) > 16384 or H * w != W * h:
        return False
    f = float(H) / float(h)
    if not (1.0 < f <= MAX_FACTOR):
        return False
    hw = DR.half_width(f)
    return H >= hw + 1 and W >= hw + 1 and (DR.out_side(H, f, None, True), DR.out_side(W, f, None, True)) == (h, w)


def cells(n, N):
    """the cell of every HR pixel of an axis: floor(Y n / N)"""
    return np.arange(N, dtype=np.int64) * n // N


@functools.lru_cache(maxsize=None)
def axis(n, N, mtf=0.1):
    """-> dict of one axis n <- N: R (n, N) float64, ring (n,) bool, lo / hi (n,) the first and last pixel with a weight, touch (n, n)
    bool: the cells output i must find valid -- its own and those of pixels lo .. hi"""
    f = float(N) / float(n)
    op = DR.axis_operator(N, f, mtf, None, True)
    R = op["R"]
    assert R.shape == (n, N)
    nz = R != 0
    lo, hi = nz.argmax(axis=1), N - 1 - nz[:, ::-1].argmax(axis=1)
    touch = np.eye(n, dtype=bool)
    for i in range(n):
        touch[i, lo[i] * n // N:hi[i] * n // N + 1] = True
    return dict(R=R, ring=op["ring"], lo=lo, hi=hi, touch=touch, own_in_stencil=np.array([lo[i] * n // N <= i <= hi[i] * n // N for i in range(n)]))


def tile_side(factor):
    hw = DR.half_width(factor)
    return max(1, min(TL, int(math.floor((CAP - (2 * hw + 4) - 2 * hw) / factor)) + 1))


def staged_span(n, N, mtf=0.1):
    """the most pixels of this axis a workgroup stages: whole cells, from the first one a stencil of the tile touches to the last"""
    a, tl = axis(n, N, mtf), tile_side(float(N) / float(n))
    most = 0
    for i0 in range(0, n, tl):
        i1 = min(i0 + tl, n) - 1
        c0, c1 = min(i0, a["lo"][i0:i1 + 1].min() * n // N), max(i1, a["hi"][i0:i1 + 1].max() * n // N)
        most = max(most, -(-(c1 + 1) * N // n) - -(-c0 * N // n))
    return most


# ---- D, U ----------------------------------------------------------------------------------------------------------------------------
def D(x, lst_shape, mtf=0.1):
    x = np.asarray(x, np.float64)
    return axis(lst_shape[0], x.shape[0], mtf)["R"] @ x @ axis(lst_shape[1], x.shape[1], mtf)["R"].T


def U(r, sr_shape):
    return RR.upsample_ref(np.asarray(r, np.float64), sr_shape)


# ---- validity, residual, step ----------------------------------------------------------------------------------------------------------
def up(c, sr_shape):
    c = np.asarray(c)
    return c[np.ix_(cells(c.shape[0], sr_shape[0]), cells(c.shape[1], sr_shape[1]))]


def cell_valid(sr, lst, mask=None):
    sr, lst = np.asarray(sr), np.asarray(lst)
    (h, w), (H, W) = lst.shape, sr.shape
    c = np.isfinite(lst) & (lst != 0)
    if mask is not None:
        c &= np.asarray(mask) != 0
    nbad = np.zeros((h, w), np.int64)
    np.add.at(nbad, (cells(h, H)[:, None], cells(w, W)[None, :]), (~(np.isfinite(sr) & (sr != 0))).astype(np.int64))
    return c & (nbad == 0)


def counted(c, sr_shape, mtf=0.1):
    ay, ax = axis(c.shape[0], sr_shape[0], mtf), axis(c.shape[1], sr_shape[1], mtf)
    bad = ay["touch"].astype(np.int64) @ (~c).astype(np.int64) @ ax["touch"].astype(np.int64).T
    return (bad == 0) & ~ay["ring"][:, None] & ~ax["ring"][None, :]


def residual(sr, lst, mask=None, mtf=0.1):
    """-> (r float64 (h, w), 0 where not counted; counted; c).  Invalid cells are zeroed before D: a counted cell never reads them."""
    sr = np.asarray(sr)
    c = cell_valid(sr, lst, mask)
    n = counted(c, sr.shape, mtf)
    srz = np.where(up(c, sr.shape), sr.astype(np.float64), 0.0)
    lstz = np.where(c, np.asarray(lst, np.float64), 0.0)
    return np.where(n, lstz - D(srz, c.shape, mtf), 0.0), n, c


def conserve_ref(sr, lst, mask=None, n_iter=1, relax=1.0, mtf=0.1):
    """-> (out float64 (H, W) of fp32 values, stats (n_iter+1, 4), r of the last row, c of the last row, counted of the last row).
    Pixels of cells without c are never assigned: they keep what `sr` held."""
    out = np.array(sr, np.float64)
    rows = []
    for it in range(n_iter + 1):
        r, n, c = residual(out, lst, mask, mtf)
        rows.append(stats_row(r, n))
        if it == n_iter:
            break
        m = up(c, out.shape)
        step = out + np.float64(np.float32(relax)) * U(r.astype(np.float32), out.shape)
        out[m] = step[m].astype(np.float32)
    return out, np.stack(rows), r, c, n


# ---- the rasters -------------------------------------------------------------------------------------------------------------------
RATIOS = [(3, 1), (5, 2), (2, 1), (4, 1), (8, 3)]
# (lst shape, (p, q)) of tests/test_rconserve_gpu.py: the issue's small rasters, the smallest raster accepted at x3, per ratio one
# raster of more than one 16 x 16 tile on both axes with a ragged last tile, and x8, whose tile is 6 x 6 cells
SHAPES = [((12, 16), (3, 1)), ((12, 16), (5, 2)), ((12, 16), (2, 1)), ((12, 16), (4, 1)), ((12, 15), (8, 3)), ((2, 2), (3, 1)),
          ((18, 35), (3, 1)), ((20, 34), (5, 2)), ((17, 33), (2, 1)), ((19, 21), (4, 1)), ((18, 33), (8, 3)), ((8, 14), (8, 1))]
HOLES = ["block", "corner", "sr_nan", "checkerboard", "nothing_valid"]


def make_case(lst_shape, pq, seed, noise=0.8):
    """-> (sr (H,W) fp32, lst (h,w) fp32): tests/conserve_reference.make_case at a ratio -- a smooth field with texture near 300 K as
    the prediction; the observation is D of a field that differs from it by a 0.3 K offset, a smooth 1 K term and 0.2 K of texture,
    plus 0.05 K of sensor noise"""
    H, W = hr_shape(lst_shape, *pq)
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rs.uniform(0, 2 * np.pi, 4)
    field = 300.0 + 6.0 * np.sin(2 * np.pi * y / 53.0 + ph[0]) * np.cos(2 * np.pi * x / 37.0 + ph[1]) + 3.0 * np.cos(2 * np.pi * (x + y) / 19.0 + ph[2])
    sr = (field + noise * rs.standard_normal(field.shape)).astype(np.float32)
    truth = sr.astype(np.float64) + 0.3 + 1.0 * np.sin(2 * np.pi * (y - x) / 29.0 + ph[3]) + 0.2 * rs.standard_normal(field.shape)
    lst = (D(truth, lst_shape) + 0.05 * rs.standard_normal(lst_shape)).astype(np.float32)
    return sr, lst


def hole_case(kind, pq, seed=7, lst_shape=(12, 16)):
    """-> (sr, lst, mask or None) with the planted gap `kind` (HOLES)"""
    if pq == (8, 3):
        lst_shape = (12, 15)
    h, w = lst_shape
    sr, lst = make_case(lst_shape, pq, seed)
    H, W = sr.shape
    mask = None
    if kind == "block":
        mask = np.full((h, w), 200, np.uint8)                        # any non-zero byte keeps
        mask[2:4, 9:12] = 0
    elif kind == "corner":
        lst[0, 0] = 0.0
        lst[h - 1, w - 1] = np.nan
    elif kind == "sr_nan":
        sr[-(-5 * H // h), -(-4 * W // w) + 1] = np.nan              # one pixel of cell (5, 4)
    elif kind == "checkerboard":
        lst[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 1] = 0.0
    elif kind == "nothing_valid":
        lst[:] = 0.0
    else:
        raise KeyError(kind)
    return sr, lst, mask


def poisoned(sr, lst, mask, junk, seed=3):
    """tests/conserve_reference.poisoned at a ratio: the same case with other contents in every pixel of a cell without c"""
    rs = np.random.RandomState(seed)
    c = cell_valid(sr, lst, mask)
    lst_ok = np.isfinite(lst) & (lst != 0)
    sr2, lst2 = sr.copy(), lst.copy()
    inv = ~c
    lst2[inv & ~lst_ok] = np.float32(junk) if (not np.isfinite(junk) or junk == 0) else np.float32(0.0)
    if mask is not None:
        lst2[np.asarray(mask) == 0] = np.float32(junk)
    only_sr = inv & lst_ok & (np.ones_like(c) if mask is None else np.asarray(mask) != 0)
    lst2[only_sr] = (lst[only_sr] + rs.uniform(1.0, 5.0, int(only_sr.sum()))).astype(np.float32)
    fill = np.full(sr.shape, np.float32(junk))
    keep_bad = up(only_sr, sr.shape) & ~(np.isfinite(sr) & (sr != 0))
    if np.isfinite(junk) and junk != 0:
        fill[keep_bad] = sr[keep_bad]
    m = up(inv, sr.shape)
    sr2[m] = fill[m]
    assert np.array_equal(cell_valid(sr2, lst2, mask), c)
    return sr2, lst2
