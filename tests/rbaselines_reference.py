"""NumPy float64 restatement of the sharpening baselines at any ratio, the yardstick of
tests/test_rbaselines_gpu.py.  Test-side only: the product never imports it.

  * TsHARP, ATPRK, AATPRK: tests/baselines_reference.py with the scale as an argument -- the reference's utils.py:876-1606 takes
    `iscale` throughout.  What reads coarse rasters alone (the regressions, the residual, the empirical semivariogram, the distance
    classes) is imported from there unchanged.  Pinned to the reference's own outputs at scales 2 and 3
    (tests/golden/golden_rbaselines_v1.npz) and to tests/baselines_reference.py at scale 4 by tests/test_rbaselines_host.py.
  * DMS: tests/dms_reference.py with the cell rule in stage 1 and the float64 bicubic of tests/ratio_reference.py in stage 5; the
    stages on coarse cells (training set, tree fit, prediction) are imported from there unchanged.

The cell of fine pixel (Y, X) of an (H, W) raster over an (h, w) raster is (floor(Y h / H), floor(X w / W)); TsHARP and DMS take any
ratio, the kriging methods integer scales only.  Scales 5..8 and the rational ratios have no counterpart in the reference: there
this file is the only yardstick."""
import numpy as np

from tests import baselines_reference as B4
from tests import dms_reference as D4
from tests import ratio_reference as RR

KS, _RC, _CLASS = B4.KS, B4._RC, B4._CLASS
linear_fit, linear_fit_window, residual, semivariogram = B4.linear_fit, B4.linear_fit_window, B4.residual, B4.semivariogram


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def cells(n, N):
    """the coarse cell of every fine index of an axis n -> N: floor(Y n / N), in integers"""
    return np.arange(N, dtype=np.int64) * n // N


def expand(a, fine_shape):
    """a (h, w) -> (H, W): every fine pixel takes the value of its cell"""
    return a[np.ix_(cells(a.shape[0], fine_shape[0]), cells(a.shape[1], fine_shape[1]))]


def scale_of(coarse_shape, fine_shape):
    s = fine_shape[0] // coarse_shape[0]
    assert (s * coarse_shape[0], s * coarse_shape[1]) == tuple(fine_shape) and s >= 2, "kriging: integer scales only"
    return s


# ---- kriging geometry at scale s ------------------------------------------------------------------------------------------------
def fine_distances(scc, s):
    """dis_f of utils.py:1070-1100 at scale s: (25, 25, s^2, s^2), [i, j, a, b] = distance between fine pixel a of block pixel i and
    fine pixel b of block pixel j, on the 5s x 5s fine grid of spacing scc / s."""
    fr = (s * _RC[:, None, 0] + np.arange(s * s)[None, :] // s).astype(np.float64)
    fc = (s * _RC[:, None, 1] + np.arange(s * s)[None, :] % s).astype(np.float64)
    dr = fr[:, None, :, None] - fr[None, :, None, :]
    dc = fc[:, None, :, None] - fc[None, :, None, :]
    return scc / s * np.sqrt(dr ** 2 + dc ** 2)


def gamma_cc(sill, ran, scc, s):
    return (sill * (1 - np.exp(-fine_distances(scc, s) / (ran / 3)))).sum((-1, -2)) / s ** 4


def regularised_model(sill, ran, scc, s):
    """Gamma_ff of utils.py:944-975 at the 15 distance classes, the reference's running division included"""
    G = gamma_cc(sill, ran, scc, s)
    m = np.zeros(15)
    for k in range(15):
        n = 0
        for i in range(25):
            sel = _CLASS[i] == k
            n += int(sel.sum())
            m[k] = (m[k] + G[i, sel].sum()) / n
    return m - m[0]


def kriging_weights(sill, ran, scc, s):
    """utils.py:1118-1182 -> lambdas (s^2, 25)"""
    G = gamma_cc(sill, ran, scc, s)
    Gfc = (sill * (1 - np.exp(-fine_distances(scc, s)[12] / (ran / 3)))).sum(-1).T / s ** 2       # (s^2, 25)
    A = np.zeros((26, 26))
    A[:25, :25], A[:25, 25], A[25, :25] = G, 1.0, 1.0
    Bm = np.concatenate([Gfc, np.ones((s * s, 1))], 1)
    return (np.linalg.inv(A) @ Bm.T).T[:, :25]


def _krige(u, delta, lam, s):
    h, w = delta.shape
    corr = np.zeros_like(u)
    blocks = np.lib.stride_tricks.sliding_window_view(delta, (5, 5)).reshape(h - 4, w - 4, 25)
    inner = np.einsum("ak,yxk->yxa", lam, blocks).reshape(h - 4, w - 4, s, s).transpose(0, 2, 1, 3).reshape(s * (h - 4), s * (w - 4))
    corr[2 * s:s * h - 2 * s, 2 * s:s * w - 2 * s] = inner
    corr[u == 0] = 0.0
    return u + corr


# ---- the three methods ----------------------------------------------------------------------------------------------------------
def tsharp(lst, ndvi_c, ndvi_f, min_T=285.0):
    """utils.py:1213-1231 at any ratio"""
    a0, a1 = linear_fit(lst, ndvi_c, min_T)
    u = (a0 + a1 * ndvi_f) * expand((lst != 0).astype(np.float64), ndvi_f.shape)
    d = expand(residual(lst, ndvi_c, a0, a1), ndvi_f.shape)
    return u + np.where(u == 0, 0.0, d)


def atprk(lst, ndvi_c, ndvi_f, variogram, scc=926.0, min_T=285.0, lambdas=None):
    """utils.py:1234-1253 with the fine-scale (sill, range) given.  -> (image, Gamma_coarse)"""
    s = scale_of(lst.shape, ndvi_f.shape)
    a0, a1 = linear_fit(lst, ndvi_c, min_T)
    u = (a0 + a1 * ndvi_f) * expand((lst != 0).astype(np.float64), ndvi_f.shape)
    d = residual(lst, ndvi_c, a0, a1)
    lam = kriging_weights(variogram[0], variogram[1], scc, s) if lambdas is None else lambdas
    return _krige(u, d, lam, s), semivariogram(d)


def aatprk(lst, ndvi_c, ndvi_f, variogram, scc=926.0, min_T=285.0, b_radius=2, lambdas=None):
    """utils.py:1588-1606 with the fine-scale (sill, range) given.  -> (image, Gamma_coarse)"""
    s = scale_of(lst.shape, ndvi_f.shape)
    a0, a1 = linear_fit_window(lst, ndvi_c, min_T, b_radius)
    with np.errstate(invalid="ignore"):
        u = np.where(np.abs(ndvi_f) > 0, expand(a0, ndvi_f.shape) + expand(a1, ndvi_f.shape) * ndvi_f, 0.0)
    d = residual(lst, ndvi_c, a0, a1)
    lam = kriging_weights(variogram[0], variogram[1], scc, s) if lambdas is None else lambdas
    return _krige(u, d, lam, s), semivariogram(d)


# ---- DMS ------------------------------------------------------------------------------------------------------------------------
def aggregate(fine, coarse_shape, pow4=False):
    """(H, W) -> (mean, std) (h, w) float64: the NaN-ignoring mean and population std of the fine pixels of every cell (of fine^4
    when pow4), added in row-major order in float64; an all-NaN cell gives NaN."""
    f = np.asarray(fine, dtype=np.float64)
    if pow4:
        f = (f * f) * (f * f)
    h, w = coarse_shape
    cy, cx = cells(h, f.shape[0]), cells(w, f.shape[1])
    mean, std = np.empty((h, w)), np.empty((h, w))
    with np.errstate(all="ignore"):
        for i in range(h):
            rows = f[cy == i]
            for j in range(w):
                v = rows[:, cx == j].ravel()
                ok = ~np.isnan(v)
                s = n = 0.0
                for k in range(v.size):
                    s = s + (v[k] if ok[k] else 0.0)
                    n = n + (1.0 if ok[k] else 0.0)
                m = np.float64(s) / np.float64(n)
                q = 0.0
                for k in range(v.size):
                    d = v[k] - m if ok[k] else 0.0
                    q = q + d * d
                mean[i, j], std[i, j] = m, np.sqrt(np.float64(q) / np.float64(n))
    return mean, std


def bicubic(a, fine_shape):
    """the float64 bicubic of tests/ratio_reference.py (its integer phases and its weights) in gather form, the columns of a row
    first: a NaN spreads over its 4 x 4 footprint only, where the matrix form of upsample_ref would spread it over rows and columns"""
    def up(v, N):                                                  # along the last axis
        n = v.shape[-1]
        i, r, den = RR.phases(n, N)
        wgt = RR.cubic_weights(r.astype(np.float64) / den)
        out = np.zeros(v.shape[:-1] + (N,))
        for t in range(4):
            out = out + v[..., np.clip(i - 1 + t, 0, n - 1)] * wgt[:, t]
        return out
    return up(up(np.asarray(a, dtype=np.float64), fine_shape[1]).T, fine_shape[0]).T


def correct(lst, sr):
    """res = lst^4 - cell mean of sr^4, resampled to the fine raster with the float64 bicubic of tests/ratio_reference.py,
    out = (res_hr + sr^4)^(1/4) -> float32"""
    sr = np.asarray(sr, dtype=np.float64)
    lst = np.asarray(lst, dtype=np.float64)
    m4, _ = aggregate(sr, lst.shape, pow4=True)
    res = (lst * lst) * (lst * lst) - m4
    with np.errstate(all="ignore"):
        return np.sqrt(np.sqrt(bicubic(res, sr.shape) + (sr * sr) * (sr * sr))).astype(np.float32)


def dms(lst, ndvi_fine, counts, do_correct=True):
    """lst (h,w), ndvi_fine (H,W), counts (E, h*w) -> (out (H,W) float32, info): tests/dms_reference.dms with stages 1 and 5 above"""
    mean, std = aggregate(ndvi_fine, np.shape(lst))
    ts = D4.training_set(lst, mean, std)
    if ts["n_train"] == 0:
        return np.full(np.shape(ndvi_fine), np.nan, dtype=np.float32), dict(ts=ts, trees=[], perm=np.zeros(0, dtype=np.int64))
    perm, x, y, w = D4.sorted_samples(ts, lst)
    trees = D4.fit(x, y, w, D4.cell_counts_to_sorted(counts, perm))
    sr = D4.predict(trees, ndvi_fine)
    out = correct(lst, sr) if do_correct else sr
    return out, dict(ts=ts, trees=trees, perm=perm, x=x, y=y, w=w, sr=sr, mean=mean, std=std)
