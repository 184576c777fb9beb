"""numpy / scipy restatement of the valid-pixel scores (include/sifsr_scores.h), built from
``tests/eval_reference.py`` (the per-pair table) and the PSNR / SSIM restatement of ``oracle/sif_oracle.py`` (f1).  Test
infrastructure only (CPU).

One rule: a term is counted iff every pixel its stencil reads is valid.  The restatement replaces the invalid pixels by a finite
constant (scipy's ``uniform_filter`` keeps a running sum, which a NaN or an inf would spoil for the rest of the row), computes the
FULL maps exactly as ``eval_reference`` does, and then selects by the eroded masks:

    V    the valid pixels                                               PSNR, RMSE            n0
    E_r  every pixel within r (Chebyshev) lies in the image and is valid   RMSE_grad r = 1, SSIM r = 3, GSSIM r = 4   n1, n3, n4
    S    every pixel within 4 THAT LIES IN THE IMAGE is valid            the strata of g = |a - ftm(a)|             ns

Selection is written as ``np.where(set, map, 0)`` over the array ``eval_reference`` takes its mean of, divided by the size of the
set: adding an exact zero changes no partial sum of numpy's pairwise summation, so with every pixel valid the rows equal
``eval_reference.metrics`` exactly (tests/test_scores_host.py holds that on the golden crops).
"""
import numpy as np
from scipy.ndimage import minimum_filter, uniform_filter, zoom
from scipy.signal import convolve2d

from tests import eval_reference as E

COUNT_NAMES = ("n0", "n1", "n3", "n4", "ns")


# ---- the sets --------------------------------------------------------------------------------------------------------------------
def valid_map(a, b, mask=None):
    """V = isfinite(a) && a != 0 && isfinite(b) && b != 0 && (mask == None || mask != 0)"""
    v = np.isfinite(a) & (a != 0) & np.isfinite(b) & (b != 0)
    return v if mask is None else v & (np.asarray(mask) != 0)


def eroded(v, r):
    """E_r: a pixel outside the image counts as invalid"""
    return minimum_filter(v.astype(np.uint8), size=2 * r + 1, mode="constant", cval=0).astype(bool)


def clipped(v, r=4):
    """S: a pixel outside the image does not count"""
    return minimum_filter(v.astype(np.uint8), size=2 * r + 1, mode="constant", cval=1).astype(bool)


def sets(v):
    return v, eroded(v, 1), eroded(v, 3), eroded(v, 4), clipped(v, 4)


def blob_mask(H, W, seed, invalid=0.30):
    """uint8 (H, W), 1 = valid: a 6 x 6 normal field zoomed (order 3) to H x W, invalid below its `invalid` quantile"""
    f = zoom(np.random.RandomState(seed).standard_normal((6, 6)), (H / 6, W / 6), order=3)
    assert f.shape == (H, W)
    return (f > np.quantile(f, invalid)).astype(np.uint8)


def zscore(a, b):
    """the pair on the network's scale (values of order 1), float32"""
    m, s = np.float32(a.mean()), np.float32(a.std())
    return ((a - m) / s).astype(np.float32), ((b - m) / s).astype(np.float32)


def _filled(x, v):
    """the invalid pixels replaced by one finite constant that depends on the valid pixels only"""
    c = np.float32(x[v].astype(np.float64).mean()) if v.any() else np.float32(0)
    return np.where(v, x, c).astype(np.float32)


def _mean_over(m, sel, n, dtype=None, crop=0):
    """mean of map `m` over `sel` (same shape), in the summation order of m[crop:-crop, crop:-crop].mean(): the zeros are put into
    the whole map and the crop is taken after, so the array summed has the strides of eval_reference's.  NaN for an empty set."""
    if n == 0:
        return np.nan
    z = np.where(sel, m, m.dtype.type(0))
    if crop:
        z = z[crop:-crop, crop:-crop]
    return z.sum(dtype=dtype) / n


# ---- the maps of eval_reference, uncropped ---------------------------------------------------------------------------------------
def ssim_map(a, b, R):
    """eval_reference.ssim before its crop and mean"""
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    cov_norm = 49.0 / 48.0
    ux, uy = uniform_filter(a, size=7), uniform_filter(b, size=7)
    uxx, uyy, uxy = uniform_filter(a * a, size=7), uniform_filter(b * b, size=7), uniform_filter(a * b, size=7)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def gssim_map(im1, im2, data_range):
    """eval_reference.gssim before its crop and mean: (H-2, W-2), entry (i, j) belongs to pixel (i+1, j+1)"""
    im1, im2 = im1.astype(np.float64), im2.astype(np.float64)
    f = [convolve2d(im1, k, mode="valid") for k in E.GSSIM_FILTERS]
    g = [convolve2d(im2, k, mode="valid") for k in E.GSSIM_FILTERS]
    fm, gm = np.sqrt(f[0] ** 2 + f[1] ** 2), np.sqrt(g[0] ** 2 + g[1] ** 2)
    im1, im2 = im1[1:-1, 1:-1], im2[1:-1, 1:-1]
    cov_norm = 49 / 48
    ux, uy = uniform_filter(im1, size=7), uniform_filter(im2, size=7)
    mf, mg = uniform_filter(fm, size=7), uniform_filter(gm, size=7)
    vx = cov_norm * (uniform_filter(fm * fm, size=7) - mf ** 2)
    vy = cov_norm * (uniform_filter(gm * gm, size=7) - mg ** 2)
    vxy = cov_norm * (uniform_filter(fm * gm, size=7) - mf * mg)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    A1, B1, B2 = 2 * ux * uy + C1, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    with np.errstate(invalid="ignore", divide="ignore"):
        L = A1 / B1
        C = (2 * np.sqrt(vx) * np.sqrt(vy) + C2) / B2
        S = (vxy + C2) / (np.sqrt(vx) * np.sqrt(vy) + C2 / 2)
        return L * C * S


def grad_diff_map(a, b):
    """eval_reference.rmse_grad before its mean and root: (H-2, W-2)"""
    gb = [convolve2d(b, k, mode="valid") for k in E.SOBEL4]
    ga = [convolve2d(a, k, mode="valid") for k in E.SOBEL4]
    mb = np.sqrt(np.power(gb[0], 2) + np.power(gb[1], 2) + np.power(gb[2], 2) + np.power(gb[3], 2))
    ma = np.sqrt(np.power(ga[0], 2) + np.power(ga[1], 2) + np.power(ga[2], 2) + np.power(ga[3], 2))
    return np.power(mb - ma, 2)


# ---- the per-pair table ----------------------------------------------------------------------------------------------------------
def metrics(a, b, mask=None, data_range=None):
    """One pair of (H, W) float32 images and an optional (H, W) mask -> (row of E.METRIC_NAMES, extras): extras holds the five
    counts, R, q25, q75, the map g and the set S."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    V, E1, E3, E4, S = sets(valid_map(a, b, mask))
    n0, n1, n3, n4, ns = (int(x.sum()) for x in (V, E1, E3, E4, S))
    a, b = _filled(a, V), _filled(b, V)
    nan = np.float32(np.nan)
    if data_range is not None:
        R = np.float32(data_range)
    else:
        R = np.max([a[V], b[V]]) - np.min([a[V], b[V]]) if n0 else nan          # :373-374 over the valid pixels, np.float32
    g = E.gradient_map(a)
    sqe = np.power(a - b, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = _mean_over((a - b) ** 2, V, n0, np.float64)
        psnr = 10 * np.log10((R ** 2) / mse)
        rmse = np.sqrt(np.float32(_mean_over(sqe, V, n0))) if n0 else nan
        ssim = _mean_over(ssim_map(a, b, R), E3, n3, np.float64, 3)
        gss = _mean_over(gssim_map(a, b, R), E4[1:-1, 1:-1], n4, np.float64, 3)
        rgrad = np.sqrt(_mean_over(grad_diff_map(a, b), E1[1:-1, 1:-1], n1)) if n1 else np.nan
    if ns:
        gs = g[S]
        q25, q75 = np.percentile(gs, 25), np.percentile(gs, 75)
        lo, mid, hi = S & (g < q25), S & (g >= q25) & (g <= q75), S & (g >= q75)
        # :382-404 restricted to S: the zeroed entries stay in the mean, the divisor is ns
        rm = [np.sqrt(np.float32(np.where(sel, sqe, np.float32(0)).flatten().sum() / ns)) for sel in (lo, mid, hi)]
        strata_counts = tuple(int(x.sum()) for x in (lo, mid, hi))
    else:
        q25 = q75 = nan
        rm = [nan] * 3
        strata_counts = (0, 0, 0)
    row = [psnr, ssim, rmse, rm[0], rm[1], rm[2], gss, rgrad]
    return np.array([float(x) for x in row]), {"counts": (n0, n1, n3, n4, ns), "R": R, "q25": q25, "q75": q75, "g": g, "S": S,
                                                "strata_counts": strata_counts}


# ---- the train-time pair (oracle.psnr_skimage / ssim_skimage, restricted) ---------------------------------------------------------
def upsampled(valid, scale):
    """(B, h, w) bytes -> (B, h * scale, w * scale) bool"""
    return np.repeat(np.repeat(np.asarray(valid) != 0, scale, axis=1), scale, axis=2)


def psnr_ssim(predictions, targets, valid, scale):
    """(B,1,H,W) x2 float32, valid (B, H/scale, W/scale) -> (psnr, ssim, (images with a PSNR, images with an SSIM)): the range over
    the valid target pixels of the batch, per image the PSNR over V and the SSIM over E_3, means over the contributing images."""
    p, t = np.asarray(predictions, np.float32)[:, 0], np.asarray(targets, np.float32)[:, 0]
    V = upsampled(valid, scale)
    assert V.shape == t.shape
    if not V.any():
        return np.nan, np.nan, (0, 0)
    R = np.float32(t[V].max() - t[V].min())
    rng = float(R)
    C1, C2 = (np.float32(0.01) * R) ** 2, (np.float32(0.03) * R) ** 2
    cov_norm = np.float32(49.0 / 48.0)
    ps, ss = [], []
    for i in range(t.shape[0]):
        v = V[i]
        n0 = int(v.sum())
        if n0 == 0:
            continue
        im1, im2 = _filled(t[i], v), _filled(p[i], v)
        with np.errstate(divide="ignore"):
            ps.append(10 * np.log10(rng ** 2 / _mean_over((im1 - im2) ** 2, v, n0, np.float64)))
        e3 = eroded(v, 3)
        n3 = int(e3.sum())
        if n3 == 0:
            continue
        ux, uy = uniform_filter(im1, size=7), uniform_filter(im2, size=7)
        uxx, uyy, uxy = uniform_filter(im1 * im1, size=7), uniform_filter(im2 * im2, size=7), uniform_filter(im1 * im2, size=7)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
        B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
        ss.append(_mean_over((A1 * A2) / (B1 * B2), e3, n3, np.float64, 3))
    return (float(np.mean(ps)) if ps else np.nan, float(np.mean(ss)) if ss else np.nan, (len(ps), len(ss)))


# ---- the cases the tests share ----------------------------------------------------------------------------------------------------
BLOB_SHAPES = ((41, 57), (96, 80))
BLOB_SEEDS = (1, 2, 3)


def pair(rs, H, W):
    from tests.test_eval_metrics_gpu import _pair
    return _pair(rs, H, W)


def blob_case(hw):
    """B = 3 Kelvin pairs with the blob masks of seeds 1-3 -> (a (3,H,W), b, mask uint8)"""
    H, W = hw
    rs = np.random.RandomState(H * 1000 + W)
    pairs = [pair(rs, H, W) for _ in BLOB_SEEDS]
    return (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), np.stack([blob_mask(H, W, s) for s in BLOB_SEEDS]))


def edge_case(hw):
    """z-scored B = 4: all invalid / one valid 9 x 9 block in the interior / a valid 9 x 9 block in the top-left corner / a blob
    mask -> (a, b, mask)"""
    H, W = hw
    rs = np.random.RandomState(H + W)
    pairs = [zscore(*pair(rs, H, W)) for _ in range(4)]
    m = np.zeros((4, H, W), np.uint8)
    m[1, 3:12, H // 4:H // 4 + 9] = 1
    m[2, :9, :9] = 1
    m[3] = blob_mask(H, W, 2, 0.1)
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), m


TRAIN_SHAPES = ((40, 24), (64, 64), (100, 36))
TRAIN_MASKS = ("blobs", "image0", "single")


def train_inputs(hw, kelvin, B=2):
    """the target / prediction pair of tests/test_pipeline_gpu.py::test_psnr_ssim at another shape"""
    shape = (B, 1) + tuple(hw)
    rs = np.random.RandomState(hw[0] * 7 + hw[1])
    t = rs.standard_normal(shape).astype(np.float32)
    t = (t + np.roll(t, 1, 2) + np.roll(t, 1, 3) + np.roll(t, (1, 1), (2, 3))) / 2
    p = t + 0.3 * rs.standard_normal(shape).astype(np.float32)
    if kelvin:
        t, p = t * 5.5 + 307, p * 5.5 + 307
    return p.astype(np.float32), t.astype(np.float32)


def train_mask(hw, scale, kind, B=2):
    """(B, H/scale, W/scale) uint8.  blobs: 30 % invalid per image; image0: image 0 invalid, image 1 blobs; single: one valid LR
    cell (4 x 4 pixels at either scale) in image 0, image 1 invalid.  Valid bytes take several non-zero values."""
    h, w = hw[0] // scale, hw[1] // scale
    if kind == "single":
        m = np.zeros((B, h, w), np.uint8)
        k = 4 // scale
        m[0, 2 * k:3 * k, 3 * k:4 * k] = 7
        return m
    m = np.stack([blob_mask(h, w, 10 + i) * (1 + 100 * i) for i in range(B)]).astype(np.uint8)
    if kind == "image0":
        m[0] = 0
    return m
