"""numpy / scipy restatement of the per-pair ASTER evaluation table, model_perf_aster_formatds.py:371-437
with the columns of :507 less LPIPS.  Test infrastructure only (CPU): ``tests/golden/make_golden_eval.py`` asserts that
``gssim`` and ``get_output_ftm`` here equal the reference's own ``us.gssim`` / ``us.get_output_ftm`` on every golden case and
stores what ``metrics`` returns; the GPU tests compare ``sifsr.metrics.aster_metrics`` with those numbers.

PSNR / SSIM come from scikit-image (not installed) and the strata lines live in a script that cannot be imported: they are
restated from the cited lines and the scikit-image 0.22 algorithm, **unpinned vs scikit-image** (as f1 is).

Two details of the reference that a reader would not guess:
  * the strata RMSEs divide by N, not by the stratum size: ``filter((0.0).__ne__, list(err.flatten()))`` runs on np.float32
    elements, for which ``float.__ne__`` returns NotImplemented (truthy), so nothing is filtered and the zeroed entries stay in
    the mean;
  * ``convolve2d`` of a float32 image with the integer Sobel lists promotes to float64, so RMSE_grad's magnitudes are float64.

``get_output_ftm`` follows the gfx950 kernel's arithmetic (separable 9-tap blur, horizontal then vertical, one float32 FMA
per tap, reflect border): the strata compare g with its own quartiles, so a one-ulp difference in g moves pixels across a
stratum border; the golden script checks this form against the reference's 2-D ``conv2d`` to float32 rounding.
"""
import numpy as np
from scipy.ndimage import uniform_filter
from scipy.signal import convolve2d

METRIC_NAMES = ("PSNR", "SSIM", "RMSE", "RMSE (low grad per image)", "RMSE (mean grad per image)",
                "RMSE (high grad per image)", "GSSIM", "RMSE_grad")

# model_perf_aster_formatds.py:414-417 == train_model_B_predef_filters.py:38-42
SOBEL4 = [[[1, 2, 1], [0, 0, 0], [-1, -2, -1]],
          [[1, 0, -1], [2, 0, -2], [1, 0, -1]],
          [[2, 1, 0], [1, 0, -1], [0, -1, -2]],
          [[0, 1, 2], [-1, 0, 1], [-2, -1, 0]]]
# utils.py:1921-1923
GSSIM_FILTERS = [[[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]],
                 [[-1, -2, -1], [0, 0, 0], [1, 2, 1]]]


def psf_taps32(mtf=0.1, factor=4.0):
    """The separable factor of generate_psf_kernel(1, factor, mtf) (utils.py:1615-1639), cast to float32 as the kernels use it."""
    from oracle.sif_oracle import psf_taps_1d
    return psf_taps_1d(mtf, factor).astype(np.float32)


def _fma32(w, x, s):
    # float32 fma(w, x, s): the float32 product is exact in float64; one float64 add, then the float32 rounding
    return (np.float64(w) * x.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def get_output_ftm(a, mtf=0.1, factor=4.0):
    """utils.py:1833-1860 on one (H, W) float32 image, in the gfx950 kernel's order of operations."""
    t = psf_taps32(mtf, factor)
    H, W = a.shape
    p = np.pad(a.astype(np.float32), 4, mode="reflect")
    m = np.zeros((H + 8, W), np.float32)
    for k in range(9):
        m = _fma32(t[k], p[:, k:k + W], m)
    out = np.zeros((H, W), np.float32)
    for k in range(9):
        out = _fma32(t[k], m[k:k + H, :], out)
    return out


def gradient_map(a):
    """:379-380, g = |a - get_output_ftm(a)| in float32."""
    a = np.asarray(a, np.float32)
    return np.abs(a - get_output_ftm(a))


def strata(a, b, g):
    """:382-404 -> (q25, q75, rmse_low, rmse_mean, rmse_high, (n_low, n_mid, n_high)); divisor N (module docstring)."""
    sqe = np.power(a - b, 2)
    q25, q75 = np.percentile(g.flatten(), 25), np.percentile(g.flatten(), 75)
    lo = sqe.copy(); lo[g >= q25] = 0
    mid = sqe.copy(); mid[g < q25] = 0; mid[g > q75] = 0
    hi = sqe.copy(); hi[g < q75] = 0
    rm = [np.sqrt(np.mean(list(e.flatten()))) for e in (lo, mid, hi)]
    counts = (int((g < q25).sum()), int(((g >= q25) & (g <= q75)).sum()), int((g >= q75).sum()))
    return q25, q75, rm[0], rm[1], rm[2], counts


def psnr(a, b, R):
    """skimage.metrics.peak_signal_noise_ratio(a, b, data_range=R) for float32 images (0.22)."""
    mse = np.mean((a - b) ** 2, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 10 * np.log10((R ** 2) / mse)


def ssim(a, b, R):
    """skimage.metrics.structural_similarity(a, b, data_range=R), 0.22 defaults on float32 images."""
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    cov_norm = 49.0 / 48.0
    ux, uy = uniform_filter(a, size=7), uniform_filter(b, size=7)
    uxx, uyy, uxy = uniform_filter(a * a, size=7), uniform_filter(b * b, size=7), uniform_filter(a * b, size=7)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    return S[3:-3, 3:-3].mean(dtype=np.float64)


def gssim(im1, im2, data_range):
    """utils.py:1904-2005 (win_size 7, grad_comp_type ignored), float64."""
    im1, im2 = im1.astype(np.float64), im2.astype(np.float64)
    f = [convolve2d(im1, k, mode="valid") for k in GSSIM_FILTERS]
    g = [convolve2d(im2, k, mode="valid") for k in GSSIM_FILTERS]
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
    L = A1 / B1
    C = (2 * np.sqrt(vx) * np.sqrt(vy) + C2) / B2
    S = (vxy + C2) / (np.sqrt(vx) * np.sqrt(vy) + C2 / 2)
    return (L * C * S)[3:-3, 3:-3].mean(dtype=np.float64)


def rmse_grad(a, b):
    """:414-437: sqrt(mean((|grad b|_4 - |grad a|_4)^2)), convolve2d 'valid' (float64)."""
    gb = [convolve2d(b, k, mode="valid") for k in SOBEL4]
    ga = [convolve2d(a, k, mode="valid") for k in SOBEL4]
    mb = np.sqrt(np.power(gb[0], 2) + np.power(gb[1], 2) + np.power(gb[2], 2) + np.power(gb[3], 2))
    ma = np.sqrt(np.power(ga[0], 2) + np.power(ga[1], 2) + np.power(ga[2], 2) + np.power(ga[3], 2))
    return np.sqrt(np.mean(np.power(mb - ma, 2)))


def metrics(a, b):
    """One pair of (H, W) float32 images (a = ASTER reference, b = prediction) -> (row of METRIC_NAMES, extras)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    R = np.max([a, b]) - np.min([a, b])                     # :373-374, np.float32
    g = gradient_map(a)
    q25, q75, lo, mid, hi, counts = strata(a, b, g)
    row = [psnr(a, b, R), ssim(a, b, R), np.sqrt(np.mean(np.power(a - b, 2))), lo, mid, hi, gssim(a, b, R),
           rmse_grad(a, b)]
    return np.array([float(v) for v in row]), {"q25": q25, "q75": q75, "counts": counts, "R": R}
