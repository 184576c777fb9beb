"""Vectorised NumPy float64 restatement of the reference's classical sharpening baselines (utils.py:854-1606: TsHARP, ATPRK,
AATPRK), the role tests/eval_reference.py has for the evaluation table.  Test-side only: the product never imports it.

It is pinned to the reference by tests/test_baselines_host.py (golden images and Gamma_coarse of tests/golden/golden_baselines_v1.npz
to 1e-9) and then serves as the reference at the shapes the golden does not hold.  The kriging methods take the FINE-scale
(sill, range) of the exponential variogram as input -- the result of the reference's second curve_fit -- so that nothing here
depends on an optimiser.  scale = 4 and block_size = 5 only, like the product.

One thing is restated as the reference has it rather than as its comments say: in Gamma_ff (utils.py:961-970) the division of a
class's running sum by its running count sits INSIDE the loop over the first coarse pixel, so the "class mean" is
m <- (m + S_i) / N_i over i = 0..24 (S_i: the class's sum in row i of Gamma_cc, N_i: its count up to row i).  The fit the
reference runs is a fit of THAT model, and `regularised_model` reproduces it.
"""
import numpy as np

KS = (0, 1, 2, 4, 5, 8, 9, 10, 13, 16, 17, 18, 20, 25, 32)          # squared coarse distances in a 5 x 5 block, ascending
_RC = np.stack(np.divmod(np.arange(25), 5), 1)                       # (25, 2) row, column of block pixel i
_K = ((_RC[:, None, :] - _RC[None, :, :]) ** 2).sum(-1)              # (25, 25) squared distance of block pixels i, j
_CLASS = np.searchsorted(np.array(KS), _K)                           # (25, 25) class index
_PAIRS = np.array([(i, j) for i in range(25) for j in range(i + 1, 25)])


def _linregress(I, T):
    """scipy.stats.linregress's slope and intercept: centred sums (np.cov with bias=1)."""
    mI, mT = I.mean(), T.mean()
    a1 = ((I - mI) * (T - mT)).mean() / ((I - mI) ** 2).mean()
    return mT - a1 * mI, a1


def linear_fit(lst, ndvi_c, min_T):
    """utils.py:854-874 -> (a0 intercept, a1 slope)."""
    T, I = lst.ravel(), ndvi_c.ravel()
    m = (T > min_T) & np.isfinite(I)
    return _linregress(I[m], T[m])


def linear_fit_window(lst, ndvi_c, min_T, b_radius=2):
    """utils.py:1256-1330 -> (a0 (h,w), a1 (h,w))."""
    h, w = lst.shape
    g0, g1 = linear_fit(lst, ndvi_c, min_T)
    a0, a1 = np.full((h, w), g0), np.full((h, w), g1)
    r = b_radius
    for y in range(r, h - r):
        for x in range(r, w - r):
            T, I = lst[y - r:y + r + 1, x - r:x + r + 1].ravel(), ndvi_c[y - r:y + r + 1, x - r:x + r + 1].ravel()
            m = (T > min_T) & np.isfinite(I)
            if m.sum() > 2 / 3 * (2 * r + 1) ** 2:
                a0[y, x], a1[y, x] = _linregress(I[m], T[m])
    return a0, a1


def residual(lst, ndvi_c, a0, a1):
    """utils.py:907-913 / :1366-1372; a0, a1 scalars or (h,w)."""
    m = a0 + a1 * ndvi_c
    m = np.where(lst > 0, m, 0.0)
    return lst - m


def semivariogram(delta):
    """utils.py:1008-1051 -> Gamma_coarse (15,)."""
    win = np.lib.stride_tricks.sliding_window_view(delta, (5, 5)).reshape(delta.shape[0] - 4, delta.shape[1] - 4, 25)
    d2 = (win[..., _PAIRS[:, 0]] - win[..., _PAIRS[:, 1]]) ** 2          # (h-4, w-4, 300)
    cls = _CLASS[_PAIRS[:, 0], _PAIRS[:, 1]]
    out = np.zeros(15)
    for k in range(1, 15):
        g = d2[..., cls == k].sum(-1) / (2 * int((cls == k).sum()))
        nz = g[g != 0]
        out[k] = nz.mean() if nz.size else 0.0
    out[np.isnan(out)] = 0.0
    return out


def fine_distances(scc):
    """dis_f of utils.py:1070-1100: (25, 25, 16, 16), [i, j, a, b] = distance between fine pixel a of block pixel i and fine pixel
    b of block pixel j, on the 20 x 20 fine grid of spacing scc / 4."""
    fr = (4 * _RC[:, None, 0] + np.arange(16)[None, :] // 4).astype(np.float64)      # (25, 16) fine row
    fc = (4 * _RC[:, None, 1] + np.arange(16)[None, :] % 4).astype(np.float64)
    dr = fr[:, None, :, None] - fr[None, :, None, :]
    dc = fc[:, None, :, None] - fc[None, :, None, :]
    return scc / 4 * np.sqrt(dr ** 2 + dc ** 2)


def gamma_cc(sill, ran, scc):
    """(25, 25): the fine-scale exponential variogram averaged over the 16 x 16 fine pairs of every pair of block pixels."""
    return (sill * (1 - np.exp(-fine_distances(scc) / (ran / 3)))).sum((-1, -2)) / 256


def regularised_model(sill, ran, scc):
    """Gamma_ff of utils.py:944-975 at the 15 distance classes, running division included (module docstring)."""
    G = gamma_cc(sill, ran, scc)
    m = np.zeros(15)
    for k in range(15):
        n = 0
        for i in range(25):
            sel = _CLASS[i] == k
            n += int(sel.sum())
            m[k] = (m[k] + G[i, sel].sum()) / n
    return m - m[0]


def kriging_weights(sill, ran, scc):
    """utils.py:1118-1182 -> lambdas (16, 25)."""
    G = gamma_cc(sill, ran, scc)
    Gfc = (sill * (1 - np.exp(-fine_distances(scc)[12] / (ran / 3)))).sum(-1).T / 16         # (16, 25)
    A = np.zeros((26, 26))
    A[:25, :25], A[:25, 25], A[25, :25] = G, 1.0, 1.0
    Bm = np.concatenate([Gfc, np.ones((16, 1))], 1)
    return (np.linalg.inv(A) @ Bm.T).T[:, :25]


def _up4(a):
    return np.repeat(np.repeat(a, 4, 0), 4, 1)


def _krige(u, delta, lam):
    h, w = delta.shape
    corr = np.zeros_like(u)
    blocks = np.lib.stride_tricks.sliding_window_view(delta, (5, 5)).reshape(h - 4, w - 4, 25)
    inner = np.einsum("ak,yxk->yxa", lam, blocks).reshape(h - 4, w - 4, 4, 4).transpose(0, 2, 1, 3).reshape(4 * (h - 4), 4 * (w - 4))
    corr[8:4 * h - 8, 8:4 * w - 8] = inner
    corr[u == 0] = 0.0
    return u + corr


def tsharp(lst, ndvi_c, ndvi_f, min_T=285.0):
    """utils.py:1213-1231."""
    a0, a1 = linear_fit(lst, ndvi_c, min_T)
    u = (a0 + a1 * ndvi_f) * _up4((lst != 0).astype(np.float64))
    d = _up4(residual(lst, ndvi_c, a0, a1))
    return u + np.where(u == 0, 0.0, d)


def atprk(lst, ndvi_c, ndvi_f, variogram, scc=926.0, min_T=285.0, lambdas=None):
    """utils.py:1234-1253 with the fine-scale (sill, range) given.  -> (image, Gamma_coarse)"""
    a0, a1 = linear_fit(lst, ndvi_c, min_T)
    u = (a0 + a1 * ndvi_f) * _up4((lst != 0).astype(np.float64))
    d = residual(lst, ndvi_c, a0, a1)
    lam = kriging_weights(variogram[0], variogram[1], scc) if lambdas is None else lambdas
    return _krige(u, d, lam), semivariogram(d)


def aatprk(lst, ndvi_c, ndvi_f, variogram, scc=926.0, min_T=285.0, b_radius=2, lambdas=None):
    """utils.py:1588-1606 with the fine-scale (sill, range) given.  -> (image, Gamma_coarse)"""
    a0, a1 = linear_fit_window(lst, ndvi_c, min_T, b_radius)
    with np.errstate(invalid="ignore"):
        u = np.where(np.abs(ndvi_f) > 0, _up4(a0) + _up4(a1) * ndvi_f, 0.0)
    d = residual(lst, ndvi_c, a0, a1)
    lam = kriging_weights(variogram[0], variogram[1], scc) if lambdas is None else lambdas
    return _krige(u, d, lam), semivariogram(d)
