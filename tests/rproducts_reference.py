"""NumPy restatement of patch mining at a ratio (sifsr/rproducts.py), step by step as include/sifsr_rproducts.h
states it -- decode, census, select, gather with the window side `ws` and the fine window side `hr` as arguments -- and of the two
mask helpers, `patch_counts` and `expand_valid`; plus `make_case`, the seeded raw inputs of the tests.

What does not depend on `hr` IS tests/products_reference.py: the generator's window order (`windows`), the acceptance rule
(`select`, `max_bad`), the float32 algebra (`decode`) and the moments of a patch.  The census and the gather are restated here with
the fine window of LST window (row0, col0) at rows [row0 p / q, row0 p / q + hr), columns likewise.  The reference knows x4 only:
tests/test_rproducts_host.py holds this file, at hr = 4 ws, to tests/products_reference.py (which is pinned to the reference's
recorded results) on every one of its cases; that comparison is the anchor.  The GPU tests compare the kernels with this file bit
for bit."""
from math import gcd

import numpy as np

from tests.products_reference import F32, decode, max_bad, moments_of, select, statistics, windows  # noqa: F401

COVERAGES = (0.0, 0.05)
# (seed, h, w, ws, hr): the LST raster and the pair.  12 full windows of 20 steps, ragged on both axes, fine pitch 84 int16 (the 8-byte
# path); 2 full windows, fine pitch 45 (odd: the 2-byte path); x10/3 with q = 3, pitch 80 (the 16-byte path); non-square the other way
# round, pitch 76 (8-byte); x4; the production tile, one window
CASES = ((21, 40, 28, 8, 24), (22, 34, 18, 16, 40), (23, 36, 24, 12, 40), (24, 26, 38, 12, 24), (25, 40, 32, 8, 32), (26, 64, 64, 64, 192))
PLANTED = ("clean", "bad_max", "bad_over", "zero_den", "both", "qc_only")


def ratio_of(ws, hr):
    g = gcd(ws, hr)
    return hr // g, ws // g


def fine_shape(h, w, ws, hr):
    p, q = ratio_of(ws, hr)
    assert h % q == 0 and w % q == 0, (h, w, q)
    return h * p // q, w * p // q


def fine_origin(row0, col0, ws, hr):
    p, q = ratio_of(ws, hr)
    assert (row0 * p) % q == 0 and (col0 * p) % q == 0
    return row0 * p // q, col0 * p // q


# ---- the steps --------------------------------------------------------------------------------------------------------------
def census(lst_raw, qc, nir, red, ws, hr, qc_mode=0):
    """counts (nwin, 2) int32: bad LST pixels, zero denominators of the hr x hr fine window; [-1, -1] for a window that is not full"""
    h, w = lst_raw.shape
    assert nir.shape == red.shape == fine_shape(h, w, ws, hr)
    den = F32(0.0001) * nir.astype(F32) + F32(0.0001) * red.astype(F32)
    out = []
    for k, row0, col0, full in windows(h, w, ws):
        if not full:
            out.append((-1, -1))
            continue
        bad = lst_raw[row0:row0 + ws, col0:col0 + ws] == 0
        if qc_mode == 1:
            bad = bad | ((qc[row0:row0 + ws, col0:col0 + ws] & 1) == 1)
        fr, fc = fine_origin(row0, col0, ws, hr)
        out.append((int(bad.sum()), int((den[fr:fr + hr, fc:fc + hr] == 0).sum())))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def gather(lst_raw, nir, red, index, ws, hr):
    """-> lst (n,1,ws,ws), ndvi (n,1,hr,hr) float32 clipped, moments (n,8) float64"""
    lst_k, ndvi = decode(lst_raw, nir, red, clip=True)
    n = len(index)
    lst, nd, mom = np.zeros((n, 1, ws, ws), F32), np.zeros((n, 1, hr, hr), F32), np.zeros((n, 8))
    for i, (_, row0, col0) in enumerate(index):
        fr, fc = fine_origin(int(row0), int(col0), ws, hr)
        lst[i, 0] = lst_k[row0:row0 + ws, col0:col0 + ws]
        nd[i, 0] = ndvi[fr:fr + hr, fc:fc + hr]
        with np.errstate(all="ignore"):
            mom[i] = moments_of(lst[i, 0], nd[i, 0])
    return lst, nd, mom


def mine(case, coverage=0.0, qc_mode=0):
    """all steps on a case of `make_case`: -> counts, index, lst, ndvi, moments"""
    ws, hr = case["ws"], case["hr"]
    counts = census(case["lst_raw"], case["qc"], case["nir"], case["red"], ws, hr, qc_mode)
    index = select(counts, *case["lst_raw"].shape, ws, coverage)
    return (counts, index) + gather(case["lst_raw"], case["nir"], case["red"], index, ws, hr)


def patch_counts(valid, hr):
    """valid (N, ws, ws) -> (N, 2) int64 {n1, n2}: cell i of an axis holds ceil((i + 1) hr / ws) - ceil(i hr / ws) HR pixels"""
    valid = np.asarray(valid) != 0
    ws = valid.shape[-1]
    per = np.array([-(-(i + 1) * hr // ws) + (-i * hr // ws) for i in range(ws)], dtype=np.int64)
    assert per.sum() == hr
    area = per[:, None] * per[None, :]
    return np.stack([valid.reshape(len(valid), -1).sum(1), (valid * area).reshape(len(valid), -1).sum(1)], 1).astype(np.int64)


def expand_valid(valid, size):
    """valid (B, h, w) -> (B, H, W) uint8: out[Y, X] = valid[Y h // H, X w // W] != 0"""
    valid = np.asarray(valid)
    (h, w), (H, W) = valid.shape[-2:], size
    ys, xs = np.arange(H) * h // H, np.arange(W) * w // W
    return (valid[:, ys][:, :, xs] != 0).astype(np.uint8)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
_CASES = {}


def make_case(seed, h, w, ws, hr):
    """Seeded raw inputs {lst_raw uint16 (h,w), qc uint8 (h,w), nir, red int16 (h p/q, w p/q)} plus `planted`: {condition: k}.

    Outside the planted spots LST is 13000..16499, NIR 1..5999 and Red 1..2999 (no accidental zero denominator, every unplanted
    NDVI inside (-1, 1)); QC has bit 0 clear.  With M = max_bad(0.05, ws), planted on the full windows in the order of k, as far as
    the raster has them:

      1st  clean, with NDVI 1.5 and -1.5 before clipping                                   accepted everywhere
      2nd  exactly M LST zeros                                                             rejected at 0, accepted at 0.05
      3rd  exactly M + 1 LST zeros                                                         rejected at 0 and at 0.05
      4th  one nir == -red != 0 pixel and one nir == red == 0 pixel, LST clean             rejected for the zero denominator only
      5th  2 LST zeros and 3 pixels nir == red == 0                                        rejected for both
      6th  2 pixels with QC bit 0 set, LST clean                                           accepted in qc_mode 0, rejected in qc_mode 1 at 0
      7th and later: clean

    The planted fine pixels lie in the last row and the last column of the fine window too, so a window that is read one pixel
    short or one pixel off misses them.  The assertions at the end keep a test from passing vacuously.  Cached and read-only."""
    key = (seed, h, w, ws, hr)
    if key in _CASES:
        return _CASES[key]
    rs = np.random.RandomState(seed)
    fh, fw = fine_shape(h, w, ws, hr)
    lst_raw = rs.randint(13000, 16500, (h, w)).astype(np.uint16)
    qc = (rs.randint(0, 128, (h, w)) * 2).astype(np.uint8)
    nir = rs.randint(1, 6000, (fh, fw)).astype(np.int16)
    red = rs.randint(1, 3000, (fh, fw)).astype(np.int16)
    full = [(k, r, c) for k, r, c, f in windows(h, w, ws) if f]
    M = max_bad(COVERAGES[1], ws)
    assert M >= 1
    planted = {}

    def lst_zeros(r, c, n):
        cells = rs.permutation(ws * ws)[:n]
        lst_raw[r + cells // ws, c + cells % ws] = 0

    for pos, (k, r, c) in enumerate(full[:6]):
        fr, fc = fine_origin(r, c, ws, hr)
        if pos == 0:
            nir[fr + 3, fc + 5], red[fr + 3, fc + 5] = 500, -100
            nir[fr + hr - 1, fc + hr - 1], red[fr + hr - 1, fc + hr - 1] = -100, 500
        elif pos == 1:
            lst_zeros(r, c, M)
        elif pos == 2:
            lst_zeros(r, c, M + 1)
        elif pos == 3:
            nir[fr + hr - 1, fc + hr - 2], red[fr + hr - 1, fc + hr - 2] = 1234, -1234
            nir[fr + 7, fc + hr - 1], red[fr + 7, fc + hr - 1] = 0, 0
        elif pos == 4:
            lst_zeros(r, c, 2)
            for y, x in ((0, 0), (hr - 1, 0), (int(rs.randint(1, hr - 1)), int(rs.randint(1, hr)))):
                nir[fr + y, fc + x], red[fr + y, fc + x] = 0, 0
        elif pos == 5:
            cells = rs.permutation(ws * ws)[:2]
            qc[r + cells // ws, c + cells % ws] |= 1
        planted[PLANTED[pos]] = k
    case = {"seed": seed, "h": h, "w": w, "ws": ws, "hr": hr, "lst_raw": lst_raw, "qc": qc, "nir": nir, "red": red, "planted": planted,
            "full": full, "max_bad": M}
    for a in (lst_raw, qc, nir, red):
        a.setflags(write=False)

    # ---- what the case must hold ----
    row = {k: i for i, (k, _, _, _) in enumerate(windows(h, w, ws))}
    c0, c1 = census(lst_raw, qc, nir, red, ws, hr, 0), census(lst_raw, qc, nir, red, ws, hr, 1)
    acc = {(cov, m): set(select(c, h, w, ws, cov)[:, 0].tolist()) for cov in COVERAGES for m, c in ((0, c0), (1, c1))}
    at = lambda c, name: tuple(int(v) for v in c[row[planted[name]]])
    assert len(full) >= 1 and all(planted["clean"] in a for a in acc.values()) and at(c0, "clean") == (0, 0)
    _, nd = decode(lst_raw, nir, red)
    fr, fc = fine_origin(full[0][1], full[0][2], ws, hr)
    patch = nd[fr:fr + hr, fc:fc + hr]
    assert patch.max() > 1.4 and patch.min() < -1.4 and np.isfinite(patch).all()                  # outside [-1, 1] before clipping
    if len(full) >= 2:
        k = planted["bad_max"]
        assert at(c0, "bad_max") == (M, 0) and k not in acc[(0.0, 0)] and k in acc[(0.05, 0)]
    if len(full) >= 3:
        k = planted["bad_over"]
        assert at(c0, "bad_over") == (M + 1, 0) and k not in acc[(0.0, 0)] and k not in acc[(0.05, 0)]
    if len(full) >= 4:
        assert at(c0, "zero_den") == (0, 2) and planted["zero_den"] not in acc[(0.05, 0)]
        assert np.isnan(nd).sum() >= 1 and np.isinf(nd).sum() >= 1                                # 0 / 0 and x / 0 both occur
    if len(full) >= 5:
        assert at(c0, "both") == (2, 3) and planted["both"] not in acc[(0.05, 0)]
    if len(full) >= 6:
        k = planted["qc_only"]
        assert at(c0, "qc_only") == (0, 0) and at(c1, "qc_only") == (2, 0)
        assert k in acc[(0.0, 0)] and k not in acc[(0.0, 1)] and k in acc[(0.05, 1)]
    if len(full) >= 9:
        assert len(acc[(0.0, 0)]) >= 3
    _CASES[key] = case
    return case
