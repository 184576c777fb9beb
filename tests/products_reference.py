"""NumPy restatement of the patch mining of sifsr/products.py, step by step as include/sifsr_products.h
states it -- decode, census, select, gather -- and of the statistics; plus `make_case`, the seeded raw inputs of the tests.

Pinned to the reference by tests/test_products_host.py against tests/golden/golden_products_v1.npz (made by
tests/golden/make_golden_products.py, which runs the reference's own us.split / us.split_NIRRed / us.compute_NDVI and
process_MOD21A1D / process_MOD11A1).  The GPU tests compare the kernels with this file bit for bit.

Window order: the reference's generator, literally (utils.py:79-84): `for i in range(0, shape[0], ws): for j in range(0, shape[1],
ws): yield LST[j:j+ws, i:i+ws]` -- the OUTER variable i is the COLUMN offset but runs over shape[0], the inner j is the ROW offset
and runs over shape[1].  On a square raster that is "column blocks outer, row blocks inner, ragged windows counted"; on a
non-square one the exchanged bounds change which windows are visited and what k they get, and this file keeps that."""
import hashlib
import random

import numpy as np

F32 = np.float32
COVERAGES = (0.0, 0.01)
# (seed, h, w): 3 x 2 full windows with ragged edges on both axes; 3 x 4 full windows the other way round (room for every planted
# condition at coverage 0); one window beside an empty one; a single window
CASES = ((11, 200, 136), (12, 200, 264), (13, 128, 64), (14, 64, 64))


# ---- the four steps ---------------------------------------------------------------------------------------------------------
def decode(lst_raw, nir, red, clip=False):
    lst_k = F32(0.02) * lst_raw.astype(F32)
    n, r = F32(0.0001) * nir.astype(F32), F32(0.0001) * red.astype(F32)
    with np.errstate(all="ignore"):
        ndvi = (n - r) / (n + r)
    if clip:
        ndvi[ndvi > 1] = 1
        ndvi[ndvi < -1] = -1
    return lst_k, ndvi


def windows(h, w, ws=64):
    """[(k, row0, col0, full)] in the generator's order, k 1-based"""
    out, k = [], 0
    for col0 in range(0, h, ws):
        for row0 in range(0, w, ws):
            k += 1
            out.append((k, row0, col0, row0 + ws <= h and col0 + ws <= w))
    return out


def census(lst_raw, qc, nir, red, ws=64, qc_mode=0):
    """counts (nwin, 2) int32: bad LST pixels, zero denominators; [-1, -1] for a window that is not full"""
    h, w = lst_raw.shape
    n, r = F32(0.0001) * nir.astype(F32), F32(0.0001) * red.astype(F32)
    den = n + r
    out = []
    for k, row0, col0, full in windows(h, w, ws):
        if not full:
            out.append((-1, -1))
            continue
        bad = lst_raw[row0:row0 + ws, col0:col0 + ws] == 0
        if qc_mode == 1:
            bad = bad | ((qc[row0:row0 + ws, col0:col0 + ws] & 1) == 1)
        out.append((int(bad.sum()), int((den[4 * row0:4 * (row0 + ws), 4 * col0:4 * (col0 + ws)] == 0).sum())))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def max_bad(coverage, ws=64):
    return int(np.floor(coverage * ws ** 2))


def select(counts, h, w, ws=64, coverage=0.0):
    """index (n, 3) int32 [k, row0, col0] of the accepted windows, in the order of k"""
    win = windows(h, w, ws)
    acc = [(k, row0, col0) for (k, row0, col0, full), (bad, zden) in zip(win, counts)
           if full and 0 <= bad <= coverage * ws ** 2 and zden == 0]
    return np.array(acc, dtype=np.int32).reshape(-1, 3)


def moments_of(lst, ndvi):
    """one row of the (n, 8) moments: float64, two passes"""
    a, b = lst.astype(np.float64), ndvi.astype(np.float64)
    return [a.size, a.mean(), ((a - a.mean()) ** 2).sum(), a.min(), a.max(), b.mean(), ((b - b.mean()) ** 2).sum(), 0.0]


def gather(lst_raw, nir, red, index, ws=64):
    """-> lst (n,1,ws,ws), ndvi (n,1,4ws,4ws) float32, moments (n,8) float64"""
    lst_k, ndvi = decode(lst_raw, nir, red, clip=True)
    n = len(index)
    lst, nd, mom = np.zeros((n, 1, ws, ws), F32), np.zeros((n, 1, 4 * ws, 4 * ws), F32), np.zeros((n, 8))
    for i, (_, row0, col0) in enumerate(index):
        lst[i, 0] = lst_k[row0:row0 + ws, col0:col0 + ws]
        nd[i, 0] = ndvi[4 * row0:4 * (row0 + ws), 4 * col0:4 * (col0 + ws)]
        mom[i] = moments_of(lst[i, 0], nd[i, 0])
    return lst, nd, mom


def mine(case, ws=64, coverage=0.0, qc_mode=0):
    """all four steps on a case of `make_case`: -> counts, index, lst, ndvi, moments"""
    counts = census(case["lst_raw"], case["qc"], case["nir"], case["red"], ws, qc_mode)
    index = select(counts, *case["lst_raw"].shape, ws, coverage)
    return (counts, index) + gather(case["lst_raw"], case["nir"], case["red"], index, ws)


# ---- the split and the statistics ----------------------------------------------------------------------------------------------
def assign_split(n, seed=42, proportions=(0.6, 0.4)):
    state = random.getstate()
    try:
        random.seed(seed)
        return np.array([random.choices(["Train", "Val"], list(proportions))[0] for _ in range(n)], dtype=object)
    finally:
        random.setstate(state)


def statistics(lst, ndvi):
    """over ALL the given patches, from the concatenation in float64 (population standard deviations)"""
    a, b = lst.astype(np.float64).ravel(), ndvi.astype(np.float64).ravel()
    return {"maxi": float(lst.max()), "mini": float(lst.min()), "mean_lst": float(a.mean()), "std_lst": float(a.std()),
            "mean_ndvi": float(b.mean()), "std_ndvi": float(b.std())}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
_CASES = {}


def make_case(seed, h, w, ws=64):
    """Seeded raw inputs {lst_raw uint16 (h,w), qc uint8 (h,w), nir, red int16 (4h,4w)} plus `planted`: {condition: k}.

    Outside the planted spots LST is 13000..16499 (260..330 K), NIR 1..5999 and Red 1..2999: both >= 1, so no accidental
    nir + red == 0 (random int16 pairs give 4 in 640 000) and every unplanted NDVI lies inside (-1, 1).  QC has bit 0 clear
    (bits 1..7 random: they must not matter).  Planted, on the full windows in the order of k, as far as the raster has them:

      1st  clean, with NDVI 1.5 and -1.5 before clipping (a negative reflectance)         accepted everywhere
      2nd  exactly 40 LST zeros (coverage 0.01: threshold 40.96)                            rejected at 0 for LST zeros only, accepted at 0.01
      3rd  exactly 41 LST zeros                                                             rejected at 0 and at 0.01
      4th  one nir == -red != 0 pixel and one nir == red == 0 pixel, LST clean              rejected for the zero denominator only
      5th  5 LST zeros and 3 pixels nir == red == 0                                         rejected for both
      6th  3 pixels with QC bit 0 set, LST clean                                            accepted in qc_mode 0, rejected in qc_mode 1 at 0
      7th  one nir == red == 0 pixel, LST clean                                             a second zero-denominator-only window
      8th and later: clean

    The assertions at the end are what keeps a test from passing vacuously.  `>= 3 accepted` is asserted at coverage 0 where the
    raster has at least 9 full windows and at coverage 0.01 (1st, 2nd, 6th) where it has 6; the two small cases have one full
    window each, which is clean and accepted.  The result is cached and read-only."""
    key = (seed, h, w, ws)
    if key in _CASES:
        return _CASES[key]
    rs = np.random.RandomState(seed)
    lst_raw = rs.randint(13000, 16500, (h, w)).astype(np.uint16)
    qc = (rs.randint(0, 128, (h, w)) * 2).astype(np.uint8)
    nir = rs.randint(1, 6000, (4 * h, 4 * w)).astype(np.int16)
    red = rs.randint(1, 3000, (4 * h, 4 * w)).astype(np.int16)
    full = [(k, r, c) for k, r, c, f in windows(h, w, ws) if f]
    planted = {}

    def lst_zeros(r, c, n):
        cells = rs.permutation(ws * ws)[:n]
        lst_raw[r + cells // ws, c + cells % ws] = 0

    def fine(r, c):
        return 4 * r + int(rs.randint(0, 4 * ws)), 4 * c + int(rs.randint(0, 4 * ws))

    for pos, (k, r, c) in enumerate(full):
        if pos == 0:
            (y, x), (y2, x2) = (4 * r + 3, 4 * c + 5), (4 * r + 4 * ws - 1, 4 * c + 4 * ws - 1)
            nir[y, x], red[y, x] = 500, -100
            nir[y2, x2], red[y2, x2] = -100, 500
            planted["clean"] = k
        elif pos == 1:
            lst_zeros(r, c, 40)
            planted["bad40"] = k
        elif pos == 2:
            lst_zeros(r, c, 41)
            planted["bad41"] = k
        elif pos == 3:
            y, x = 4 * r + 17, 4 * c + 4 * ws - 2
            nir[y, x], red[y, x] = 1234, -1234
            nir[y + 1, x], red[y + 1, x] = 0, 0
            planted["zero_den"] = k
        elif pos == 4:
            lst_zeros(r, c, 5)
            for _ in range(3):
                y, x = fine(r, c)
                nir[y, x], red[y, x] = 0, 0
            planted["both"] = k
        elif pos == 5:
            cells = rs.permutation(ws * ws)[:3]
            qc[r + cells // ws, c + cells % ws] |= 1
            planted["qc_only"] = k
        elif pos == 6:
            y, x = fine(r, c)
            nir[y, x], red[y, x] = 0, 0
            planted["zero_den_2"] = k
    case = {"seed": seed, "h": h, "w": w, "lst_raw": lst_raw, "qc": qc, "nir": nir, "red": red, "planted": planted, "full": full}
    for a in (lst_raw, qc, nir, red):
        a.setflags(write=False)

    # ---- what the case must hold ----
    row = {k: i for i, (k, _, _, _) in enumerate(windows(h, w, ws))}
    c0, c1 = census(lst_raw, qc, nir, red, ws, 0), census(lst_raw, qc, nir, red, ws, 1)
    acc = {(cov, m): set(select(c, h, w, ws, cov)[:, 0].tolist()) for cov in COVERAGES for m, c in ((0, c0), (1, c1))}
    assert len(full) >= 1 and planted["clean"] in acc[(0.0, 0)] and planted["clean"] in acc[(0.0, 1)]
    _, nd = decode(lst_raw, nir, red)
    k, r, c = full[0]
    patch = nd[4 * r:4 * (r + ws), 4 * c:4 * (c + ws)]
    assert patch.max() > 1.4 and patch.min() < -1.4 and np.isfinite(patch).all()                  # outside [-1, 1] before clipping
    if len(full) >= 6:
        k40, k41, kz, kb, kq = (planted[n] for n in ("bad40", "bad41", "zero_den", "both", "qc_only"))
        assert tuple(c0[row[k40]]) == (40, 0) and k40 not in acc[(0.0, 0)] and k40 in acc[(0.01, 0)]
        assert tuple(c0[row[k41]]) == (41, 0) and k41 not in acc[(0.0, 0)] and k41 not in acc[(0.01, 0)]
        assert tuple(c0[row[kz]]) == (0, 2) and tuple(c0[row[kb]]) == (5, 3)
        yz = np.argwhere((nir[4 * full[3][1]:, 4 * full[3][2]:] == 1234))
        assert len(yz) >= 1                                                                       # nir == -red != 0 is there
        assert tuple(c0[row[kq]]) == (0, 0) and tuple(c1[row[kq]]) == (3, 0)
        assert kq in acc[(0.0, 0)] and kq not in acc[(0.0, 1)] and kq in acc[(0.01, 1)]
        assert len(acc[(0.01, 0)]) >= 3
        assert np.isnan(nd).sum() >= 1 and np.isinf(nd).sum() >= 1                                # 0 / 0 and x / 0 both occur
    if len(full) >= 9:
        assert tuple(c0[row[planted["zero_den_2"]]]) == (0, 1) and len(acc[(0.0, 0)]) >= 3
    _CASES[key] = case
    return case
