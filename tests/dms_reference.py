"""A NumPy-only float64 restatement of the DMS sharpener (Gao et al. 2012) as the reference's evaluation calls it
(data_mining_sharpener_modified.py through model_perf_aster_formatds.py:220-250): one predictor (NDVI), global regression only,
bagged regression trees (max_leaf_nodes 30, min_samples_leaf 10) with a ridge regression in every leaf, radiance residual
correction.  The five stages are those of include/sifsr_dms.h; the bootstrap multiplicities `counts` are an INPUT.

With one feature every node of a tree is an interval of the samples sorted by the float32 feature, so scikit-learn's best-first
builder (sklearn/tree/_tree.pyx BestFirstTreeBuilder, _splitter.pyx, _criterion.pyx MSE) is prefix sums plus an arg-max per node.
`fit_tree` also reports how close the fit came to a tie: the smallest relative gap between the best and the second-best split
proxy of a node, and between the two largest priorities of the frontier at every pick.
tests/test_dms_host.py pins this file to a live scikit-learn and to outputs of the reference's own tree class."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
FEATURE_THRESHOLD = np.float32(1e-7)
MAX_LEAVES, MIN_LEAF, MIN_TRAIN, RATIO = 30, 10, 10, 0.25
# cv2 INTER_CUBIC x4 (A = -0.75): the coefficients of t = 0.625, 0.875, 0.125, 0.375 for the output phases 0 .. 3 (exact in binary)
UP4 = np.array([[-0.06591796875, 0.42626953125, 0.74951171875, -0.10986328125],
                [-0.01025390625, 0.11474609375, 0.96728515625, -0.07177734375],
                [-0.07177734375, 0.96728515625, 0.11474609375, -0.01025390625],
                [-0.10986328125, 0.74951171875, 0.42626953125, -0.06591796875]])


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------
def aggregate(fine, pow4=False):
    """(4h,4w) -> (mean, std) (h,w) float64: the NaN-ignoring mean and population std of every 4 x 4 block (of fine^4 when pow4),
    the 16 values added row by row in float64; an all-NaN block gives NaN."""
    f = np.asarray(fine, dtype=np.float64)
    H, W = f.shape
    v = f.reshape(H // 4, 4, W // 4, 4).transpose(0, 2, 1, 3).reshape(H // 4, W // 4, 16)
    if pow4:
        v = (v * v) * (v * v)
    ok = ~np.isnan(v)
    s, n = np.zeros(v.shape[:2]), np.zeros(v.shape[:2])
    for k in range(16):
        s = s + np.where(ok[..., k], v[..., k], 0.0)
        n = n + ok[..., k]
    with np.errstate(all="ignore"):
        mean = s / n
        q = np.zeros_like(s)
        for k in range(16):
            d = np.where(ok[..., k], v[..., k] - mean, 0.0)
            q = q + d * d
        std = np.sqrt(q / n)
    return mean, std


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------
def percentile80(sorted_cv):
    """np.percentile(., 80), linear interpolation, on ascending values, as NumPy computes it"""
    n = sorted_cv.size
    v = (80 / 100) * (n - 1)
    lo = int(np.floor(v))
    hi = min(lo + 1, n - 1)
    t = v - lo
    a, b = sorted_cv[lo], sorted_cv[hi]
    return b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t


def training_set(lst, mean, std):
    """-> dict(good (h,w) bool, x (h,w) float64 feature, cv (h,w), w (h,w) weights (0 outside good), thr, n_train).  trainSharpener
    :653-736 with the global window; lst <= 0 is also no-data.  Fewer than MIN_TRAIN good cells: n_train = 0, good all False."""
    lst = np.asarray(lst, dtype=np.float64)
    x = np.where(mean == 0, 1e-6, mean)
    with np.errstate(all="ignore"):
        cv = std / x
    cv = np.where(np.isnan(cv), 1000.0, cv)
    good = np.isfinite(lst) & (lst > 0) & np.isfinite(x) & (cv > 0) & (cv < 1000)
    n = int(good.sum())
    w = np.zeros_like(cv)
    if n < MIN_TRAIN:
        return dict(good=np.zeros_like(good), x=x, cv=cv, w=w, thr=0.0, n_train=0)
    thr = percentile80(np.sort(cv[good]))
    with np.errstate(all="ignore"):
        wi = 1.0 / cv[good]
        wi = (wi - wi.min()) / (wi.max() - wi.min())
    wi = np.where(cv[good] < thr, wi, wi / 2)
    w[good] = wi
    return dict(good=good, x=x, cv=cv, w=w, thr=float(thr), n_train=n)


def sorted_samples(ts, lst):
    """the good cells in ascending order of the float32 feature (stable: ties in row-major order) -> (perm into the flat cells,
    x float64, y float64, w)"""
    idx = np.flatnonzero(ts["good"].ravel())
    x = ts["x"].ravel()[idx]
    o = np.argsort(x.astype(np.float32), kind="stable")
    perm = idx[o]
    return perm, x[o], np.asarray(lst, dtype=np.float64).ravel()[perm], ts["w"].ravel()[perm]


# ---- stage 3 ------------------------------------------------------------------------------------------------------------------
def _gap(best, second):
    return abs(best - second) / abs(best) if best != 0 else (0.0 if second == 0 else np.inf)


def fit_tree(x, y, sw):
    """x (n,) float64 ascending in float32, y (n,), sw (n,) = weight * bootstrap count.  -> dict(thresholds (L-1,) float64,
    bounds (L+1,) positions in the sorted samples, leaves (L,4) = coef, intercept, lo, hi, values (L,) the tree's own leaf means,
    proxy_gap, heap_gap)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    x32 = x.astype(np.float32)
    nz = np.flatnonzero(sw != 0)
    xz, yz, wz = x32[nz], y[nz], np.asarray(sw, dtype=np.float64)[nz]
    m = nz.size
    P0 = np.concatenate([[0.0], np.cumsum(wz)])
    P1 = np.concatenate([[0.0], np.cumsum(wz * yz)])
    P2 = np.concatenate([[0.0], np.cumsum(wz * yz * yz)])
    W = P0[m]
    cand_ok = np.zeros(m + 1, dtype=bool)
    with np.errstate(all="ignore"):
        cand_ok[1:m] = ~(xz[1:] <= (xz[:-1] + FEATURE_THRESHOLD).astype(np.float32))
    gaps = {"proxy": np.inf, "heap": np.inf}

    def evaluate(s, e, imp):
        node = dict(s=s, e=e, imp=imp, leaf=True, prio=0.0)
        if e - s < 2 * MIN_LEAF or imp <= EPS:
            return node
        p = np.arange(s + MIN_LEAF, e - MIN_LEAF + 1)
        p = p[cand_ok[p]]
        if p.size == 0:
            return node
        with np.errstate(all="ignore"):
            sl, wl = P1[p] - P1[s], P0[p] - P0[s]
            sr, wr = P1[e] - P1[p], P0[e] - P0[p]
            proxy = sl * sl / wl + sr * sr / wr
        fin = ~np.isnan(proxy)
        if not fin.any():
            return node
        proxy = np.where(fin, proxy, -np.inf)
        k = int(np.argmax(proxy))                       # first maximum
        if p.size > 1:
            gaps["proxy"] = min(gaps["proxy"], _gap(proxy[k], np.max(np.delete(proxy, k))))
        b = int(p[k])
        wn, wl, wr = P0[e] - P0[s], P0[b] - P0[s], P0[e] - P0[b]
        il = (P2[b] - P2[s]) / wl - ((P1[b] - P1[s]) / wl) ** 2
        ir = (P2[e] - P2[b]) / wr - ((P1[e] - P1[b]) / wr) ** 2
        prio = wn / W * (imp - wr / wn * ir - wl / wn * il)
        if not prio + EPS >= 0:
            return node
        thr = np.float64(xz[b - 1]) / 2.0 + np.float64(xz[b]) / 2.0
        if thr == xz[b] or np.isinf(thr):
            thr = np.float64(xz[b - 1])
        node.update(leaf=False, prio=prio, pos=b, il=il, ir=ir, thr=thr)
        return node

    root_imp = P2[m] / W - (P1[m] / W) ** 2 if m > 0 and W != 0 else 0.0
    frontier, splits = [evaluate(0, m, root_imp)], 0
    while True:
        open_ = [n for n in frontier if not n["leaf"]]
        if not open_ or splits == MAX_LEAVES - 1:
            break
        open_.sort(key=lambda n: -n["prio"])
        if len(open_) > 1:
            gaps["heap"] = min(gaps["heap"], _gap(open_[0]["prio"], open_[1]["prio"]))
        n = open_[0]
        frontier.remove(n)
        splits += 1
        frontier += [evaluate(n["s"], n["pos"], n["il"]), evaluate(n["pos"], n["e"], n["ir"])]
    leaves = sorted(frontier, key=lambda n: n["s"])
    L = len(leaves)
    thresholds = np.empty(L - 1)
    for k in range(1, L):
        b = leaves[k]["s"]
        t = np.float64(xz[b - 1]) / 2.0 + np.float64(xz[b]) / 2.0
        thresholds[k - 1] = np.float64(xz[b - 1]) if (t == xz[b] or np.isinf(t)) else t
    with np.errstate(all="ignore"):
        values = np.array([(P1[n["e"]] - P1[n["s"]]) / (P0[n["e"]] - P0[n["s"]]) for n in leaves])
    # the ridge of every leaf over ALL the samples that predict into it (unweighted; zero-weight and out-of-bag ones included)
    leaf_of = np.searchsorted(thresholds, x32.astype(np.float64), side="left")
    bounds = np.searchsorted(leaf_of, np.arange(L + 1), side="left")
    par = np.zeros((L, 4))
    for k in range(L):
        xs, ys = x[bounds[k]:bounds[k + 1]], y[bounds[k]:bounds[k + 1]]
        xm, ym = xs.sum() / xs.size, ys.sum() / ys.size
        sxx, sxy = ((xs - xm) ** 2).sum(), ((xs - xm) * (ys - ym)).sum()
        coef = sxy / (sxx + 1.0)
        r = ys.max() - ys.min()
        par[k] = coef, ym - coef * xm, ys.min() - RATIO * r, ys.max() + RATIO * r
    return dict(thresholds=thresholds, bounds=bounds, leaves=par, values=values, proxy_gap=gaps["proxy"], heap_gap=gaps["heap"])


def fit(x, y, w, counts):
    """counts (E, n) bootstrap multiplicities of the sorted samples -> list of E trees"""
    return [fit_tree(x, y, w * c) for c in np.asarray(counts)]


# ---- stage 4 ------------------------------------------------------------------------------------------------------------------
def predict_tree(tree, xq):
    """xq float64 (any shape): the leaf by `float32(x) <= threshold -> left`, then the clamped ridge"""
    xq = np.asarray(xq, dtype=np.float64)
    k = np.searchsorted(tree["thresholds"], xq.astype(np.float32).astype(np.float64), side="left")
    c, i, lo, hi = (tree["leaves"][k, j] for j in range(4))
    return np.minimum(np.maximum(xq * c + i, lo), hi)


def predict(trees, ndvi_fine):
    """mean over the estimators in index order; a NaN index is predicted as 0 and stored as NaN; rounded to float32 (the
    reference stores the sharpened image as a float32 raster); no trees: all NaN"""
    f = np.asarray(ndvi_fine, dtype=np.float64)
    if not trees:
        return np.full(f.shape, np.nan, dtype=np.float32)
    nan = np.isnan(f)
    xq = np.where(nan, 0.0, f)
    acc = np.zeros(f.shape)
    for t in trees:
        acc = acc + predict_tree(t, xq)
    out = acc / len(trees)
    out[nan] = np.nan
    return out.astype(np.float32)


# ---- stage 5 ------------------------------------------------------------------------------------------------------------------
def bicubic_up4(a):
    """cv2.resize INTER_CUBIC x4 of a float64 (h,w) array as the pipeline restates it: replicate border, rows first"""
    h, w = a.shape

    def up(v, n):                                              # along the last axis
        j = np.arange(4 * n)
        base = j // 4 - 2 + (j % 4 >= 2)
        out = np.zeros(v.shape[:-1] + (4 * n,))
        for t in range(4):
            out = out + v[..., np.clip(base + t, 0, n - 1)] * UP4[j % 4, t]
        return out
    return up(up(a, w).T, h).T


def correct(lst, sr):
    """residualAnalysis with temperature: res = lst^4 - mean4x4(sr^4), upsampled x4, out = (res_hr + sr^4)^(1/4) -> float32"""
    sr = np.asarray(sr, dtype=np.float64)
    lst = np.asarray(lst, dtype=np.float64)
    m4, _ = aggregate(sr, pow4=True)
    res = (lst * lst) * (lst * lst) - m4
    with np.errstate(all="ignore"):
        return np.sqrt(np.sqrt(bicubic_up4(res) + (sr * sr) * (sr * sr))).astype(np.float32)


# ---- the whole method ---------------------------------------------------------------------------------------------------------
def cell_counts_to_sorted(counts, perm):
    """counts (E, h*w) in row-major cell order -> (E, n_train) in sorted-sample order"""
    return np.asarray(counts)[:, perm]


def dms(lst, ndvi_fine, counts, do_correct=True):
    """lst (h,w), ndvi_fine (4h,4w), counts (E, h*w) -> (out (4h,4w) float32, info)"""
    mean, std = aggregate(ndvi_fine)
    ts = training_set(lst, mean, std)
    if ts["n_train"] == 0:
        return np.full(np.shape(ndvi_fine), np.nan, dtype=np.float32), dict(ts=ts, trees=[], perm=np.zeros(0, dtype=np.int64))
    perm, x, y, w = sorted_samples(ts, lst)
    trees = fit(x, y, w, cell_counts_to_sorted(counts, perm))
    sr = predict(trees, ndvi_fine)
    out = correct(lst, sr) if do_correct else sr
    return out, dict(ts=ts, trees=trees, perm=perm, x=x, y=y, w=w, sr=sr)
