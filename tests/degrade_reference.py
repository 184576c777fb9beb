"""float64 NumPy restatement of the sensor model at any ratio (include/sifsr_degrade.h): the reference's
downscale_Aster_to_coarse / downscale_Aster_to_fine / generic_downscale / downscale_LST_SR_to_LR (utils.py:1642-1830) as ONE banded
operator per axis, out = Ry . x . Rx^T, built by composing the three steps literally:

    P  (Np, n)   reflect pad by hw without repeating the edge (-k -> k, n-1+k -> n-1-k), Np = n + 2 hw
    G  (Np, Np)  the normalised 1-D Gaussian with padding="same": taps that fall outside [0, Np) meet zeros (the darkened ring)
    C  (on, Np)  bicubic resampling as F.interpolate(scale_factor=1/factor, mode="bicubic") does it: on = floor(Np * (1/factor)),
                 scale = float32(1 / (1/factor)), s = scale * (o + 0.5f) - 0.5f in fp32, f = floor(s), t = s - f, the four source
                 indices f-1 .. f+2 clamped to [0, Np-1], Keys coefficients with A = -0.75 in float64 from the fp32 t
    crop         drops int(hw / factor) outputs on each side

R = C G P.  The stencil of output o is the set of original pixels with a non-zero weight in R[o]; o touches the zero ring iff a
blurred pixel it samples with a non-zero coefficient lies within hw of the padded edge.  out_valid = the whole 2-D stencil is valid
and neither axis touches the ring.  tests/test_degrade_host.py holds this file to the reference's recorded outputs."""
import math
import zlib

import numpy as np

A = -0.75
COARSE = 926.25 / 90
FINE = 231.656 / 90
MAX_HW = 16
FP32_FLOOR_SPLIT = 1328
# the cases of tests/golden/golden_degrade_v1.npz: (name, kind, shape, factor, mtf, hkw, crop, seed)
CASES = [
    ("coarse_12x12", "coarse", (12, 12), COARSE, 0.1, None, False, 11),
    ("coarse_12x40", "coarse", (12, 40), COARSE, 0.1, None, False, 12),
    ("coarse_97x131", "coarse", (97, 131), COARSE, 0.1, None, False, 13),
    ("fine_4x4", "fine", (4, 4), FINE, 0.1, None, False, 14),
    ("fine_61x83", "fine", (61, 83), FINE, 0.1, None, False, 15),
    ("fine_97x131", "fine", (97, 131), FINE, 0.1, None, False, 16),
    # output column 1328 is the first at which floor of the fp32 source coordinate is not floor of the float64 one (FP32_FLOOR_SPLIT)
    ("fine_4x3415", "fine", (4, 3415), FINE, 0.1, None, False, 19),
    ("generic_2x3x40x52", "generic", (2, 3, 40, 52), 2.0, 0.1, 3, False, 17),
    ("generic_4x4", "generic", (1, 1, 4, 4), 2.0, 0.1, 3, False, 18),
] + [(f"lr_f{f}_mtf{m}", "lr", (1, 1, 40, 52), float(f), m, None, True, 20 + 2 * f + (m > 0.1))
     for f in (2, 3, 4) for m in (0.1, 0.25)]
SWEEP_FACTORS = [(COARSE, None), (FINE, None), (2.0, 3)]      # crop off; with crop on the reference's hkw is None for all three


def half_width(factor, hkw=None):
    return int(math.ceil(factor)) if hkw is None else int(hkw)


def taps(factor, mtf, hkw=None):
    """the separable factor of generate_psf_kernel(1.0, factor, mtf, hkw): 2 hw + 1 float64 taps that sum to 1"""
    hw = half_width(factor, hkw)
    sigma = math.sqrt(-math.log(mtf) / 2) / (math.pi * (0.5 / factor))
    g = np.exp(-(np.arange(-hw, hw + 1, dtype=np.float64) ** 2) / (2 * sigma * sigma))
    return g / g.sum()


def out_side(n, factor, hkw=None, crop=False):
    hw = half_width(factor, hkw)
    full = int(math.floor(float(n + 2 * hw) * (1.0 / factor)))
    return full - (2 * int(hw / factor) if crop else 0)


def coords(n_pad, factor, count):
    """-> (s32 fp32, s64 float64, f, t float64 from the fp32 t) of the first `count` outputs; every fp32 step rounded on its own"""
    scale = np.float32(1.0 / (1.0 / factor))
    o = np.arange(count, dtype=np.float32)
    s32 = (scale * (o + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    s64 = (1.0 / (1.0 / factor)) * (np.arange(count, dtype=np.float64) + 0.5) - 0.5
    f = np.floor(s32)
    t = (s32 - f).astype(np.float32)
    return s32, s64, f.astype(np.int64), t.astype(np.float64)


def keys(t):
    """(count, 4) Keys coefficients of the sources f-1, f, f+1, f+2"""
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=1)


def axis_operator(n, factor, mtf=0.1, hkw=None, crop=False):
    """-> dict: R (on, n) float64, ring (on,) bool, idx (on, 4) the clamped blurred indices, raw (on, 4) the unclamped ones,
    coef (on, 4), hw, n_pad, cut"""
    hw = half_width(factor, hkw)
    if not (1 <= hw <= MAX_HW and n >= hw + 1):
        raise ValueError(f"side {n} with half width {hw}")
    g = taps(factor, mtf, hkw)
    n_pad = n + 2 * hw
    # G P, row q: the taps of blurred entry q over the original pixels; a tap beyond [0, n_pad) meets a zero and is dropped
    GP = np.zeros((n_pad, n))
    q = np.arange(n_pad)
    for k in range(-hw, hw + 1):
        p = q + k
        inside = (p >= 0) & (p < n_pad)
        i = p[inside] - hw
        i = np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
        np.add.at(GP, (q[inside], i), g[k + hw])
    full = int(math.floor(float(n_pad) * (1.0 / factor)))
    _, _, f, t = coords(n_pad, factor, full)
    coef = keys(t)
    raw = f[:, None] - 1 + np.arange(4)[None, :]
    idx = np.clip(raw, 0, n_pad - 1)
    sampled = coef != 0
    ring = (sampled & ((idx < hw) | (idx > n_pad - 1 - hw))).any(axis=1)
    R = sum(coef[:, a, None] * GP[idx[:, a]] for a in range(4))
    cut = int(hw / factor) if crop else 0
    sl = slice(cut, full - cut)
    if full - 2 * cut < 1:
        raise ValueError("no output left")
    return dict(R=R[sl], ring=ring[sl], idx=idx[sl], raw=raw[sl], coef=coef[sl], hw=hw, n_pad=n_pad, cut=cut)


def degrade_ref(x, factor, mtf=0.1, hkw=None, crop=False, valid=None, fill_value=np.nan):
    """x (..., H, W) -> (out float64 (..., oh, ow), out_valid bool (oh, ow)); valid (H, W) or None"""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    ay, ax = axis_operator(H, factor, mtf, hkw, crop), axis_operator(W, factor, mtf, hkw, crop)
    v = np.ones((H, W), bool) if valid is None else np.asarray(valid) != 0
    x0 = np.where(v, x.astype(np.float64), 0.0)
    out = ay["R"] @ x0 @ ax["R"].T
    bad = (ay["R"] != 0).astype(np.int64) @ (~v).astype(np.int64) @ (ax["R"] != 0).astype(np.int64).T
    ov = (bad == 0) & ~ay["ring"][:, None] & ~ax["ring"][None, :]
    if valid is not None:
        out = np.where(ov, out, fill_value)
    return out, ov


def make_field(shape, seed):
    """a synthetic LST field near 300 K: two smooth waves, a ramp and pixel noise, fp32"""
    rs = np.random.RandomState(seed)
    H, W = shape[-2:]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    lead = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    out = []
    for _ in range(lead):
        a, b, c = rs.uniform(0.05, 0.4, 3)
        f = 300.0 + 6.0 * np.sin(a * x + rs.uniform(0, 6)) * np.cos(b * y + rs.uniform(0, 6)) + 0.02 * c * (x - y)
        out.append(f + rs.standard_normal((H, W)) * 1.5)
    return np.stack(out).reshape(shape).astype(np.float32)


def case_input(name):
    for c in CASES:
        if c[0] == name:
            return make_field(c[2], c[7])
    raise KeyError(name)


def checksum(a):
    return zlib.crc32(np.ascontiguousarray(a, np.float32).tobytes())


def quad_valid(H, W):
    """a rotated quadrilateral in a zero-filled raster, as an ASTER scene lies in its bounding box -> (H, W) uint8"""
    corners = np.array([[0.08 * H, 0.30 * W], [0.25 * H, 0.95 * W], [0.93 * H, 0.72 * W], [0.70 * H, 0.04 * W]])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    inside = np.ones((H, W), bool)
    for k in range(4):
        (y0, x0), (y1, x1) = corners[k], corners[(k + 1) % 4]
        inside &= (x1 - x0) * (y - y0) - (y1 - y0) * (x - x0) >= 0
    return inside.astype(np.uint8)
