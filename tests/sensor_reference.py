"""float64 NumPy restatement of the differentiable sensor model (include/sifsr_sensor.h), built on the banded
operator of tests/degrade_reference.py:

    axis_operator       degrade_reference.axis_operator with the source coordinate as sifsrs_degrade's table kernel forms it: ONE
                        rounding to fp32 of scale * (o + 0.5) - 0.5 (the compiled kernel holds one v_fma_f32), where
                        degrade_reference.coords rounds the product and the difference separately.  The two differ by one ulp of
                        the coordinate on the few outputs per axis whose product lies in [2^k, 2^k + 0.5): weights by <= 1.5e-7,
                        outputs by <= 3e-5 K -- under the 2e-4 K bar of the forward's tests, far above one fp32 rounding of a
                        gradient.  The adjoint must be the transpose of the operator the forward applies, so it is held per
                        element to THIS R.  (The torch build that recorded the goldens forms the coordinate with one rounding as
                        well; the recordings lie equally near either restatement.)
    downscale_ref / downscale_bwd_ref   out = Ry . x . Rx^T and dx = Ry^T . dout . Rx with that R: downscale_LST_SR_to_LR(x, factor=f)
                        (utils.py:1671-1706), generic_downscale, downscale_Aster_to_* and their autograd gradients
    lowpass_operator    L (n, n): get_output_ftm(factor=f) (utils.py:1833-1860) per axis -- reflect pad by hw without repeating the
                        edge, the 2 hw + 1 float64 taps of degrade_reference.taps, the crop by hw (no zero ring survives it)
    input_ranges        per input pixel the run [o_lo, o_hi] of outputs whose stencil holds it (the device's range table)
    loss_ref            the eight lines of oracle.sr2_loss / sr1_loss at a factor, through the factor arguments that
                        oracle.downscale_LST_SR_to_LR / get_output_ftm already have; float64 when its inputs are

tests/test_sensor_host.py holds this file to the reference's recorded outputs and gradients (tests/golden/golden_sensor_v1.npz)."""
import contextlib
import zlib

import numpy as np

from tests import degrade_reference as R

COARSE = R.COARSE
FACTORS = [2.0, 2.5, 3.0, 4.0, COARSE]
SHAPES = [(2, 1, 24, 40), (1, 1, 40, 24), (1, 1, 12, 12)]
DOWN_MTF = 0.1           # the mtf of the recorded downscale_LST_SR_to_LR calls
LOWPASS_MTF = 0.25       # ... and of the get_output_ftm calls
# the cases of tests/golden/golden_sensor_v1.npz: (name, shape, factor, seed)
CASES = [(f"f{f:.4g}_{'x'.join(map(str, s))}", s, f, 100 + 10 * i + j) for i, f in enumerate(FACTORS) for j, s in enumerate(SHAPES)]
# the sweep over which stencil monotonicity is held (tests/test_sensor_host.py): (factor, hkw)
SWEEP = [(COARSE, None), (R.FINE, None), (2.0, 3), (2.0, None), (2.5, None), (3.0, None), (4.0, None), (1.25, 16), (1.5, 16),
         (1.001, 1), (7.3, 5), (16.0, None)]


def coords(n_pad, factor, count):
    """degrade_reference.coords with the fp32 coordinate in one rounding: scale (24 bits) times o + 0.5 (15 bits) minus 0.5 is exact
    in float64, so the cast is the fused multiply-add's rounding"""
    scale = np.float32(1.0 / (1.0 / factor))
    o = np.arange(count, dtype=np.float64)
    s32 = (np.float64(scale) * (o + 0.5) - 0.5).astype(np.float32)
    s64 = (1.0 / (1.0 / factor)) * (o + 0.5) - 0.5
    f = np.floor(s32)
    t = (s32 - f).astype(np.float32)                       # exact
    return s32, s64, f.astype(np.int64), t.astype(np.float64)


@contextlib.contextmanager
def _kernel_coordinates():
    prev, R.coords = R.coords, coords
    try:
        yield
    finally:
        R.coords = prev


def axis_operator(n, factor, mtf=0.1, hkw=None, crop=False):
    """degrade_reference.axis_operator, every step of it, over the coordinates above -> the same dict"""
    with _kernel_coordinates():
        return R.axis_operator(n, factor, mtf, hkw, crop)


def differing_outputs(n_pad, factor, count):
    """the outputs at which the two coordinate rules differ"""
    return np.nonzero(coords(n_pad, factor, count)[0] != R.coords(n_pad, factor, count)[0])[0]


def stencils(axis):
    """-> (lo, hi) int arrays: the span of original pixels with a non-zero weight per output of axis_operator's result"""
    nz = axis["R"] != 0
    assert nz.any(axis=1).all()
    lo = nz.argmax(axis=1)
    hi = nz.shape[1] - 1 - nz[:, ::-1].argmax(axis=1)
    return lo, hi


def table_stencils(axis, n):
    """-> (lo, hi): the stencil as the device's table kernel stores it (csrc/degrade.hip fold_range): the original pixels that the
    blurred entries sampled with a non-zero coefficient reach through the taps and the reflection -- a span that holds every non-zero
    weight.  The device's range table is the bisection of these two arrays."""
    hw, n_pad = axis["hw"], axis["n_pad"]
    sampled = axis["coef"] != 0
    q_lo = np.where(sampled, axis["idx"], n_pad).min(axis=1)
    q_hi = np.where(sampled, axis["idx"], -1).max(axis=1)
    i_lo = np.maximum(q_lo - hw, 0) - hw
    i_hi = np.minimum(q_hi + hw, n_pad - 1) - hw
    a, b = np.maximum(i_lo, 0), np.minimum(i_hi, n - 1)
    b = np.where(i_lo < 0, np.maximum(b, -i_lo), b)
    a = np.where(i_lo < 0, 0, a)
    a = np.where(i_hi >= n, np.minimum(a, 2 * (n - 1) - i_hi), a)
    return a, b


def input_ranges(axis):
    """-> (n, 2) int: per input pixel i the first and last output whose stencil [lo, hi] contains i, (count, -1)-style empty
    runs as first > last.  Raises if the outputs that contain i are not one run."""
    lo, hi = stencils(axis)
    n = axis["R"].shape[1]
    out = np.zeros((n, 2), np.int64)
    for i in range(n):
        inside = np.nonzero((lo <= i) & (i <= hi))[0]
        if inside.size == 0:
            first = int(np.searchsorted(hi, i, side="left"))
            out[i] = (first, first - 1)
            continue
        if not np.array_equal(inside, np.arange(inside[0], inside[-1] + 1)):
            raise ValueError(f"the outputs over pixel {i} are not one run: {inside}")
        out[i] = (inside[0], inside[-1])
    return out


def downscale_ref(x, factor, mtf=0.1, hkw=None, crop=True):
    """x (..., H, W) -> out (..., oh, ow) float64"""
    x = np.asarray(x, np.float64)
    return axis_operator(x.shape[-2], factor, mtf, hkw, crop)["R"] @ x @ axis_operator(x.shape[-1], factor, mtf, hkw, crop)["R"].T


def downscale_bwd_ref(dout, shape, factor, mtf=0.1, hkw=None, crop=True, out_valid=None):
    """dout (..., oh, ow) -> dx (..., H, W) float64, (H, W) = shape; out_valid (oh, ow) or shaped as dout: outputs that count"""
    H, W = shape
    ay, ax = axis_operator(H, factor, mtf, hkw, crop), axis_operator(W, factor, mtf, hkw, crop)
    d = np.asarray(dout, np.float64)
    if out_valid is not None:
        d = np.where(np.asarray(out_valid) != 0, d, 0.0)
    return ay["R"].T @ d @ ax["R"]


def lowpass_operator(n, factor, mtf=0.1, hkw=None):
    """L (n, n) float64: out = L @ x along one axis"""
    hw = R.half_width(factor, hkw)
    if not (1 <= hw <= R.MAX_HW and n >= hw + 1):
        raise ValueError(f"side {n} with half width {hw}")
    g = R.taps(factor, mtf, hkw)
    L = np.zeros((n, n))
    o = np.arange(n)
    for k in range(-hw, hw + 1):
        p = o + k
        p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))
        np.add.at(L, (o, p), g[k + hw])
    return L


def lowpass_ref(x, factor, mtf=0.1, hkw=None):
    x = np.asarray(x, np.float64)
    return lowpass_operator(x.shape[-2], factor, mtf, hkw) @ x @ lowpass_operator(x.shape[-1], factor, mtf, hkw).T


def lowpass_bwd_ref(dout, factor, mtf=0.1, hkw=None):
    d = np.asarray(dout, np.float64)
    return lowpass_operator(d.shape[-2], factor, mtf, hkw).T @ d @ lowpass_operator(d.shape[-1], factor, mtf, hkw)


def loss_ref(kind, sr, lst, ndvi, factor, mean, std, alpha, gamma):
    """oracle.sr2_loss / sr1_loss with the sensor model at `factor`: torch tensors (float64 for the yardstick) ->
    (ds, pl, loss), differentiable with respect to sr"""
    from oracle import sif_oracle as O
    down = (O.downscale_LST_SR_to_LR(sr * std + mean, factor=factor, mtf=DOWN_MTF) - mean) / std
    ds = O.huber(down, lst)
    if kind == "sr2":
        pl = O.huber(sr - O.get_output_ftm(sr, factor=factor, mtf=LOWPASS_MTF),
                     gamma * (ndvi - O.get_output_ftm(ndvi, factor=factor, mtf=LOWPASS_MTF)))
    else:
        pl = O.huber(O.sobel_bank(sr), gamma * O.sobel_bank(ndvi))
    return ds, pl, alpha * ds + (1 - alpha) * pl


# ---- the golden file's seeded inputs --------------------------------------------------------------------------------------------
def case_input(name):
    """-> (x fp32 near 300 K, d_down fp32 unit-normal cotangent of the downscaled raster, d_low the same for the low-pass)"""
    for n, shape, factor, seed in CASES:
        if n == name:
            x = R.make_field(shape, seed)
            rs = np.random.RandomState(seed + 5000)
            oh, ow = R.out_side(shape[-2], factor, None, True), R.out_side(shape[-1], factor, None, True)
            d_down = rs.standard_normal(shape[:-2] + (oh, ow)).astype(np.float32)
            d_low = rs.standard_normal(shape).astype(np.float32)
            return x, d_down, d_low
    raise KeyError(name)


def checksum(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a, np.float32).tobytes(), c)
    return c
