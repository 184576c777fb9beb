"""Float64 restatements of the operators around the 3x3 convs (thin first / last conv, BatchNorm backward, pooling, bilinear x2
upsampling, their adjoints, the fused head and tail) and the per-element error bound the storage-edge tests hold the HIP kernels to.

Everything is NCHW on the CPU and takes the values the device tensors HOLD: for bf16 storage the bf16-rounded inputs, widened
(``rb``).  Every function that has a bound returns the pair (ref, ref_abs); ref_abs is the same operator evaluated on the absolute
values of all its inputs and weights (the ReLU'd magnitudes where a BatchNorm+ReLU is folded in) -- the yardstick of fp32 rounding.

The bound (no measured constant enters it):
    delta = k * 2^-24 * ref_abs,  k = K[op] = accumulated terms per output + 8
    fp32-stored output:  |got - ref| <= delta
    bf16-stored output:  |got - ref| <= 2^-8 |ref| + 2 delta
The bf16 line is ONE round-to-nearest-even of an fp32 value v that is itself within delta of ref: RNE to 8 significant bits errs
by at most half an ulp <= 2^-8 |v| <= 2^-8 (|ref| + delta), plus the delta of v itself.

Reduced fp32 outputs (weight / bias gradients, dgamma, dbeta, statistic partial sums) are held to the project's bars, relative to
the same sum over absolute values (``sum_abs``), never to the signed result, which can cancel: BAR_SUM for weight gradients and
(sum dz, sum dz*y) partial sums, BAR_TOL for dgamma / dbeta and what the fp32 tests hold at TOL."""
import torch

U = 2.0 ** -24           # unit roundoff of fp32
BF_EPS = 2.0 ** -8       # half an ulp of bf16 (8 significant bits), relative
BAR_SUM = 1e-5
BAR_TOL = 1e-4
BF = torch.bfloat16

# accumulated terms per output + 8
K = {
    "pool": 12,            # 4 ReLU'd values (each one rounding of the exact fma) + 8
    "pool_bwd": 10,        # 0.25 * gp (exact) + g: 2 terms + 8
    "add": 10,             # p + relu(fma): 2 terms + 8
    "up2x": 12,            # 4 taps + 8
    "up2x_bwd": 33,        # 5 x 5 high-resolution pixels + 8
    "bn_bwd_dy": 16,       # sd*dz + k1*y + k0 (3 terms, float64, rounded once) + the reduced sums' roundings (partial store, the two
                           # of xhat = (y - mean) * invstd, the pooled addend, the final store: 5) + 8
    "g_complete": 10,      # g + 0.25 * gpool: 2 terms + 8
    "conv_in_fwd": 26,     # 2 channels x 9 taps + 8
    "conv_out_fwd": 153,   # 16 channels x 9 taps + bias + 8
    "conv_out_dgrad": 21,  # 9 taps, each a sum of up to 4 border-folded pixels (3 additions, counted once over the 9: 4) + 8
    "tail_dy": 37,         # conv_out_dgrad (13) feeding bn_bwd_dy (16) + 8
}


def rb(t):
    """what a bf16 tensor holds, as float32"""
    return t.to(BF).float()


def stored(t, bf16):
    return rb(t) if bf16 else t.float()


def _c(v):
    return v.double().view(1, -1, 1, 1)


def preact(y, sc, sh):
    """z = y*sc + sh in float64: for float inputs the product is exact and the sum is rounded once, so sign(z) is the sign of the
    kernels' single-rounded fmaf.  Callers assert z != 0 (no tie tolerance)."""
    z = y.double() * _c(sc) + _c(sh)
    assert bool((z != 0).all()), "a pre-activation is exactly zero: choose another seed"
    return z


def bnrelu(y, sc, sh):
    """relu(y*sc + sh), or y itself with sc None -> (a, |a|)"""
    if sc is None:
        return y.double(), y.double().abs()
    a = preact(y, sc, sh).clamp_min(0.0)
    return a, a


def pool2(a, a_abs):
    f = lambda t: 0.25 * t.reshape(t.shape[0], t.shape[1], t.shape[2] // 2, 2, t.shape[3] // 2, 2).sum((3, 5))
    return f(a), f(a_abs)


def pool2_adj(gp):
    return 0.25 * gp.double().repeat_interleave(2, 2).repeat_interleave(2, 3)


def pool2_bwd(gp, g=None):
    """adjoint of AvgPool2d(2, 2), added to g when given -> (ref, ref_abs)"""
    r, ra = pool2_adj(gp), pool2_adj(gp.double().abs())
    return (r, ra) if g is None else (r + g.double(), ra + g.double().abs())


def add(p, a, a_abs):
    return p.double() + a, p.double().abs() + a_abs


def interp_matrix(n):
    """(2n, n) float64 matrix of Upsample(x2, bilinear, align_corners=True), built from ATen's float32 recipe:
    ratio = (in-1)/(out-1) (0 when out <= 1), src = ratio*o, i0 = int(src), lambda = src - i0 -- all float32."""
    f32 = torch.float32
    out = 2 * n
    ratio = (torch.tensor(float(n - 1), dtype=f32) / torch.tensor(float(out - 1), dtype=f32)) if out > 1 else torch.zeros((), dtype=f32)
    M = torch.zeros(out, n, dtype=torch.float64)
    for o in range(out):
        src = ratio * torch.tensor(float(o), dtype=f32)
        i0 = int(src)
        i1 = i0 + (1 if i0 < n - 1 else 0)
        l1 = src - torch.tensor(float(i0), dtype=f32)
        l0 = torch.tensor(1.0, dtype=f32) - l1
        M[o, i0] += float(l0)
        M[o, i1] += float(l1)
    return M


def up2x(a, a_abs, My=None, Mx=None):
    """My . A . Mx^T (the weights are non-negative, so the same matrices serve ref_abs)"""
    My = interp_matrix(a.shape[2]) if My is None else My
    Mx = interp_matrix(a.shape[3]) if Mx is None else Mx
    f = lambda t: torch.einsum("oh,bchw,pw->bcop", My, t.double(), Mx)
    return f(a), f(a_abs)


def up2x_adj(gu, My=None, Mx=None):
    """My^T . G . Mx -> (ref, ref_abs)"""
    My = interp_matrix(gu.shape[2] // 2) if My is None else My
    Mx = interp_matrix(gu.shape[3] // 2) if Mx is None else Mx
    f = lambda t: torch.einsum("oh,bcop,pw->bchw", My, t, Mx)
    return f(gu.double()), f(gu.double().abs())


def sum_abs(*terms):
    """per-channel sum over (B, H, W) of the product of |terms|"""
    p = terms[0].double().abs()
    for t in terms[1:]:
        p = p * t.double().abs()
    return p.sum((0, 2, 3))


def bn_sums_y(g, y, sc, sh):
    """(sum dz, sum dz*y) per channel, dz = g*[y*sc + sh > 0] -> ((C, 2) ref, (C, 2) ref_abs)"""
    dz = torch.where(preact(y, sc, sh) > 0, g.double(), torch.zeros((), dtype=torch.float64))
    return (torch.stack((dz.sum((0, 2, 3)), (dz * y.double()).sum((0, 2, 3))), 1),
            torch.stack((sum_abs(dz), sum_abs(dz, y)), 1))


def bn_bwd(g, y, scale, shift, mean, invstd, g_abs=None):
    """BatchNorm(training) + ReLU backward from the folded coefficients the device gets:
    dz = g*[z > 0], dbeta = sum dz, dgamma = sum dz*xhat, dy = scale*dz + k1*y + k0 with k1 = -scale*invstd*dgamma/N,
    k0 = -scale*dbeta/N - k1*mean.  -> dict of refs and their absolute-value twins (g_abs: the magnitude twin of g where g is
    itself a computed quantity; default |g|).  xhat's magnitude is |y - mean| * invstd: a float subtraction of two inputs errs
    relative to its RESULT, so the difference is an input-level quantity, not a cancellation to be charged."""
    n = y.shape[0] * y.shape[2] * y.shape[3]
    pos = preact(y, scale, shift) > 0
    zero = torch.zeros((), dtype=torch.float64)
    dz = torch.where(pos, g.double(), zero)
    dz_a = dz.abs() if g_abs is None else torch.where(pos, g_abs.double(), zero)
    xhat = (y.double() - _c(mean)) * _c(invstd)
    db, dg = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
    db_a, dg_a = sum_abs(dz_a), sum_abs(dz_a, xhat)
    sd, isd, mu = scale.double(), invstd.double(), mean.double()
    k1 = -sd * isd * dg / n
    k0 = -sd * db / n - k1 * mu
    dy = _c(sd) * dz + _c(k1) * y.double() + _c(k0)
    k1_a = sd.abs() * isd.abs() * dg_a / n
    dy_a = _c(sd.abs()) * dz_a +_c(k1_a) * (y.double().abs() + _c(mu.abs())) + _c(sd.abs() * db_a / n)
    return dict(dz=dz, dbeta=db, dgamma=dg, dbeta_abs=db_a, dgamma_abs=dg_a, dy=dy, dy_abs=dy_a,
                coef=torch.cat((sd, k1, k0)), coef_abs=torch.cat((sd.abs(), k1_a, sd.abs() * db_a / n + k1_a * mu.abs())))


def coef_from_sums(db, dg, scale, shift, mean, invstd, beta, n):
    """the finalize step alone, float64 from given (dbeta, dgamma): coef = [sd | k1 | k0] (float64, 3C) and coef_f = [sc | sh | k1f |
    k0f] (4C) with k1f = -invstd*dgamma/N and k0f = -scale*dbeta/N - k1f*beta (dy = sc*dz + k1f*z + k0f on z = y*sc + sh); each with
    its absolute-value twin."""
    sd, isd, mu = scale.double(), invstd.double(), mean.double()
    k1 = -sd * isd * dg / n
    coef = torch.cat((sd, k1, -sd * db / n - k1 * mu))
    coef_a = torch.cat((sd.abs(), k1.abs(), (sd * db / n).abs() + (k1 * mu).abs()))
    if beta is None:
        return coef, coef_a, None, None
    k1f = -isd * dg / n
    coef_f = torch.cat((sd, shift.double(), k1f, -sd * db / n - k1f * beta.double()))
    coef_f_a = torch.cat((sd.abs(), shift.double().abs(), k1f.abs(), (sd * db / n).abs() + (k1f * beta.double()).abs()))
    return coef, coef_a, coef_f, coef_f_a


# ---- 3x3 convolution with replicate padding, written out tap by tap on clamped indices ----
def _clamped(n, k):
    return (torch.arange(n) + k - 1).clamp(0, n - 1)


def conv3_rep(a, w, bias=None):
    """out[b,o,y,x] = bias[o] + sum_{i,ky,kx} w[o,i,ky,kx] * a[b,i,clamp(y+ky-1),clamp(x+kx-1)]"""
    a, w = a.double(), w.double()
    H, W = a.shape[2:]
    out = torch.zeros(a.shape[0], w.shape[0], H, W, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("oi,bihw->bohw", w[:, :, ky, kx], a[:, :, _clamped(H, ky)][:, :, :, _clamped(W, kx)])
    return out if bias is None else out + bias.double().view(1, -1, 1, 1)


def conv3_rep_dgrad(g, w):
    """adjoint of conv3_rep in its input: every output pixel's gradient goes to the clamped pixel its tap read"""
    g, w = g.double(), w.double()
    H, W = g.shape[2:]
    out = torch.zeros(g.shape[0], w.shape[1], H, W, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            t = torch.einsum("oi,bohw->bihw", w[:, :, ky, kx], g)
            rows = torch.zeros_like(t).index_add_(2, _clamped(H, ky), t)
            out += torch.zeros_like(t).index_add_(3, _clamped(W, kx), rows)
    return out


def conv3_rep_wgrad(a, g):
    """dw[o,i,ky,kx] = sum_{b,y,x} g[b,o,y,x] * a[b,i,clamp(y+ky-1),clamp(x+kx-1)]"""
    a, g = a.double(), g.double()
    H, W = a.shape[2:]
    dw = torch.zeros(g.shape[1], a.shape[1], 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", g, a[:, :, _clamped(H, ky)][:, :, :, _clamped(W, kx)])
    return dw


def with_abs(f, *args):
    """(f(args), f(|args|)) for the bilinear maps above"""
    return f(*args), f(*[None if t is None else t.double().abs() for t in args])


# ---- the bound ----
def bound(ref, ref_abs, k, bf16):
    delta = k * U * ref_abs.double()
    return BF_EPS * ref.double().abs() + 2.0 * delta if bf16 else delta


def check(got, ref, ref_abs, k, bf16, what=""):
    """assert |got - ref| <= bound per element; returns the largest error / bound (0/0 counts as 0)"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (what, "non-finite output")
    err, bnd = (got - ref).abs(), bound(ref, ref_abs, k, bf16)
    ratio = torch.where(err > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError((what, "error/bound", worst, "at flat index", i, "got", float(got.flatten()[i]), "ref",
                              float(ref.flatten()[i]), "elements over", int((ratio > 1).sum()), "of", ratio.numel()))
    return worst


def check_sum(got, ref, ref_abs, bar, what=""):
    """reduced outputs: |got - ref| <= bar * ref_abs per element; returns the largest error / (bar * ref_abs)"""
    got, ref, ref_abs = got.double(), ref.double(), ref_abs.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (what, "non-finite output")
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / (bar * ref_abs).clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= 1.0, (what, "error/bar", worst, "bar", bar)
    return worst
