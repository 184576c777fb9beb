"""The operators around the 3x3 convs -- thin first / last conv, BatchNorm reductions, pooling / upsampling with their adjoints, the
fused head and tail -- in both activation-storage modes (fp32 and bf16, sifsr_set_op_storage_bf16) at the shapes where a pixel is
both borders, a tile is partial, a workgroup is empty or a grid cap is passed, against the float64 restatements and the derived
per-element bound of tests/storage_reference.py (no measured constant: delta = k 2^-24 ref_abs; bf16 outputs one RNE of a value
within delta).  Every output lives between two sentinel guards inside a larger allocation and is NaN-filled before the launch.

Which kernel serves a case cannot be observed from outside other than through its results; `tile_form` restates the launch rule
(resample.hip) and is held against what IS observable: sifsr_up2x_bwd_stat_rows and the argument error of the fused sums where only
the generic kernel exists.

SIFSR_STORAGE_EDGE_REPORT=<path>: write the largest error / bound per operator group and storage mode there (DESIGN.md's table)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import storage_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 256            # guard ELEMENTS on both sides (>= 256 bytes for every dtype used)
SENT = -416.0          # exactly representable in bf16
ERR_SHAPE, ERR_ARG = 1001, 1002
WORST = {}


@pytest.fixture(scope="module")
def sifsr():
    import sifsr as pkg
    assert torch.cuda.is_available()
    return pkg


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SIFSR_STORAGE_EDGE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({k: {"tensors": v[0], "worst_error_over_bound": v[1]} for k, v in sorted(WORST.items())}, f, indent=1)


@pytest.fixture(params=[False, True], ids=["fp32", "bf16"])
def hs(request, sifsr):
    """the storage mode of the single-operator entry points for one test; restored on teardown"""
    from sifsr import _lib
    _lib.call("sifsr_set_op_storage_bf16", 1 if request.param else 0)
    yield request.param
    _lib.call("sifsr_set_op_storage_bf16", 0)


@pytest.fixture()
def L(sifsr):
    from sifsr import _lib
    return _lib


def S():
    return torch.cuda.current_stream().cuda_stream


def note(group, bf16, ratio):
    key = f"{group}/{'bf16' if bf16 else 'fp32'}"
    n, w = WORST.get(key, (0, 0.0))
    WORST[key] = (n + 1, max(w, float(ratio)))


class Out:
    """an output tensor inside a larger allocation: [GUARD sentinels | payload | GUARD sentinels]; the payload starts NaN-filled
    (or holds `init` for operators that update in place)"""

    def __init__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)
        self.n = n

    def ok(self, what=""):
        g = torch.cat((self.buf[:GUARD], self.buf[GUARD + self.n:])).float()
        assert bool((g == SENT).all()), (what, "guard overwritten")
        return self.t


def act_dtype(bf16):
    return BF if bf16 else torch.float32


def dev(t, bf16):
    """NCHW host values -> NHWC device tensor in the storage mode"""
    return t.permute(0, 2, 3, 1).contiguous().to(act_dtype(bf16)).cuda()


def host(t):
    """NHWC device tensor -> NCHW float host"""
    return t.float().permute(0, 3, 1, 2).cpu()


def vals(rs, shape, bf16, scale=1.0, off=0.0):
    return R.stored(torch.from_numpy((scale * rs.standard_normal(shape) + off).astype(np.float32)), bf16)


def chan(rs, C):
    sc = torch.from_numpy(rs.uniform(0.5, 1.5, C).astype(np.float32))
    sh = torch.from_numpy((0.3 * rs.standard_normal(C)).astype(np.float32))
    return sc, sh


def act_out(B, H, W, C, bf16, init=None):
    return Out((B, H, W, C), act_dtype(bf16), None if init is None else init.permute(0, 2, 3, 1).to(act_dtype(bf16)))


def raw_bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ pool, adjoint, add
def run_pool_add(L, hs, B, H, W, C, rs, group):
    y, p = vals(rs, (B, C, H, W), hs), vals(rs, (B, C, H, W), hs)
    sc, sh = chan(rs, C)
    dy_, dp = dev(y, hs), dev(p, hs)
    for with_bn in (True, False):
        dsc, dsh = (sc.cuda(), sh.cuda()) if with_bn else (None, None)
        a, a_abs = R.bnrelu(y, sc if with_bn else None, sh if with_bn else None)
        o = act_out(B, H // 2, W // 2, C, hs)
        L.call("sifsr_bnrelu_pool2", dy_, dsc, dsh, o.t, B, H, W, C, S())
        ref, ref_abs = R.pool2(a, a_abs)
        note(group + ":pool", hs, R.check(host(o.ok("pool")), ref, ref_abs, R.K["pool"], hs, ("pool", with_bn)))
        o = act_out(B, H, W, C, hs)
        L.call("sifsr_bnrelu_add", dp, dy_, dsc, dsh, o.t, C, B * H * W, S())
        ref, ref_abs = R.add(p, a, a_abs)
        note(group + ":add", hs, R.check(host(o.ok("add")), ref, ref_abs, R.K["add"], hs, ("add", with_bn)))
    gp = vals(rs, (B, C, H // 2, W // 2), hs)
    dgp = dev(gp, hs)
    for accumulate in (0, 1):
        o = act_out(B, H, W, C, hs, init=p if accumulate else None)
        L.call("sifsr_pool2_bwd", dgp, o.t, B, H, W, C, accumulate, S())
        ref, ref_abs = R.pool2_bwd(gp, p if accumulate else None)
        note(group + ":pool_bwd", hs, R.check(host(o.ok("pool_bwd")), ref, ref_abs, R.K["pool_bwd"], hs, ("pool_bwd", accumulate)))


@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 6, 10), (2, 18, 34)])
@pytest.mark.parametrize("C", [8, 16, 32, 64])
def test_pool_adjoint_add(L, hs, C, shape):
    B, H, W = shape
    run_pool_add(L, hs, B, H, W, C, np.random.RandomState(100 + C + H), "pool/add")


def test_pool_adjoint_add_past_the_grid_cap(L, hs):
    """(1, 520, 520) at C = 64: 4,326,400 quads, more than the 16384 x 256 threads the grid-stride kernels launch"""
    B, H, W, C = 1, 520, 520, 64
    assert B * H * W * C // 4 > 16384 * 256
    run_pool_add(L, hs, B, H, W, C, np.random.RandomState(5), "pool/add")


# ------------------------------------------------------------------------------------------------ upsample and adjoint
def tile_form(op, C, Hin, Win):
    """the launch rule of resample.hip: tiled kernels for the model's channel counts; the forward one needs two source pixels per axis"""
    return C in (16, 32, 64) and (op == "bwd" or (Hin >= 2 and Win >= 2))


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (3, 5), (7, 9), (8, 8), (9, 17), (12, 20)])
@pytest.mark.parametrize("C", [8, 16, 32, 64])
def test_upsample_and_adjoint(L, hs, C, hw):
    Hin, Win = hw
    My, Mx = R.interp_matrix(Hin), R.interp_matrix(Win)
    for B in (1, 3):
        rs = np.random.RandomState(1000 * B + 10 * Hin + Win + C)
        y = vals(rs, (B, C, Hin, Win), hs)
        sc, sh = chan(rs, C)
        dy_ = dev(y, hs)
        dsc, dsh = sc.cuda(), sh.cuda()
        for with_bn in (True, False):
            a, a_abs = R.bnrelu(y, sc if with_bn else None, sh if with_bn else None)
            o = act_out(B, 2 * Hin, 2 * Win, C, hs)
            L.call("sifsr_bnrelu_up2x", dy_, dsc if with_bn else None, dsh if with_bn else None, o.t, B, Hin, Win, C, S())
            ref, ref_abs = R.up2x(a, a_abs, My, Mx)
            note("up2x", hs, R.check(host(o.ok("up2x")), ref, ref_abs, R.K["up2x"], hs, ("up2x", B, with_bn, tile_form("fwd", C, Hin, Win))))
        gu = vals(rs, (B, C, 2 * Hin, 2 * Win), hs)
        dgu = dev(gu, hs)
        g = act_out(B, Hin, Win, C, hs)
        L.call("sifsr_up2x_bwd", dgu, g.t, B, Hin, Win, C, S())
        ref, ref_abs = R.up2x_adj(gu, My, Mx)
        g_host = host(g.ok("up2x_bwd"))
        note("up2x_bwd", hs, R.check(g_host, ref, ref_abs, R.K["up2x_bwd"], hs, ("up2x_bwd", B, tile_form("bwd", C, Hin, Win))))
        # the fused BatchNorm-backward sums exist in the tiled form only
        rows = L.call("sifsr_up2x_bwd_stat_rows", B, Hin, Win, C)
        ty, tx = (Hin + 7) // 8, (Win + 7) // 8
        assert rows == (B * ty * tx if tile_form("bwd", C, Hin, Win) else 0)
        g2 = act_out(B, Hin, Win, C, hs)
        if rows == 0:
            part = Out((1, C, 2))
            rc = L.lib().sifsr_up2x_bwd_bn_sums(dgu.data_ptr(), g2.t.data_ptr(), B, Hin, Win, C, dy_.data_ptr(), dsc.data_ptr(),
                                               dsh.data_ptr(), part.t.data_ptr(), S())
            torch.cuda.synchronize()
            assert rc == ERR_ARG and bool(torch.isnan(g2.ok().float()).all()) and bool(torch.isnan(part.ok()).all())
            continue
        part = Out((rows, C, 2))
        L.call("sifsr_up2x_bwd_bn_sums", dgu, g2.t, B, Hin, Win, C, dy_, dsc, dsh, part.t, S())
        assert torch.equal(raw_bits(g2.ok("bn_sums g")), raw_bits(g.t))              # bit-equal to the plain adjoint's
        got = part.ok("bn_sums partials").cpu()
        for b in range(B):
            for j in range(ty):
                for i in range(tx):
                    sl = (slice(b, b + 1), slice(None), slice(8 * j, min(8 * j + 8, Hin)), slice(8 * i, min(8 * i + 8, Win)))
                    ref, ref_abs = R.bn_sums_y(g_host[sl], y[sl], sc, sh)              # the sums are those of the STORED gradient
                    note("up2x_bwd_bn_sums", hs, R.check_sum(got[(b * ty + j) * tx + i], ref, ref_abs, R.BAR_SUM, ("bn_sums row", b, j, i)))


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def bn_case(rs, B, C, H, W, hs):
    y = vals(rs, (B, C, H, W), hs, 1.5, 0.7)
    g = vals(rs, (B, C, H, W), hs)
    gp = vals(rs, (B, C, H // 2, W // 2), hs)
    gamma, beta = chan(rs, C)
    mean64 = y.double().mean((0, 2, 3))
    invstd64 = 1.0 / torch.sqrt(y.double().var((0, 2, 3), unbiased=False) + 1e-5)
    mean, invstd = mean64.float(), invstd64.float()
    scale = gamma * invstd
    shift = beta - mean * scale
    return y, g, gp, beta, mean, invstd, scale, shift


def check_coef(L, hs, part, nblk, C, npix, scale, shift, mean, invstd, beta, coef, coef_f, what):
    """the finalize step against float64 from the device's own partial rows: coef to 1e-12, coef_f to one float rounding"""
    p = part.double().cpu().view(nblk, C, 2)
    assert bool(torch.isfinite(p).all()), (what, "partials")
    PP = 1024 // C                                                     # pixels a workgroup covers per pass
    empty = [b for b in range(nblk) if b * PP >= npix]
    assert all(bool((p[b] == 0).all()) for b in empty), (what, "an empty workgroup left a non-zero partial")
    db, dg = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    db_a, dg_a = p[:, :, 0].abs().sum(0), p[:, :, 1].abs().sum(0)
    ref, _, ref_f, _ = R.coef_from_sums(db, dg, scale, shift, mean, invstd, beta, npix)
    sd_a = scale.double().abs()
    k1_a = sd_a * invstd.double() * dg_a / npix
    ref_a = torch.cat((sd_a, k1_a, sd_a * db_a / npix + k1_a * mean.double().abs()))
    note("bn_bwd:coef", hs, R.check_sum(coef.cpu(), ref, ref_a, 1e-12, (what, "coef")))
    if coef_f is not None:
        cf = coef_f.cpu()
        assert torch.equal(cf[:C], scale) and torch.equal(cf[C:2 * C], shift), (what, "coef_f sc | sh")
        k1f_a = invstd.double() * dg_a / npix
        ref_f_a = torch.cat((scale.double().abs(), shift.double().abs(), k1f_a, (scale.double() * db_a / npix).abs() + k1f_a * beta.double().abs()))
        note("bn_bwd:coef_f", hs, R.check_sum(cf, ref_f, ref_f_a, 2.0 ** -23, (what, "coef_f")))


def run_bn_bwd(L, hs, B, C, H, W, nblk, rs, with_coef=True):
    y, g, gp, beta, mean, invstd, scale, shift = bn_case(rs, B, C, H, W, hs)
    npix = B * H * W
    dy_, dgp = dev(y, hs), dev(gp, hs)
    dv = [t.cuda() for t in (scale, shift, mean, invstd)]
    for with_pool in (False, True):
        what = ("bn_relu_bwd", B, C, H, W, nblk, with_pool)
        g_eff, g_eff_abs = R.pool2_bwd(gp, g) if with_pool else (g.double(), g.double().abs())
        ref = R.bn_bwd(g_eff, y, scale, shift, mean, invstd, g_eff_abs)
        part, dgam, dbet, coef = Out((nblk * C * 2,)), Out((C,)), Out((C,)), Out((3 * C,), torch.float64)
        dy = act_out(B, H, W, C, hs)
        dg_in = dev(g, hs)
        L.call("sifsr_bn_relu_bwd", dg_in, dy_, *dv, C, npix, part.t, nblk, dgam.t, dbet.t, coef.t, dy.t, dgp if with_pool else None, H, W, S())
        torch.cuda.synchronize()
        assert torch.equal(raw_bits(dg_in), raw_bits(dev(g, hs)))                          # g is an input here
        note("bn_bwd:dy", hs, R.check(host(dy.ok(what)), ref["dy"], ref["dy_abs"], R.K["bn_bwd_dy"], hs, what))
        note("bn_bwd:dgamma", hs, R.check_sum(dgam.ok(what).cpu(), ref["dgamma"], ref["dgamma_abs"], R.BAR_TOL, (what, "dgamma")))
        note("bn_bwd:dbeta", hs, R.check_sum(dbet.ok(what).cpu(), ref["dbeta"], ref["dbeta_abs"], R.BAR_TOL, (what, "dbeta")))
        check_coef(L, hs, part.ok(what), nblk, C, npix, scale, shift, mean, invstd, None, coef.ok(what), None, what)
        if not with_coef:
            continue
        # the statistics half alone; with gpool it completes g in place (one rounding in bf16) and sums the STORED values
        what = ("bn_relu_bwd_coef",) + what[1:]
        part, dgam, dbet, coef, coef_f = Out((nblk * C * 2,)), Out((C,)), Out((C,)), Out((3 * C,), torch.float64), Out((4 * C,))
        gio = act_out(B, H, W, C, hs, init=g)
        L.call("sifsr_bn_relu_bwd_coef", gio.t, dy_, *dv, beta.cuda(), C, npix, part.t, nblk, dgam.t, dbet.t, coef.t, coef_f.t,
               dgp if with_pool else None, H, W, S())
        torch.cuda.synchronize()
        g_st = host(gio.ok(what))
        if with_pool:
            note("bn_bwd:g_completed", hs, R.check(g_st, g_eff, g_eff_abs, R.K["g_complete"], hs, (what, "completed g")))
        else:
            assert torch.equal(g_st, g)
        ref2 = R.bn_bwd(g_st, y, scale, shift, mean, invstd)
        note("bn_bwd:dgamma", hs, R.check_sum(dgam.ok(what).cpu(), ref2["dgamma"], ref2["dgamma_abs"], R.BAR_TOL, (what, "dgamma")))
        note("bn_bwd:dbeta", hs, R.check_sum(dbet.ok(what).cpu(), ref2["dbeta"], ref2["dbeta_abs"], R.BAR_TOL, (what, "dbeta")))
        check_coef(L, hs, part.ok(what), nblk, C, npix, scale, shift, mean, invstd, beta, coef.ok(what), coef_f.ok(what), what)


@pytest.mark.parametrize("nblk", [1, 3, 64])
@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 6, 10), (2, 18, 34)])
@pytest.mark.parametrize("C", [16, 32, 64])
def test_bn_relu_bwd(L, hs, C, shape, nblk):
    """npix = 4 is below one pass of a workgroup for every C (16 / 32 / 64 pixels); nblk = 64 exceeds the pixels there, so most
    workgroups are empty and must still write zero partials"""
    B, H, W = shape
    run_bn_bwd(L, hs, B, C, H, W, nblk, np.random.RandomState(7 * C + H + nblk))


@pytest.mark.parametrize("C", [16, 32])
def test_bn_relu_bwd_past_the_apply_grid_cap(L, hs, C):
    """(1, 520, 520): at C = 16 the apply kernel launches 4225 workgroups; C = 32 is the size that passes its 8192-block cap
    (8450 blocks of 256 quads) and makes the grid-stride loop take a second step"""
    if C == 32:
        assert 520 * 520 * C // 4 > 8192 * 256
    run_bn_bwd(L, hs, 1, C, 520, 520, 64, np.random.RandomState(C), with_coef=False)


@pytest.mark.parametrize("nblk", [1, 255, 257, 2049])
@pytest.mark.parametrize("C", [16, 64])
def test_bn_finalize(L, sifsr, C, nblk):
    """fp32 only (no activation tensor): synthetic partial rows, float64 reference from the SAME float partials -- this tests the
    kernel, not the partial representation.  Channel 0 has |mean| / std = 50, channel 1 exactly zero variance."""
    L.call("sifsr_set_op_storage_bf16", 0)
    rs = np.random.RandomState(C + nblk)
    eps, mom = 1e-5, 0.1
    gamma, beta = chan(rs, C)
    for count in (1, 2, 2 * 18 * 34):
        m = rs.uniform(-2.0, 2.0, C)
        s = rs.uniform(0.3, 2.0, C)
        m[0], s[0] = 5.0, 0.1
        f = rs.uniform(0.5, 1.5, (nblk, 1))
        f /= f.sum()
        p = np.stack((count * m * f, count * (s * s + m * m) * f), 2).astype(np.float32)          # [nblk][C][2]
        cnt = np.zeros(nblk)
        cnt[rs.randint(0, nblk, 1)] = count                                                     # channel 1: every sample equals 2
        p[:, 1, 0], p[:, 1, 1] = 2.0 * cnt, 4.0 * cnt
        part = torch.from_numpy(p)
        S1, S2 = part.double()[:, :, 0].sum(0), part.double()[:, :, 1].sum(0)
        mean = S1 / count
        var = (S2 / count - mean * mean).clamp_min(0.0)
        assert float(var[1]) == 0.0 and abs(float(mean[0])) / float(var[0].sqrt()) > 40
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = gamma.double() * invstd
        shift_terms = (beta.double(), -mean * scale)
        unb = var * count / (count - 1.0) if count > 1 else var
        dpart = part.cuda()
        for with_running in (False, True):
            rm0, rv0 = torch.from_numpy(rs.standard_normal(C).astype(np.float32)), torch.from_numpy(rs.uniform(0.5, 2.0, C).astype(np.float32))
            rm, rv = Out((C,), init=rm0), Out((C,), init=rv0)
            o = [Out((C,)) for _ in range(4)]
            L.call("sifsr_bn_finalize", dpart, nblk, C, float(count), gamma.cuda(), beta.cuda(), rm.t if with_running else None,
                   rv.t if with_running else None, mom, eps, o[0].t, o[1].t, o[2].t, o[3].t, S())
            torch.cuda.synchronize()
            what = ("bn_finalize", C, nblk, count, with_running)
            g_mean, g_invstd, g_scale, g_shift = [t.ok(what).cpu() for t in o]
            note("bn_finalize", False, R.check_sum(g_mean, mean, mean.abs(), 1e-6, (what, "mean")))
            cancel = 1.0 + mean * mean / (var + eps)                  # (var + eps: what is under the root; never above 1 + mean^2/var)
            note("bn_finalize", False, R.check_sum(g_invstd, invstd, invstd * cancel, 1e-6, (what, "invstd")))
            note("bn_finalize", False, R.check_sum(g_scale, scale, scale.abs(), 1e-6, (what, "scale")))
            note("bn_finalize", False, R.check_sum(g_shift, shift_terms[0] + shift_terms[1], shift_terms[0].abs() + shift_terms[1].abs(), 1e-6, (what, "shift")))
            if with_running:
                rm_ref = (1.0 - mom) * rm0.double() + mom * mean
                rv_ref = (1.0 - mom) * rv0.double() + mom * unb
                note("bn_finalize", False, R.check_sum(rm.ok(what).cpu(), rm_ref, (1.0 - mom) * rm0.double().abs() + mom * mean.abs(), 1e-6, (what, "running_mean")))
                note("bn_finalize", False, R.check_sum(rv.ok(what).cpu(), rv_ref, rv_ref, 1e-6, (what, "running_var")))
            else:
                assert torch.equal(rm.ok(what).cpu(), rm0) and torch.equal(rv.ok(what).cpu(), rv0)


# ------------------------------------------------------------------------------------------------ thin convs, head, tail
THIN_SHAPES = [(1, 1, 1), (2, 1, 7), (2, 2, 3), (1, 3, 3), (1, 8, 8), (2, 17, 33)]


def ntiles(B, H, W):
    return B * ((H + 15) // 16) * ((W + 15) // 16)


@pytest.mark.parametrize("shape", THIN_SHAPES)
def test_conv_in_and_head(L, hs, shape):
    B, H, W = shape
    rs = np.random.RandomState(31 * H + W + B)
    x = torch.from_numpy(rs.standard_normal((B, 2, H, W)).astype(np.float32))                  # the model input stays fp32 NCHW
    w = torch.from_numpy((0.3 * rs.standard_normal((16, 2, 3, 3))).astype(np.float32))
    dx, dw_ = x.cuda(), w.cuda()
    # forward with statistics
    blocks = L.call("sifsr_conv_in_stat_blocks", B, H, W)
    assert blocks == min(ntiles(B, H, W), 2048)
    y_o, part = act_out(B, H, W, 16, hs), Out((blocks, 16, 2))
    L.call("sifsr_conv_in_fwd", dx, dw_, y_o.t, part.t, B, H, W, S())
    ref, ref_abs = R.with_abs(R.conv3_rep, x, w)
    y_st = host(y_o.ok("conv_in_fwd"))
    note("conv_in:fwd", hs, R.check(y_st, ref, ref_abs, R.K["conv_in_fwd"], hs, ("conv_in_fwd", shape)))
    st = part.ok("conv_in stats").double().cpu().sum(0)                                          # of the STORED values
    ys = y_st.double()
    note("conv_in:stats", hs, R.check_sum(st, torch.stack((ys.sum((0, 2, 3)), (ys * ys).sum((0, 2, 3))), 1),
                                          torch.stack((R.sum_abs(ys), R.sum_abs(ys, ys)), 1), R.BAR_SUM, ("conv_in stats", shape)))
    # BatchNorm of that layer, from the stored y
    gamma, beta = chan(rs, 16)
    mean = ys.mean((0, 2, 3)).float()
    invstd = (1.0 / torch.sqrt(ys.var((0, 2, 3), unbiased=False) + 1e-5)).float()
    scale = gamma * invstd
    shift = beta - mean * scale
    g = vals(rs, (B, 16, H, W), hs)
    dyv = vals(rs, (B, 16, H, W), hs)
    bn = R.bn_bwd(g, y_st, scale, shift, mean, invstd)
    dz = R.stored(bn["dz"].float(), hs)                                                          # (a masked copy of g: exact in either mode)
    assert torch.equal(dz.double(), bn["dz"])
    y_lin, y_lin_abs = ref, ref_abs                                                             # the linear form takes y = W p itself
    sd, k1, k0 = [bn["coef"][i * 16:(i + 1) * 16].view(1, -1, 1, 1) for i in range(3)]
    dy_lin, dy_lin_abs = sd * bn["dz"] + k1 * y_lin + k0, sd.abs() * bn["dz"].abs() + k1.abs() * y_lin_abs + k0.abs()
    dv = [t.cuda() for t in (scale, shift, mean, invstd)]
    for nblk in (1, 3, ntiles(B, H, W) + 5):
        what = ("conv_in", shape, nblk)
        scratch, dw = Out((nblk * 288,)), Out((16, 2, 3, 3))
        L.call("sifsr_conv_in_wgrad", dx, dev(dyv, hs), scratch.t, nblk, dw.t, B, H, W, S())
        r, ra = R.with_abs(R.conv3_rep_wgrad, x, dyv)
        scratch.ok(what)
        note("conv_in:wgrad", hs, R.check_sum(dw.ok(what).cpu(), r, ra, R.BAR_SUM, (what, "wgrad")))
        scratch, dw, dgam, dbet, coef = Out((nblk * 288,)), Out((16, 2, 3, 3)), Out((16,)), Out((16,)), Out((48,), torch.float64)
        L.call("sifsr_conv_in_bn_relu_bwd", dx, dev(g, hs), dev(y_st, hs), *dv, scratch.t, nblk, dw.t, dgam.t, dbet.t, coef.t, B, H, W, S())
        scratch.ok(what)
        note("conv_in:head dgamma", hs, R.check_sum(dgam.ok(what).cpu(), bn["dgamma"], bn["dgamma_abs"], R.BAR_TOL, (what, "dgamma")))
        note("conv_in:head dbeta", hs, R.check_sum(dbet.ok(what).cpu(), bn["dbeta"], bn["dbeta_abs"], R.BAR_TOL, (what, "dbeta")))
        note("conv_in:head coef", hs, R.check_sum(coef.ok(what).cpu(), bn["coef"], bn["coef_abs"], R.BAR_TOL, (what, "coef")))
        note("conv_in:head dw", hs, R.check_sum(dw.ok(what).cpu(), R.conv3_rep_wgrad(x, bn["dy"]), R.conv3_rep_wgrad(x.abs(), bn["dy_abs"]),
                                                R.BAR_SUM, (what, "head dw")))
        scratch, dw = Out((L.call("sifsr_conv_in_bwd_linear_scratch_floats", nblk),)), Out((16, 2, 3, 3))
        L.call("sifsr_conv_in_bwd_linear", dx, dev(dz, hs), dw_, bn["coef"].cuda(), scratch.t, nblk, dw.t, B, H, W, S())
        scratch.ok(what)
        note("conv_in:bwd_linear", hs, R.check_sum(dw.ok(what).cpu(), R.conv3_rep_wgrad(x, dy_lin), R.conv3_rep_wgrad(x.abs(), dy_lin_abs),
                                                   R.BAR_SUM, (what, "bwd_linear dw")))


@pytest.mark.parametrize("shape", THIN_SHAPES)
def test_conv_out_and_tail(L, hs, shape):
    B, H, W = shape
    rs = np.random.RandomState(17 * H + W + B)
    y = vals(rs, (B, 16, H, W), hs, 1.5, 0.7)
    gamma, beta = chan(rs, 16)
    mean = y.double().mean((0, 2, 3)).float()
    invstd = (1.0 / torch.sqrt(y.double().var((0, 2, 3), unbiased=False) + 1e-5)).float()
    scale = gamma * invstd
    shift = beta - mean * scale
    w = torch.from_numpy((0.2 * rs.standard_normal((1, 16, 3, 3))).astype(np.float32))
    bias = torch.tensor([0.1])
    dsr = torch.from_numpy(rs.standard_normal((B, 1, H, W)).astype(np.float32))                # sr and dsr stay fp32 NCHW
    dy_, dw_, ddsr = dev(y, hs), w.cuda(), dsr.cuda()
    dv = [t.cuda() for t in (scale, shift, mean, invstd)]
    for with_bn in (True, False):
        a, a_abs = R.bnrelu(y, scale if with_bn else None, shift if with_bn else None)
        sr = Out((B, 1, H, W))
        L.call("sifsr_conv_out_fwd", dy_, dv[0] if with_bn else None, dv[1] if with_bn else None, dw_, bias.cuda(), sr.t, B, H, W, S())
        note("conv_out:fwd", hs, R.check(sr.ok("conv_out_fwd").cpu(), R.conv3_rep(a, w, bias), R.conv3_rep(a_abs, w.abs(), bias.abs()),
                                         R.K["conv_out_fwd"], False, ("conv_out_fwd", shape, with_bn)))
    a, a_abs = R.bnrelu(y, scale, shift)
    g_o = act_out(B, H, W, 16, hs)
    L.call("sifsr_conv_out_dgrad", ddsr, dw_, g_o.t, B, H, W, S())
    g_ref, g_abs = R.with_abs(R.conv3_rep_dgrad, dsr, w)
    note("conv_out:dgrad", hs, R.check(host(g_o.ok("conv_out_dgrad")), g_ref, g_abs, R.K["conv_out_dgrad"], hs, ("conv_out_dgrad", shape)))
    dwb_ref = torch.cat((R.conv3_rep_wgrad(a, dsr).flatten(), dsr.double().sum().view(1)))
    dwb_abs = torch.cat((R.conv3_rep_wgrad(a_abs, dsr.abs()).flatten(), dsr.double().abs().sum().view(1)))
    bn = R.bn_bwd(g_ref, y, scale, shift, mean, invstd, g_abs)
    for nblk in (1, 3, ntiles(B, H, W) + 5):
        what = ("conv_out", shape, nblk)
        scratch, dwb = Out((nblk * 145,)), Out((145,))
        L.call("sifsr_conv_out_wgrad", dy_, dv[0], dv[1], ddsr, scratch.t, nblk, dwb.t, B, H, W, S())
        scratch.ok(what)
        note("conv_out:wgrad", hs, R.check_sum(dwb.ok(what).cpu(), dwb_ref, dwb_abs, R.BAR_SUM, (what, "wgrad")))
        # the fused tail: H, W >= 3, the shape error (and no launch) otherwise
        scratch = Out((2 * ((nblk * 145 + 63) // 64 * 64) + nblk * 64,))
        dwb, dgam, dbet, coef, dy = Out((145,)), Out((16,)), Out((16,)), Out((48,), torch.float64), act_out(B, H, W, 16, hs)
        args = (dy_, *dv, ddsr, dw_, scratch.t, nblk, dwb.t, dgam.t, dbet.t, coef.t, dy.t, B, H, W, S())
        if H < 3 or W < 3:
            rc = L.lib().sifsr_conv_out_bn_relu_bwd(*[t.data_ptr() if isinstance(t, torch.Tensor) else t for t in args])
            torch.cuda.synchronize()
            assert rc == ERR_SHAPE, rc
            for o in (scratch, dwb, dgam, dbet, coef, dy):
                assert bool(torch.isnan(o.ok(what).float()).all()), (what, "something was launched")
            continue
        L.call("sifsr_conv_out_bn_relu_bwd", *args)
        scratch.ok(what)
        note("tail:dwb", hs, R.check_sum(dwb.ok(what).cpu(), dwb_ref, dwb_abs, R.BAR_SUM, (what, "tail dwb")))
        note("tail:dgamma", hs, R.check_sum(dgam.ok(what).cpu(), bn["dgamma"], bn["dgamma_abs"], R.BAR_TOL, (what, "tail dgamma")))
        note("tail:dbeta", hs, R.check_sum(dbet.ok(what).cpu(), bn["dbeta"], bn["dbeta_abs"], R.BAR_TOL, (what, "tail dbeta")))
        note("tail:coef", hs, R.check_sum(coef.ok(what).cpu(), bn["coef"], bn["coef_abs"], R.BAR_TOL, (what, "tail coef")))
        note("tail:dy", hs, R.check(host(dy.ok(what)), bn["dy"], bn["dy_abs"], R.K["tail_dy"], hs, (what, "tail dy")))
