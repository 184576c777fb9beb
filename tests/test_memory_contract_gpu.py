"""GPU: the MEMORY contract of every C-ABI operator (include/sifsr_hip.h).  The values are pinned elsewhere (tests/test_ops_gpu.py
and friends, float64 autograd at 1e-4); here every pointer argument comes out of a guarded arena (tests/memcheck.py) and each
case runs under the three poisons:

  * no byte outside an output / scratch buffer of exactly the size the header or its size query states is written (1 MiB guards),
  * no `const` input changes (the one documented in-place update, g of sifsr_bn_relu_bwd_coef with a pooled gradient, is asserted bit for bit),
  * every output -- statistic partials rows included, and the result reduced from every scratch -- is bit-identical whether the
    written buffers held zeros, NaN or N(0,1) values before the call, and NaN-free: nothing reads what this call did not write,
  * the same call on ordinary allocations gives the same bits (carving cannot change which path runs).

Nothing takes a tolerance.  The operands are random but well-scaled: the contract does not depend on them being a consistent
forward state.  CONTRACT is also the coverage table tests/test_capi_gate.py checks against the header."""
import numpy as np
import pytest
import torch

from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import Partial, bit_equal

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ENGINE_ENTRY_POINTS = ("sifsr_model_forward", "sifsr_model_backward", "sifsr_model_forward_ex", "sifsr_model_backward_ex")


_PACKS = {}


def packs(L, cin, cout):
    """real fragment packs of a seeded weight (the bf16 halves of wdgrad must hold bf16 values, not fp32 mantissa bits)"""
    if (cin, cout) not in _PACKS:
        rs = np.random.RandomState(1000 * cin + cout)
        w = torch.from_numpy((rs.standard_normal((cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32))
        n = 9 * cin * cout
        wf, wd = torch.zeros(n, device="cuda"), torch.zeros(4 * n, device="cuda")
        wwf, wwd = torch.zeros(16 * cin * cout, device="cuda"), torch.zeros(16 * cin * cout, device="cuda")
        L.call("sifsr_pack_conv_weights", w.cuda(), cin, cout, wf, wd, S())
        L.call("sifsr_pack_conv_weights_wino", w.cuda(), cin, cout, wwf, wwd, S())
        torch.cuda.synchronize()
        _PACKS[(cin, cout)] = (w, wf.cpu(), wd.cpu(), wwf.cpu(), wwd.cpu())
    return _PACKS[(cin, cout)]


def bf16_storage(L, fn):
    def call():
        L.call("sifsr_set_op_storage_bf16", 1)
        try:
            fn()
        finally:
            L.call("sifsr_set_op_storage_bf16", 0)
    return call


# ---- 3x3 convolutions ---------------------------------------------------------------------------------------------------
# (C0, C1, cout, H, W, B): the smallest image the conv tests use, partial 16x16 tiles in both directions, the two-source
# (concat) forms, and one layer-sized problem (16 -> 16 at 128 x 128, batch 8)
CONV_SHAPES = [(64, 0, 64, 4, 6, 2), (64, 64, 64, 12, 20, 2), (16, 16, 16, 12, 20, 2), (16, 0, 32, 20, 36, 1),
               (32, 0, 32, 24, 40, 2), (16, 0, 16, 128, 128, 8)]


def _srcs(k, shp, dtype=F32):
    C0, C1, cout, H, W, B = shp
    a0 = C1 == 0 or C0 == 16
    src0 = k.i("src0", B, H, W, C0, dtype=dtype)
    sc0, sh0 = (k.pos("scale0", C0), k.i("shift0", C0, scale=0.3)) if a0 else (None, None)
    src1 = k.i("src1", B, H, W, C1, dtype=dtype) if C1 else None
    sc1, sh1 = (k.pos("scale1", C1), k.i("shift1", C1, scale=0.3)) if C1 else (None, None)
    return (src0, C0, sc0, sh0, src1, C1, sc1, sh1)


def conv_fwd(kind):
    def make(shp):
        def case(k):
            L = k.L
            C0, C1, cout, H, W, B = shp
            cin = C0 + C1
            _, wf, wd, wwf, _ = packs(L, cin, cout)
            dt = BF16 if kind == "bf16" else F32
            src = _srcs(k, shp, dt)
            y = k.o("y", B, H, W, cout, dtype=dt)
            if kind == "wino":
                nblk = L.call("sifsr_conv3x3_stat_blocks_wino", B, H, W, cin, cout)
            else:
                nblk = L.call("sifsr_conv3x3_stat_blocks", B, H, W, cout)
            part = k.o("stat_partials", nblk, cout, 2)
            if kind == "tap":
                w_ = k.t("wfwd", wf)
                call = lambda: L.call("sifsr_conv3x3_fwd", *src, w_, y, cout, part, B, H, W, S())
            elif kind == "wino":
                w_, ww_ = k.t("wfwd", wf), k.t("wwf", wwf)
                call = lambda: L.call("sifsr_conv3x3_fwd_wino", *src, w_, ww_, y, cout, part, B, H, W, S())
            else:
                w_ = k.t("wdgrad", wd)
                call = lambda: L.call("sifsr_conv3x3_fwd_bf16", *src, w_, y, cout, part, B, H, W, S())
            return call, {"y": y, "stat_partials": part}
        return case
    return [make(s) for s in CONV_SHAPES]


def conv_dgrad(kind):
    def make(shp, with_add):
        def case(k):
            L = k.L
            C0, C1, cout, H, W, B = shp
            cin = C0 + C1
            w, _, wd, _, wwd = packs(L, cin, cout)
            dt = BF16 if kind == "bf16" else F32
            dy = k.i("dy", B, H, W, cout, dtype=dt)
            wd_ = k.t("wdgrad", wd)
            g0 = k.o("g0", B, H, W, C0, dtype=dt)
            g1 = k.o("g1", B, H, W, C1, dtype=dt) if C1 else None
            add = k.i("addend", B, H, W, cin, dtype=dt) if with_add else None
            if kind == "tap":
                w_ = k.t("w_oihw", w)
                call = lambda: L.call("sifsr_conv3x3_dgrad", dy, cout, wd_, w_, cin, g0, C0, g1, C1, add, B, H, W, S())
            elif kind == "wino":
                ww_ = k.t("wwd", wwd)
                call = lambda: L.call("sifsr_conv3x3_dgrad_wino", dy, cout, wd_, ww_, cin, g0, C0, g1, C1, add, B, H, W, S())
            else:
                call = lambda: L.call("sifsr_conv3x3_dgrad_bf16", dy, cout, wd_, cin, g0, C0, g1, C1, add, B, H, W, S())
            outs = {"g0": g0}
            if C1:
                outs["g1"] = g1
            return call, outs
        return case
    return [make(s, False) for s in CONV_SHAPES] + [make(s, True) for s in CONV_SHAPES if s[1] == 0][:3]


def _coef_f(k, cout):
    c = torch.cat([torch.from_numpy(k.rs.uniform(0.5, 1.5, cout).astype(np.float32)),
                   torch.from_numpy((k.rs.standard_normal(3 * cout) * 0.3).astype(np.float32))])
    return k.t("coef_f", c)


FUSED_SHAPES = [(16, 16, 32, 48, 2), (32, 16, 24, 40, 2), (64, 64, 12, 20, 2), (16, 16, 20, 36, 1), (128, 64, 16, 16, 1)]


def conv_dgrad_fused():
    def make(shp, wino, with_add):
        def case(k):
            L = k.L
            cin, cout, H, W, B = shp
            _, _, wd, _, wwd = packs(L, cin, cout)
            g, y = k.i("g", B, H, W, cout), k.i("y", B, H, W, cout)
            cf, wd_ = _coef_f(k, cout), k.t("wdgrad", wd)
            ww_ = k.t("wwd", wwd) if wino else None
            gin = k.o("g0", B, H, W, cin)
            add = k.i("addend", B, H, W, cin) if with_add else None
            border, bres = k.border("border", B, H, W, cout)
            call = lambda: L.call("sifsr_conv3x3_dgrad_fused", g, y, cf, cout, wd_, ww_, cin, gin, cin, None, 0, add, border,
                                  B, H, W, S())
            return call, {"g0": gin, "border": bres}
        return case
    return [make(s, w, a) for s in FUSED_SHAPES for w, a in ((False, False), (True, False))] + [make(FUSED_SHAPES[0], True, True)]


# more workgroups than tiles (nblk 64 and 97 on a 16 x 16 image), one workgroup, a count that divides nothing, partial tiles, concat
WGRAD_CASES = [((16, 0, 32, 16, 16, 1), (1, 64, 97)), ((64, 64, 64, 12, 20, 2), (7, 64)), ((16, 16, 16, 12, 20, 2), (1, 7)),
               ((32, 0, 32, 24, 40, 2), (7, 97)), ((64, 0, 64, 4, 6, 2), (64,)), ((16, 0, 16, 128, 128, 8), (97,))]


def conv_wgrad(kind):
    def make(shp, nb):
        def case(k):
            L = k.L
            C0, C1, cout, H, W, B = shp
            cin = C0 + C1
            dt = BF16 if kind == "bf16" else F32
            src = _srcs(k, shp, dt)
            dy = k.i("dy" if kind in ("tap", "bf16", "wino") else "g", B, H, W, cout, dtype=dt)
            fused = kind in ("fused", "wino_fused")
            y, cf = (k.i("y", B, H, W, cout), _coef_f(k, cout)) if fused else (None, None)
            q = "sifsr_conv3x3_wgrad_wino_scratch_floats" if kind.startswith("wino") else "sifsr_conv3x3_wgrad_scratch_floats"
            scratch = k.s("scratch", L.call(q, cin, cout, nb))
            dw = k.o("dw", cout, cin, 3, 3)
            if kind == "tap":
                call = lambda: L.call("sifsr_conv3x3_wgrad", *src, dy, cout, scratch, nb, dw, B, H, W, S())
            elif kind == "bf16":
                call = lambda: L.call("sifsr_conv3x3_wgrad_bf16", *src, dy, cout, scratch, nb, dw, B, H, W, S())
            elif kind == "fused":
                call = lambda: L.call("sifsr_conv3x3_wgrad_fused", *src, dy, y, cf, cout, scratch, nb, dw, B, H, W, S())
            else:
                call = lambda: L.call("sifsr_conv3x3_wgrad_wino", *src, dy, y, cf, cout, scratch, nb, dw, B, H, W, S())
            return call, {"dw": dw}
        return case
    return [make(s, nb) for s, nbs in WGRAD_CASES for nb in nbs]


# ---- the fused 16 -> 16 backward (conv_bwd16.hip): (H, W, B, x_bn, dy formed from (g, y), addend, BatchNorm sums) ---------------
BWD16_CASES = [(32, 48, 2, True, True, False, True), (32, 32, 1, True, False, False, True), (48, 32, 2, False, True, True, False),
               (128, 128, 8, True, True, False, True), (64, 32, 3, False, False, False, False), (32, 32, 1, True, True, False, False)]


def _bwd16_common(k, H, W, B, x_bn, dt=F32):
    L = k.L
    _, _, wd, _, wwd = packs(L, 16, 16)
    x = k.i("x", B, H, W, 16, dtype=dt)
    xs, xsh = (k.pos("x_scale", 16), k.i("x_shift", 16, scale=0.3)) if x_bn else (None, None)
    rows = L.call("sifsr_conv3x3_bwd16_stat_rows", B, H, W)
    assert rows > 0
    nscr = L.call("sifsr_conv3x3_bwd16_scratch_floats", B, H, W)
    return x, xs, xsh, k.t("wdgrad", wd), k.t("wwd", wwd), rows, nscr


def conv_bwd16(storage_bf16=False):
    def make(c):
        def case(k):
            L = k.L
            H, W, B, x_bn, dyf, with_add, with_stats = c
            dt = BF16 if storage_bf16 else F32
            x, xs, xsh, wd_, ww_, rows, nscr = _bwd16_common(k, H, W, B, x_bn, dt)
            g = k.i("g", B, H, W, 16, dtype=dt)
            outs = {}
            if dyf:
                y, cf = k.i("y", B, H, W, 16, dtype=dt), _coef_f(k, 16)
                border, bres = k.border("border", B, H, W, 16, dtype=dt)
                outs["border"] = bres
            else:
                y = cf = border = None
            gin = k.o("gin", B, H, W, 16, dtype=dt)
            add = k.i("addend", B, H, W, 16, dtype=dt) if with_add else None
            bnp = k.o("bn_partials", rows, 16, 2) if with_stats else None
            scratch, dw = k.s("scratch", nscr), k.o("dw", 16, 16, 3, 3)
            st = (x, xs, xsh) if with_stats else (None, None, None)
            call = lambda: L.call("sifsr_conv3x3_bwd16", x, xs, xsh, g, y, cf, border, wd_, ww_, gin, add, *st, bnp, scratch, dw,
                                  B, H, W, S())
            outs.update({"gin": gin, "dw": dw})
            if with_stats:
                outs["bn_partials"] = bnp
            return (bf16_storage(L, call) if storage_bf16 else call), outs
        return case
    cases = BWD16_CASES if not storage_bf16 else [BWD16_CASES[0], BWD16_CASES[4]]
    return [make(c) for c in cases]


def conv_bwd16_variant(which):
    def make(H, W, B, with_stats, bf=False):
        def case(k):
            L = k.L
            dt = BF16 if bf else F32
            x, xs, xsh, wd_, ww_, rows, nscr = _bwd16_common(k, H, W, B, True, dt)
            if which == "pool":
                g, gp = k.i("g", B, H, W, 16, dtype=dt), k.i("pool_gp", B, H // 2, W // 2, 16, dtype=dt)
            else:
                dsr, w_out = k.i("dsr", B, H, W), k.i("w_out", 1, 16, 3, 3, scale=0.2)      # fp32 in every storage mode
            y, cf = k.i("y", B, H, W, 16, dtype=dt), _coef_f(k, 16)
            border, bres = k.border("border", B, H, W, 16, dtype=dt)
            gin = k.o("gin", B, H, W, 16, dtype=dt)
            bnp = k.o("bn_partials", rows, 16, 2) if with_stats else None
            scratch, dw = k.s("scratch", nscr), k.o("dw", 16, 16, 3, 3)
            st = (x, xs, xsh) if with_stats else (None, None, None)
            if which == "pool":
                call = lambda: L.call("sifsr_conv3x3_bwd16_pool", x, xs, xsh, g, gp, y, cf, border, wd_, ww_, gin, *st, bnp, scratch,
                                      dw, B, H, W, S())
            else:
                call = lambda: L.call("sifsr_conv3x3_bwd16_tail", x, xs, xsh, dsr, w_out, y, cf, border, wd_, ww_, gin, *st, bnp,
                                      scratch, dw, B, H, W, S())
            outs = {"gin": gin, "dw": dw, "border": bres}
            if with_stats:
                outs["bn_partials"] = bnp
            return (bf16_storage(L, call) if bf else call), outs
        return case
    return [make(32, 48, 2, True), make(48, 32, 3, False), make(128, 128, 8, True), make(32, 48, 2, True, bf=True),
            make(48, 32, 3, False, bf=True)]


# ---- thin first / last convolutions and the fused head / tail (edge_conv.hip, fused_edges.hip) ----------------------------------
EDGE_SHAPES = [(1, 16, 16), (2, 24, 40), (2, 40, 24), (2, 32, 48)]


def conv_in_fwd():
    def make(B, H, W, bf):
        def case(k):
            L = k.L
            x, w = k.i("x", B, 2, H, W), k.i("w", 16, 2, 3, 3, scale=0.3)
            y = k.o("y", B, H, W, 16, dtype=BF16 if bf else F32)
            part = k.o("stat_partials", L.call("sifsr_conv_in_stat_blocks", B, H, W), 16, 2)
            call = lambda: L.call("sifsr_conv_in_fwd", x, w, y, part, B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"y": y, "stat_partials": part}
        return case
    return [make(*s, False) for s in EDGE_SHAPES] + [make(2, 24, 40, True)]


def conv_in_wgrad():
    def make(B, H, W, nb, bf=False):
        def case(k):
            L = k.L
            x, dy = k.i("x", B, 2, H, W), k.i("dy", B, H, W, 16, dtype=BF16 if bf else F32)
            scratch, dw = k.s("scratch", nb * 288), k.o("dw", 16, 2, 3, 3)
            call = lambda: L.call("sifsr_conv_in_wgrad", x, dy, scratch, nb, dw, B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"dw": dw}
        return case
    return [make(1, 16, 16, 64), make(2, 24, 40, 5), make(2, 40, 24, 1), make(2, 32, 48, 97), make(2, 24, 40, 5, bf=True)]


def conv_out_fwd():
    def make(B, H, W, bf):
        def case(k):
            L = k.L
            y = k.i("y", B, H, W, 16, dtype=BF16 if bf else F32)
            sc, sh, w, b = k.pos("scale", 16), k.i("shift", 16, scale=0.3), k.i("w", 1, 16, 3, 3, scale=0.2), k.i("bias", 1)
            sr = k.o("sr", B, 1, H, W)
            call = lambda: L.call("sifsr_conv_out_fwd", y, sc, sh, w, b, sr, B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"sr": sr}
        return case
    return [make(*s, False) for s in EDGE_SHAPES] + [make(2, 24, 40, True)]


def conv_out_dgrad():
    def make(B, H, W, bf=False):
        def case(k):
            L = k.L
            dsr, w = k.i("dsr", B, 1, H, W), k.i("w", 1, 16, 3, 3, scale=0.2)
            g = k.o("g", B, H, W, 16, dtype=BF16 if bf else F32)
            call = lambda: L.call("sifsr_conv_out_dgrad", dsr, w, g, B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"g": g}
        return case
    return [make(*s) for s in EDGE_SHAPES] + [make(2, 24, 40, bf=True), make(1, 16, 16, bf=True)]


def conv_out_wgrad():
    def make(B, H, W, nb, bf=False):
        def case(k):
            L = k.L
            y, sc, sh = k.i("y", B, H, W, 16, dtype=BF16 if bf else F32), k.pos("scale", 16), k.i("shift", 16, scale=0.3)
            dsr = k.i("dsr", B, 1, H, W)
            scratch, dwb = k.s("scratch", nb * 145), k.o("dwb", 145)
            call = lambda: L.call("sifsr_conv_out_wgrad", y, sc, sh, dsr, scratch, nb, dwb, B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"dwb": dwb}
        return case
    return [make(1, 16, 16, 64), make(2, 24, 40, 5), make(2, 40, 24, 1), make(2, 32, 48, 97), make(2, 24, 40, 5, bf=True)]


def _bn_vecs(k, C):
    return k.pos("scale", C), k.i("shift", C, scale=0.3), k.i("mean", C, scale=0.3), k.pos("invstd", C)


def conv_out_bn_relu_bwd():
    def make(B, H, W, nb, bf):
        def case(k):
            L = k.L
            dt = BF16 if bf else F32
            y = k.i("y", B, H, W, 16, dtype=dt)
            sc, sh, mean, inv = _bn_vecs(k, 16)
            dsr, w = k.i("dsr", B, 1, H, W), k.i("w", 1, 16, 3, 3, scale=0.2)
            scratch = k.s("scratch", 64 + nb * (145 + 32))          # the size the header states
            dwb, dgam, dbet = k.o("dwb", 145), k.o("dgamma", 16), k.o("dbeta", 16)
            coef, dy = k.o("coef", 48, dtype=F64), k.o("dy", B, H, W, 16, dtype=dt)
            call = lambda: L.call("sifsr_conv_out_bn_relu_bwd", y, sc, sh, mean, inv, dsr, w, scratch, nb, dwb, dgam, dbet, coef, dy,
                                  B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"dwb": dwb, "dgamma": dgam, "dbeta": dbet, "coef": coef, "dy": dy}
        return case
    return [make(1, 16, 16, 64, False), make(2, 24, 40, 3, False), make(1, 19, 37, 6, False), make(3, 64, 32, 1, False),
            make(2, 32, 48, 97, False), make(2, 32, 48, 12, True)]


def conv_in_bn_relu_bwd():
    def make(B, H, W, nb, bf=False):
        def case(k):
            L = k.L
            dt = BF16 if bf else F32
            x, g, y = k.i("x", B, 2, H, W), k.i("g", B, H, W, 16, dtype=dt), k.i("y", B, H, W, 16, dtype=dt)
            sc, sh, mean, inv = _bn_vecs(k, 16)
            scratch = k.s("scratch", nb * 288)
            dw, dgam, dbet, coef = k.o("dw", 16, 2, 3, 3), k.o("dgamma", 16), k.o("dbeta", 16), k.o("coef", 48, dtype=F64)
            call = lambda: L.call("sifsr_conv_in_bn_relu_bwd", x, g, y, sc, sh, mean, inv, scratch, nb, dw, dgam, dbet, coef, B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"dw": dw, "dgamma": dgam, "dbeta": dbet, "coef": coef}
        return case
    return [make(1, 16, 16, 64), make(2, 24, 40, 3), make(2, 32, 48, 1), make(8, 128, 128, 97), make(2, 24, 40, 3, bf=True)]


def conv_in_bwd_linear():
    def make(B, H, W, nb, bf=False):
        def case(k):
            L = k.L
            x, dz = k.i("x", B, 2, H, W), k.i("dz", B, H, W, 16, dtype=BF16 if bf else F32)
            w, coef = k.i("w", 16, 2, 3, 3, scale=0.3), k.i("coef", 48, dtype=F64)
            scratch = k.s("scratch", L.call("sifsr_conv_in_bwd_linear_scratch_floats", nb))
            dw = k.o("dw", 16, 2, 3, 3)
            call = lambda: L.call("sifsr_conv_in_bwd_linear", x, dz, w, coef, scratch, nb, dw, B, H, W, S())
            return (bf16_storage(L, call) if bf else call), {"dw": dw}
        return case
    return [make(1, 16, 16, 64), make(2, 24, 40, 3), make(2, 32, 48, 1), make(8, 128, 128, 97), make(2, 24, 40, 3, bf=True)]


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------
def bn_finalize():
    def make(C, nb, with_running):
        def case(k):
            L = k.L
            p = torch.from_numpy(k.rs.standard_normal((nb, C, 2)).astype(np.float32))
            p[:, :, 1] = p[:, :, 1].abs() * 300 + 300                # sum of squares well above (sum)^2 / count
            part = k.t("stat_partials", p)
            gamma, beta = k.pos("gamma", C), k.i("beta", C, scale=0.2)
            rm = k.A.inout(torch.zeros(C), "running_mean") if with_running else None
            rv = k.A.inout(torch.ones(C), "running_var") if with_running else None
            mean, inv, sc, sh = k.o("mean", C), k.o("invstd", C), k.o("scale", C), k.o("shift", C)
            call = lambda: L.call("sifsr_bn_finalize", part, nb, C, 256.0 * nb, gamma, beta, rm, rv, 0.1, 1e-5, mean, inv, sc, sh, S())
            outs = {"mean": mean, "invstd": inv, "scale": sc, "shift": sh}
            if with_running:
                outs.update({"running_mean": rm, "running_var": rv})
            return call, outs
        return case
    return [make(16, 1, True), make(32, 7, True), make(64, 97, False), make(16, 2048, True)]


def bn_relu_bwd(coef_form):
    def make(C, B, H, W, nb, pool, bf=False):
        def case(k):
            L = k.L
            dt = BF16 if bf else F32
            npix = B * H * W
            gt = torch.from_numpy(k.rs.standard_normal((B, H, W, C)).astype(np.float32)).to(dt)
            y = k.i("y", B, H, W, C, dtype=dt)
            sc, sh, mean, inv = _bn_vecs(k, C)
            gp = k.i("gpool", B, H // 2, W // 2, C, dtype=dt) if pool else None
            partials = k.s("partials", nb * C * 2)
            dgam, dbet, coef = k.o("dgamma", C), k.o("dbeta", C), k.o("coef", 3 * C, dtype=F64)
            outs = {"dgamma": dgam, "dbeta": dbet, "coef": coef}
            if coef_form:
                # documented: with a pooled gradient g is completed IN PLACE; without one it must come back unchanged
                g = k.A.inout(gt, "g") if pool else k.A.input(gt, "g")
                beta, cf = k.i("beta", C, scale=0.2), k.o("coef_f", 4 * C)
                call = lambda: L.call("sifsr_bn_relu_bwd_coef", g, y, sc, sh, mean, inv, beta, C, npix, partials, nb, dgam, dbet, coef,
                                      cf, gp, H, W, S())
                outs["coef_f"] = cf
                if pool:
                    # g + 0.25 * gpool[y/2][x/2]: one fp32 multiply by a power of two and one add, then the storage rounding
                    want = (gt.float() + 0.25 * gp.cpu().float().repeat_interleave(2, 1).repeat_interleave(2, 2)).to(dt)
                    inner = call

                    def call():
                        inner()
                        torch.cuda.synchronize()
                        assert bit_equal(g.cpu(), want), "g was not completed in place to g + 0.25 * gpool[y/2][x/2]"
                    outs["g"] = g
            else:
                g = k.A.input(gt, "g")
                dy = k.o("dy", B, H, W, C, dtype=dt)
                call = lambda: L.call("sifsr_bn_relu_bwd", g, y, sc, sh, mean, inv, C, npix, partials, nb, dgam, dbet, coef, dy, gp,
                                      H if pool else 0, W if pool else 0, S())
                outs["dy"] = dy
            return (bf16_storage(L, call) if bf else call), outs
        return case
    return [make(16, 1, 16, 16, 64, False), make(16, 2, 32, 32, 8, True), make(32, 1, 12, 20, 1, True), make(64, 2, 12, 20, 7, False),
            make(16, 8, 128, 128, 97, True), make(32, 2, 16, 24, 3, True, bf=True)]


# ---- resampling ----------------------------------------------------------------------------------------------------------------
RES_SHAPES = [(16, 2, 16, 24), (64, 2, 4, 6), (32, 1, 64, 64), (16, 2, 36, 20), (8, 2, 16, 24)]


def resample(which):
    def make(C, B, H, W, bf=False):
        def case(k):
            L = k.L
            dt = BF16 if bf else F32
            wrap = (lambda c: bf16_storage(L, c)) if bf else (lambda c: c)
            if which in ("pool2", "add", "up2x"):
                y, sc, sh = k.i("y", B, H, W, C, dtype=dt), k.pos("scale", C), k.i("shift", C, scale=0.3)
                if which == "pool2":
                    out = k.o("out", B, H // 2, W // 2, C, dtype=dt)
                    call = lambda: L.call("sifsr_bnrelu_pool2", y, sc, sh, out, B, H, W, C, S())
                elif which == "add":
                    p, out = k.i("p", B, H, W, C, dtype=dt), k.o("out", B, H, W, C, dtype=dt)
                    call = lambda: L.call("sifsr_bnrelu_add", p, y, sc, sh, out, C, B * H * W, S())
                else:
                    out = k.o("out", B, 2 * H, 2 * W, C, dtype=dt)
                    call = lambda: L.call("sifsr_bnrelu_up2x", y, sc, sh, out, B, H, W, C, S())
                return wrap(call), {"out": out}
            if which in ("pool2_bwd", "pool2_bwd_acc"):
                gp = k.i("gp", B, H // 2, W // 2, C, dtype=dt)
                if which == "pool2_bwd":
                    g = k.o("g", B, H, W, C, dtype=dt)
                else:
                    g = k.A.inout(torch.from_numpy(k.rs.standard_normal((B, H, W, C)).astype(np.float32)).to(dt), "g")
                call = lambda: L.call("sifsr_pool2_bwd", gp, g, B, H, W, C, 1 if which == "pool2_bwd_acc" else 0, S())
                return wrap(call), {"g": g}
            gu, g = k.i("gu", B, 2 * H, 2 * W, C, dtype=dt), k.o("g", B, H, W, C, dtype=dt)
            if which == "up2x_bwd":
                return wrap(lambda: L.call("sifsr_up2x_bwd", gu, g, B, H, W, C, S())), {"g": g}
            rows = L.call("sifsr_up2x_bwd_stat_rows", B, H, W, C)
            assert rows > 0
            y, sc, sh = k.i("y", B, H, W, C, dtype=dt), k.pos("scale", C), k.i("shift", C, scale=0.3)
            part = k.o("partials", rows, C, 2)
            call = lambda: L.call("sifsr_up2x_bwd_bn_sums", gu, g, B, H, W, C, y, sc, sh, part, S())
            return wrap(call), {"g": g, "partials": part}
        return case
    shapes = [s for s in RES_SHAPES if not (which == "up2x_bwd_bn_sums" and s[0] == 8)]
    return [make(*s) for s in shapes] + [make(32, 2, 16, 24, bf=True)]


# ---- SIF loss operators, optimizer, pipeline, metrics ------------------------------------------------------------------------------
def _taps(mtf):
    from sifsr.sif_ops import _taps_c
    return _taps_c(mtf, 4, None)


def image_op(name, out_shape, in_shape, taps, sizes):
    def make(B, H, W):
        def case(k):
            L = k.L
            x = k.i("in", *in_shape(B, H, W))
            out = k.o("out", *out_shape(B, H, W))
            if taps:
                call = lambda: L.call(name, x, _taps(0.25), out, B, H, W, S())
            else:
                call = lambda: L.call(name, x, out, B, H, W, S())
            return call, {"out": out}
        return case
    return [make(*s) for s in sizes]


ANY = [(2, 12, 16), (2, 37, 50), (1, 100, 36), (2, 64, 128)]       # any H, W >= 10
MUL4 = [(2, 12, 16), (2, 40, 56), (1, 100, 36), (2, 64, 128)]      # multiples of 4 where a /4 decimation is involved
full = lambda B, H, W: (B, 1, H, W)
quarter = lambda B, H, W: (B, 1, H // 4, W // 4)
four = lambda B, H, W: (B, 4, H, W)


def huber(bwd):
    def make(n):
        def case(k):
            L = k.L
            a, b = k.i("a", n, scale=1.5), k.i("b", n)
            if bwd:
                gout, ga = k.i("gout", 1), k.o("ga", n)
                return (lambda: L.call("sifsr_huber_bwd", a, b, -0.4, gout, n, ga, S())), {"ga": ga}
            partials = k.s("partials", L.call("sifsr_huber_partial_blocks", n))
            out = k.o("out", 1)
            return (lambda: L.call("sifsr_huber_fwd", a, b, -0.4, n, partials, out, S())), {"out": out}
        return case
    return [make(1), make(255), make(8192), make(1000003)]


def sif_loss():
    def make(kind, B, H, W, with_grad):
        def case(k):
            L = k.L
            sr, lst = k.i("sr", B, 1, H, W, scale=1.3), k.i("lst", B, 1, H // 4, W // 4)
            ndvi = k.i("ndvi", B, 1, H, W)
            nbytes = L.call("sifsr_sif_loss_workspace_bytes", kind, B, H, W)
            ws = k.A.scratch(nbytes, "workspace")
            losses = k.o("losses3", 3)
            dsr = k.o("dsr", B, 1, H, W) if with_grad else None
            call = lambda: L.call("sifsr_sif_loss", kind, sr, lst, ndvi, B, H, W, 307.2378, 5.5698, 0.5, -0.25, _taps(0.1), _taps(0.25),
                                  ws, nbytes, losses, dsr, S())
            outs = {"losses3": losses}
            if with_grad:
                outs["dsr"] = dsr
            return call, outs
        return case
    return [make(2, 2, 48, 80, True), make(1, 2, 48, 80, True), make(2, 2, 100, 36, True), make(1, 1, 32, 32, False),
            make(2, 2, 256, 256, True)]


def adam(dev_step):
    def make(n):
        def case(k):
            L = k.L
            rnd = lambda *s: torch.from_numpy(k.rs.standard_normal(s).astype(np.float32))
            p, g = k.A.inout(rnd(n), "params"), k.i("grads", n, scale=0.01)
            m, v = k.A.inout(rnd(n) * 0.01, "exp_avg"), k.A.inout(rnd(n).abs() * 1e-4, "exp_avg_sq")
            outs = {"params": p, "exp_avg": m, "exp_avg_sq": v}
            if dev_step:
                step = k.A.inout(torch.full((1,), 3, dtype=torch.int64), "step_dev")
                coef2 = k.o("coef2", 2)
                call = lambda: L.call("sifsr_adam_flat_dev", p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, coef2, 0.25, S())
                outs.update({"step_dev": step, "coef2": coef2})
            else:
                call = lambda: L.call("sifsr_adam_flat", p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 4, 0.25, S())
            return call, outs
        return case
    return [make(1), make(255), make(10007), make(282705)]


def tiles_prepare():
    def make(win, ty, tx, granule):
        def case(k):
            L = k.L
            T, hr = ty * tx, 4 * win
            if granule:
                h, w = ty * win + 3, tx * win + 5                      # a raster larger than the tiles cut from it
                lst, ndvi = k.i("lst", h, w, scale=5.0, shift=300.0), k.i("ndvi", 4 * h, 4 * w, scale=0.5)
            else:
                h = w = 0
                lst, ndvi = k.i("lst", T, 1, win, win, scale=5.0, shift=300.0), k.i("ndvi", T, 1, hr, hr, scale=0.5)
            x = k.o("x", T, 2, hr, hr)
            call = lambda: L.call("sifsr_tiles_prepare", lst, ndvi, x, ty, tx, win, h, w, granule, 307.2378, 5.5698, 0.3, 0.2, 1, S())
            return call, {"x": x}
        return case
    return [make(16, 3, 1, 0), make(64, 2, 1, 0), make(16, 2, 3, 1), make(4, 1, 1, 0), make(64, 1, 2, 1)]


def tiles_paste():
    def make(win, ty, tx, extra):
        def case(k):
            L = k.L
            hr = 4 * win
            lst_w = tx * win + extra
            sr = k.i("sr", ty * tx, 1, hr, hr)
            out = k.o("out", ty * hr, 4 * lst_w)
            init = out.clone()
            m = torch.zeros(1, 4 * lst_w, dtype=torch.bool)
            m[:, :tx * hr] = True                                      # columns right of the last tile are not the call's to write
            call = lambda: L.call("sifsr_tiles_paste", sr, out, ty, tx, win, lst_w, 307.2378, 5.5698, S())
            return call, {"out": (lambda: Partial(out, m, init))}
        return case
    return [make(16, 2, 3, 0), make(16, 2, 3, 5), make(64, 1, 2, 1), make(4, 1, 1, 0)]


def psnr_ssim():
    def make(B, H, W):
        def case(k):
            L = k.L
            p, t = k.i("pred", B, 1, H, W, scale=5.0, shift=300.0), k.i("targ", B, 1, H, W, scale=5.0, shift=300.0)
            nbytes = L.call("sifsr_psnr_ssim_scratch_bytes", B, H, W)
            scratch, out = k.A.scratch(nbytes, "scratch"), k.o("out2", 2)
            return (lambda: L.call("sifsr_psnr_ssim", p, t, B, H, W, scratch, nbytes, out, S())), {"out2": out}
        return case
    return [make(2, 96, 80), make(1, 16, 16), make(3, 256, 256), make(2, 41, 57)]


def eval_metrics():
    def make(B, H, W, dr):
        def case(k):
            L = k.L
            ref = k.i("ref", B, 1, H, W, scale=5.0, shift=300.0)
            pred = k.t("pred", ref.cpu() + torch.from_numpy(k.rs.standard_normal((B, 1, H, W)).astype(np.float32)))
            nbytes = L.call("sifsr_eval_metrics_scratch_bytes", B, H, W)
            scratch, out = k.A.scratch(nbytes, "scratch"), k.o("out8", B, 8, dtype=F64)
            call = lambda: L.call("sifsr_eval_metrics", ref, pred, B, H, W, _taps(0.1), dr, scratch, nbytes, out, S())
            return call, {"out8": out}
        return case
    return [make(1, 16, 16, -1.0), make(2, 41, 57, -1.0), make(3, 256, 256, 40.0), make(1, 335, 374, -1.0)]


def gradient_strata():
    def make(B, H, W):
        def case(k):
            L = k.L
            ref = k.i("ref", B, 1, H, W, scale=5.0, shift=300.0)
            g, q2, cnt = k.o("g", B, 1, H, W), k.o("q2", B, 2), k.o("counts3", B, 3, dtype=torch.int32)
            call = lambda: L.call("sifsr_gradient_strata", ref, B, H, W, _taps(0.1), g, q2, cnt, S())
            return call, {"g": g, "q2": q2, "counts3": cnt}
        return case
    return [make(1, 16, 16), make(2, 41, 57), make(2, 256, 256)]


def l4pool4():
    def make(B, H, W):
        def case(k):
            L = k.L
            x, out = k.i("x", B, H, W, scale=5.0, shift=300.0), k.o("out", B, H // 4, W // 4)
            return (lambda: L.call("sifsr_l4pool4", x, out, B, H, W, S())), {"out": out}
        return case
    return [make(1, 4, 4), make(2, 12, 16), make(2, 100, 36), make(3, 256, 256)]


def fft2():
    def make(B, H, W, want_mag, want_spec):
        def case(k):
            L = k.L
            img = k.i("img", B, H, W, scale=5.0, shift=300.0)
            nbytes = L.call("sifsr_fft2_attenuation_scratch_bytes", B, H, W)
            scratch = k.A.scratch(nbytes, "scratch")
            nr = min(H // 2, W // 2) - 1
            mag = k.o("mag", B, H, W) if want_mag else None
            spec = k.o("spectrum", B, nr + 1) if want_spec else None
            call = lambda: L.call("sifsr_fft2_attenuation", img, B, H, W, scratch, nbytes, mag, spec, S())
            outs = {}
            if want_mag:
                outs["mag"] = mag
            if want_spec:
                outs["spectrum"] = spec
            return call, outs
        return case
    return [make(1, 4, 4, True, True), make(2, 64, 256, True, True), make(3, 256, 256, False, True), make(1, 128, 32, True, False)]


def pack(wino):
    def make(cin, cout):
        def case(k):
            L = k.L
            w = k.i("w_oihw", cout, cin, 3, 3, scale=(2.0 / (9 * cin)) ** 0.5)
            n = 9 * cin * cout
            if wino:
                a, b = k.o("wwf", 16 * cin * cout), k.o("wwd", 16 * cin * cout)
                return (lambda: L.call("sifsr_pack_conv_weights_wino", w, cin, cout, a, b, S())), {"wwf": a, "wwd": b}
            a, b = k.o("wfwd", n), k.o("wdgrad", 4 * n)
            init = b.clone()
            m = torch.zeros(4 * n, dtype=torch.bool)
            m[:2 * n] = True                                           # the last 2n floats are documented as unused
            return (lambda: L.call("sifsr_pack_conv_weights", w, cin, cout, a, b, S())), {"wfwd": a, "wdgrad": (lambda: Partial(b, m, init))}
        return case
    return [make(16, 16), make(32, 16), make(128, 64), make(64, 128)]


ENGINE = ["covered by tests/test_workspace_poison_gpu.py"]

CONTRACT = {
    "sifsr_model_forward": ENGINE, "sifsr_model_backward": ENGINE, "sifsr_model_forward_ex": ENGINE, "sifsr_model_backward_ex": ENGINE,
    "sifsr_pack_conv_weights": pack(False), "sifsr_pack_conv_weights_wino": pack(True),
    "sifsr_conv3x3_fwd": conv_fwd("tap"), "sifsr_conv3x3_fwd_wino": conv_fwd("wino"), "sifsr_conv3x3_fwd_bf16": conv_fwd("bf16"),
    "sifsr_conv3x3_dgrad": conv_dgrad("tap"), "sifsr_conv3x3_dgrad_wino": conv_dgrad("wino"),
    "sifsr_conv3x3_dgrad_bf16": conv_dgrad("bf16"), "sifsr_conv3x3_dgrad_fused": conv_dgrad_fused(),
    "sifsr_conv3x3_wgrad": conv_wgrad("tap"), "sifsr_conv3x3_wgrad_fused": conv_wgrad("fused"),
    "sifsr_conv3x3_wgrad_wino": conv_wgrad("wino") + conv_wgrad("wino_fused"), "sifsr_conv3x3_wgrad_bf16": conv_wgrad("bf16"),
    "sifsr_conv3x3_bwd16": conv_bwd16() + conv_bwd16(storage_bf16=True),
    "sifsr_conv3x3_bwd16_pool": conv_bwd16_variant("pool"), "sifsr_conv3x3_bwd16_tail": conv_bwd16_variant("tail"),
    "sifsr_conv_in_fwd": conv_in_fwd(), "sifsr_conv_in_wgrad": conv_in_wgrad(),
    "sifsr_conv_out_fwd": conv_out_fwd(), "sifsr_conv_out_dgrad": conv_out_dgrad(), "sifsr_conv_out_wgrad": conv_out_wgrad(),
    "sifsr_conv_out_bn_relu_bwd": conv_out_bn_relu_bwd(), "sifsr_conv_in_bn_relu_bwd": conv_in_bn_relu_bwd(),
    "sifsr_conv_in_bwd_linear": conv_in_bwd_linear(),
    "sifsr_bn_finalize": bn_finalize(), "sifsr_bn_relu_bwd": bn_relu_bwd(False), "sifsr_bn_relu_bwd_coef": bn_relu_bwd(True),
    "sifsr_bnrelu_pool2": resample("pool2"), "sifsr_bnrelu_add": resample("add"), "sifsr_bnrelu_up2x": resample("up2x"),
    "sifsr_pool2_bwd": resample("pool2_bwd") + resample("pool2_bwd_acc"), "sifsr_up2x_bwd": resample("up2x_bwd"),
    "sifsr_up2x_bwd_bn_sums": resample("up2x_bwd_bn_sums"),
    "sifsr_gauss9_reflect_fwd": image_op("sifsr_gauss9_reflect_fwd", full, full, True, ANY),
    "sifsr_gauss9_reflect_bwd": image_op("sifsr_gauss9_reflect_bwd", full, full, True, ANY),
    "sifsr_gauss9_decimate4_fwd": image_op("sifsr_gauss9_decimate4_fwd", quarter, full, True, MUL4),
    "sifsr_gauss9_decimate4_bwd": image_op("sifsr_gauss9_decimate4_bwd", full, quarter, True, MUL4),
    "sifsr_sobel4_fwd": image_op("sifsr_sobel4_fwd", four, full, False, ANY),
    "sifsr_sobel4_bwd": image_op("sifsr_sobel4_bwd", full, four, False, ANY),
    "sifsr_huber_fwd": huber(False), "sifsr_huber_bwd": huber(True), "sifsr_sif_loss": sif_loss(),
    "sifsr_adam_flat": adam(False), "sifsr_adam_flat_dev": adam(True),
    "sifsr_tiles_prepare": tiles_prepare(), "sifsr_tiles_paste": tiles_paste(),
    "sifsr_psnr_ssim": psnr_ssim(), "sifsr_eval_metrics": eval_metrics(), "sifsr_gradient_strata": gradient_strata(),
    "sifsr_l4pool4": l4pool4(), "sifsr_fft2_attenuation": fft2(),
}

CASES = [(name, i) for name, cases in CONTRACT.items() if cases is not ENGINE for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[6:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx)


def test_table_is_complete():
    """every row has cases and every case index is reachable (the header-side gate is tests/test_capi_gate.py)"""
    assert len(CASES) >= 250 and all(CONTRACT[n] for n in CONTRACT)
    assert set(ENGINE_ENTRY_POINTS) == {n for n, c in CONTRACT.items() if c is ENGINE}


@pytest.mark.parametrize("C,pool", [(16, False), (32, True), (64, True)])
def test_bn_relu_bwd_follows_bf16_storage(L, C, pool):
    """The finding of this module: with sifsr_set_op_storage_bf16(1) the reduction half of sifsr_bn_relu_bwd read g and y as bf16
    but its second pass read them as fp32 and wrote dy as fp32 -- twice the bytes of the bf16 tensor the header describes.  Now
    both follow the mode: the same bf16 VALUES handed over as fp32 tensors give bit-identical dgamma / dbeta / coef (same values,
    same float64 sums), and dy is that fp32 dy rounded to nearest-even bf16 (stA4, common.h), bit for bit."""
    rs = np.random.RandomState(50 + C)
    B, H, W, nb = 2, 16, 24, 5
    rb = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(BF16)
    g, y = rb(B, H, W, C), rb(B, H, W, C)
    gp = rb(B, H // 2, W // 2, C) if pool else None
    vec = lambda lo, hi: torch.from_numpy(rs.uniform(lo, hi, C).astype(np.float32)).cuda()
    sc, sh, mean, inv = vec(0.5, 1.5), vec(-0.3, 0.3), vec(-0.3, 0.3), vec(0.5, 1.5)
    out = {}
    for mode, dt in (("fp32", F32), ("bf16", BF16)):
        partials = torch.full((nb * C * 2,), float("nan"), device="cuda")
        dgam, dbet = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        coef = torch.full((3 * C,), float("nan"), dtype=F64, device="cuda")
        dy = torch.full((B, H, W, C), float("nan"), dtype=dt, device="cuda")
        call = lambda: L.call("sifsr_bn_relu_bwd", g.to(dt).cuda(), y.to(dt).cuda(), sc, sh, mean, inv, C, B * H * W, partials, nb, dgam,
                              dbet, coef, dy, gp.to(dt).cuda() if pool else None, H if pool else 0, W if pool else 0, S())
        (bf16_storage(L, call) if mode == "bf16" else call)()
        torch.cuda.synchronize()
        out[mode] = (dgam, dbet, coef, dy)
    a, b = out["bf16"], out["fp32"]
    assert bit_equal(a[0], b[0]) and bit_equal(a[1], b[1]) and bit_equal(a[2], b[2])
    assert not torch.isnan(a[3].float()).any()
    assert bit_equal(a[3], b[3].to(BF16))


@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (1, 16, 16), (2, 32, 48)])
def test_conv_out_backward_follows_bf16_storage(L, B, H, W):
    """The second finding: sifsr_conv_out_dgrad wrote g as fp32 and sifsr_conv_out_wgrad read y as fp32 whatever the storage
    mode.  With sifsr_set_op_storage_bf16(1) g must be the fp32 result rounded to nearest-even bf16, and the weight gradient of a
    bf16 y must equal, bit for bit, that of the same values handed over as an fp32 tensor (same kernel arithmetic after widening)."""
    rs = np.random.RandomState(90 + H)
    f = lambda *s, sc=1.0: torch.from_numpy((rs.standard_normal(s) * sc).astype(np.float32))
    dsr, w, y = f(B, 1, H, W).cuda(), f(1, 16, 3, 3, sc=0.2).cuda(), f(B, H, W, 16).to(BF16)
    sc = torch.from_numpy(rs.uniform(0.5, 1.5, 16).astype(np.float32)).cuda()
    sh = f(16, sc=0.3).cuda()
    nb = 5
    out = {}
    for mode, dt in (("fp32", F32), ("bf16", BF16)):
        g = torch.full((B, H, W, 16), float("nan"), dtype=dt, device="cuda")
        yy = y.to(dt).cuda()
        scratch = torch.full((nb * 145,), float("nan"), device="cuda")
        dwb = torch.full((145,), float("nan"), device="cuda")

        def call():
            L.call("sifsr_conv_out_dgrad", dsr, w, g, B, H, W, S())
            L.call("sifsr_conv_out_wgrad", yy, sc, sh, dsr, scratch, nb, dwb, B, H, W, S())
        (bf16_storage(L, call) if mode == "bf16" else call)()
        torch.cuda.synchronize()
        out[mode] = (g, dwb)
    assert not torch.isnan(out["bf16"][0].float()).any() and not torch.isnan(out["bf16"][1]).any()
    assert bit_equal(out["bf16"][0], out["fp32"][0].to(BF16))
    assert bit_equal(out["bf16"][1], out["fp32"][1])
