"""conv3x3_bwd16_kernel (csrc/conv_bwd16.hip: input gradient, weight gradient and the BatchNorm-backward sums of the layer below from
one read of the operands) across its tile walk, through its three entry points sifsr_conv3x3_bwd16, _pool and _tail, in both storage
modes.  Mirror, float64 restatements, case table, inputs and the comparison live in tests/bwd16_reference.py and are pinned on the
CPU by tests/test_bwd16_walk_host.py.

Every case asserts its regime from the mirror BEFORE it launches (grid, XCD or plain stride, power-of-two or generic tile index,
tiles per workgroup, interior tiles): a case that drifts out of its regime fails instead of passing trivially.  Every output -- gin,
dw, the border scratch, the statistic rows, the slab scratch -- starts NaN-filled between sentinel guards.

  * exact cases (small-integer operands, hand-made coef_f): gin, dw, the border scratch (NaN off the image border), every statistic
    row of the main kernel (= the float64 sums over exactly the tiles the mirror gives that workgroup) and the column sums are compared
    with the float64 restatement BIT FOR BIT, in fp32 and in bf16 storage (there: round-to-nearest-even where the kernels round,
    the second rounding of image-border pixels by the border-fold kernel included).  A mismatch names the image, the tile, the pixel,
    interior or not, the workgroup and the position in its walk.
  * random cases (N(0,1) operands, coef_f from float64 statistics on the host): the project's bars -- gin 1e-4 of the maximum
    (BASELINE.json), dw per element 1e-5 x the F(3x3,2x2) yardstick of tests/wgrad_reference.py, sums 1e-4 * sum|dz|, 1e-4 * sum|dz*y|;
    bf16 storage by the bars of test_bf16_storage_fused_backward_of_16_channel_layers.
  * walk independence: the same tensors in batch chunks of at most 256 tiles (one tile per workgroup) give bit-identical gin and
    border scratch; dw and the summed statistic rows of the chunks meet the same bars (exact cases: equal); two whole runs are
    bit-identical in everything.
  * exactly grid() slabs written, none beyond; all stat_rows() rows finite.
  * refusals return their status code without a launch: outputs stay NaN, guards intact.

SIFSR_BWD16_WALK_REPORT=<path>: write the largest error / bar of the random cases per entry point and storage mode."""
import json
import os

import pytest
import torch

from tests import bwd16_reference as M
from tests import storage_reference as R
from tests import wgrad_reference as WR
from tests.test_storage_edge_gpu import ERR_ARG, ERR_SHAPE, Out, raw_bits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
C = 16
TOL = 1e-4                                   # BASELINE.json north_star: within 1e-4 relative fp32
BAR_DW = 1e-5                                # the project's bar for weight gradients, x the yardstick (tests/wgrad_reference.py)
BF16_GIN_MAX, BF16_GIN_MEAN, BF16_DW_FORMED, BF16_DW_STORED, BF16_SUMS = 1.2e-2, 2.5e-3, 2e-3, 1e-5, 2e-3   # tests/test_bf16_gpu.py
WORST = {}


@pytest.fixture(scope="module")
def L():
    import sifsr  # noqa: F401
    from sifsr import _lib
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SIFSR_BWD16_WALK_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({k: {"launches": v[0], "worst_error_over_bar": v[1], "at": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)


@pytest.fixture(params=[False, True], ids=["fp32", "bf16"])
def hs(request, L):
    L.call("sifsr_set_op_storage_bf16", 1 if request.param else 0)
    yield request.param
    L.call("sifsr_set_op_storage_bf16", 0)


def S():
    return torch.cuda.current_stream().cuda_stream


def note(entry, quantity, bf16, ratio, at):
    key = f"{entry}/{quantity}/{'bf16' if bf16 else 'fp32'}"
    n, w, a = WORST.get(key, (0, 0.0, ""))
    WORST[key] = (n + 1, max(w, float(ratio)), at if float(ratio) > w else a)


def up(t, hs):
    """NCHW host -> NHWC device activation tensor in the storage mode"""
    return t.permute(0, 2, 3, 1).contiguous().to(BF if hs else torch.float32).cuda()


def host(t):
    return t.to(F64).permute(0, 3, 1, 2).cpu()


class Operands:
    """the device tensors of one (case, mode): activations in the storage mode, parameters fp32, the packed weights"""

    def __init__(self, L, inp, mode, hs):
        m = M.MODES[mode]
        self.m, self.hs = m, hs
        self.B, _, self.H, self.W = inp["x"].shape
        w = inp["w"].float().cuda()
        wf = torch.empty(9 * C * C, device="cuda"); self.wd = torch.empty(4 * 9 * C * C, device="cuda")
        L.call("sifsr_pack_conv_weights", w, C, C, wf, self.wd, S())
        wwf = torch.empty(16 * C * C, device="cuda"); self.wwd = torch.empty(16 * C * C, device="cuda")
        L.call("sifsr_pack_conv_weights_wino", w, C, C, wwf, self.wwd, S())
        self.x = up(inp["x"], hs)
        self.xs, self.xsh = (inp["xs"].float().cuda(), inp["xsh"].float().cuda()) if m.folded else (None, None)
        self.g = self.y = self.coef = self.gp = self.dsr = self.w_out = self.addend = None
        if not m.formed:
            self.g = up(inp["dy"], hs)
        else:
            self.y, self.coef = up(inp["y"], hs), inp["coef_f"].float().cuda()
            if m.entry == "tail":
                self.dsr, self.w_out = inp["dsr"].float().contiguous().cuda(), inp["w_out"].float().contiguous().cuda()
            else:
                self.g = up(inp["g"], hs)
                if m.entry == "pool":
                    self.gp = up(inp["gp"], hs)
        if m.addend:
            self.addend = up(inp["addend"], hs)


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(L, op, b0=0, b1=None):
    """one call on images b0 .. b1 of the operands -> (status, dict of guarded outputs)"""
    m, hs, H, W = op.m, op.hs, op.H, op.W
    b1 = op.B if b1 is None else b1
    B = b1 - b0
    sl = lambda t: None if t is None else t[b0:b1]
    rows = L.call("sifsr_conv3x3_bwd16_stat_rows", B, H, W)
    nscr = L.call("sifsr_conv3x3_bwd16_scratch_floats", B, H, W)
    assert rows == M.stat_rows(B, H, W) and nscr == M.scratch_floats(B, H, W)        # the mirror against what is observable
    act = BF if hs else torch.float32
    o = dict(gin=Out((B, H, W, C), act), dw=Out((C, C, 3, 3)), scratch=Out((nscr,)))
    if m.formed:
        o["border"] = Out((B, H, W, C), act)
    if m.sums:
        o["rows"] = Out((rows, C, 2))
    x = sl(op.x)
    bn = (ptr(x), ptr(op.xs), ptr(op.xsh), o["rows"].t.data_ptr()) if m.sums else (None, None, None, None)
    brd = o["border"].t.data_ptr() if m.formed else None
    tailargs = (o["scratch"].t.data_ptr(), o["dw"].t.data_ptr(), B, H, W, S())
    lib = L.lib()
    if m.entry == "main":
        rc = lib.sifsr_conv3x3_bwd16(ptr(x), ptr(op.xs), ptr(op.xsh), ptr(sl(op.g)), ptr(sl(op.y)), ptr(op.coef), brd, ptr(op.wd), ptr(op.wwd),
                                     o["gin"].t.data_ptr(), ptr(sl(op.addend)), *bn, *tailargs)
    elif m.entry == "pool":
        rc = lib.sifsr_conv3x3_bwd16_pool(ptr(x), ptr(op.xs), ptr(op.xsh), ptr(sl(op.g)), ptr(sl(op.gp)), ptr(sl(op.y)), ptr(op.coef), brd,
                                          ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), *bn, *tailargs)
    else:
        rc = lib.sifsr_conv3x3_bwd16_tail(ptr(x), ptr(op.xs), ptr(op.xsh), ptr(sl(op.dsr)), ptr(op.w_out), ptr(sl(op.y)), ptr(op.coef), brd,
                                          ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), *bn, *tailargs)
    torch.cuda.synchronize()
    return rc, o


def collect(o, B, H, W):
    """guards checked; -> host float64 results in the restatement's terms"""
    g = M.grid(B, H, W)
    got = dict(gin=host(o["gin"].ok("gin")), dw=o["dw"].ok("dw").to(F64).cpu())
    slabs = o["scratch"].ok("slab scratch")
    assert slabs.numel() == g * 9 * 256 and bool(torch.isfinite(slabs).all()), "a slab of a launched workgroup is not fully written"
    if "border" in o:
        got["border"] = host(o["border"].ok("border"))
    if "rows" in o:
        rows = o["rows"].ok("statistic rows").to(F64).cpu()
        assert bool(torch.isfinite(rows).all()), "a statistic row was left unwritten"
        got["rows_main"], got["rows_border"] = rows[:g], rows[g:].sum(0)
        got["cols"] = rows.sum(0)
    return got


def same_run(o1, o2):
    for k in o1:
        assert torch.equal(raw_bits(o1[k].t), raw_bits(o2[k].t)), f"two runs differ in {k}"


def chunked(L, op, walk):
    """the same tensors in batch chunks of one tile per workgroup -> results in the whole run's terms (dw, rows summed in float64)"""
    per_img = walk.ty * walk.tx
    nb = max(1, 256 // per_img) if walk.tmax > 1 else 1
    outs = []
    for b0 in range(0, op.B, nb):
        b1 = min(op.B, b0 + nb)
        wk = M.Walk(b1 - b0, op.H, op.W)
        assert wk.tmax == 1 and wk.pow2 == walk.pow2, wk.describe()
        rc, o = launch(L, op, b0, b1)
        assert rc == 0
        outs.append(collect(o, b1 - b0, op.H, op.W))
    res = dict(gin=torch.cat([c["gin"] for c in outs]), dw=sum(c["dw"] for c in outs))
    if "border" in outs[0]:
        res["border"] = torch.cat([c["border"] for c in outs])
    if "cols" in outs[0]:
        res["cols"] = sum(c["cols"] for c in outs)
        res["rows_border"] = sum(c["rows_border"] for c in outs)
    return res


def independent_of_the_walk(walk, got, chk):
    for k in ("gin", "border"):
        if k in got:
            rep = M.first_mismatch(walk, {k: chk[k]}, {k: got[k]})
            assert rep is None, "the whole run (expected) against one tile per workgroup (got): " + rep


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", M.PAIRS, ids=lambda v: str(v))
def test_exact(L, hs, name, mode):
    case = M.BY_NAME[name]
    walk = M.wanted_walk(case)                       # the regime, before any launch
    inp = M.exact_inputs(name)
    exp = M.expected(inp, mode, hs, walk)
    op = Operands(L, inp, mode, hs)
    rc, o = launch(L, op)
    assert rc == 0
    got = collect(o, case.B, case.H, case.W)
    rep = M.first_mismatch(walk, got, exp)
    assert rep is None, f"{name}/{mode} ({walk.describe()}): {rep}"
    rc, o2 = launch(L, op)
    assert rc == 0
    same_run(o, o2)
    if case.B > 1:
        chk = chunked(L, op, walk)
        independent_of_the_walk(walk, got, chk)
        for k in ("dw", "cols", "rows_border"):      # exact values in any grouping
            if k in chk:
                assert torch.equal(chk[k], exp[k]), k


def _yardstick(a, dy, chunk=8):
    y = torch.zeros(C, C, 3, 3, dtype=F64)
    for b0 in range(0, a.shape[0], chunk):
        y += WR.wino_wgrad(a[b0:b0 + chunk], dy[b0:b0 + chunk], absolute=True)
    return y


def _check_random(entry, hs, at, got, ref, yard, m, x, pos):
    """the bars, each from where it already stands in the project"""
    gin, rg = got["gin"], ref["gin"]
    assert bool(torch.isfinite(gin).all())
    err = (gin - rg).abs()
    if not hs:
        r = float(err.max()) / (TOL * float(rg.abs().max()))
        note(entry, "gin", hs, r, at); assert r <= 1.0, (at, "gin", r)
        r = float(((got["dw"] - ref["dw"]).abs() / (BAR_DW * yard)).max())
        note(entry, "dw", hs, r, at); assert r <= 1.0, (at, "dw", r)
    else:
        r = max(float(err.max()) / (BF16_GIN_MAX * float(rg.abs().max())), float(err.mean()) / (BF16_GIN_MEAN * float(rg.abs().mean())))
        note(entry, "gin", hs, r, at); assert r <= 1.0, (at, "gin", r)
        bar = BF16_DW_FORMED if m.formed else BF16_DW_STORED
        r = float((got["dw"] - ref["dw"]).abs().max()) / (bar * float(ref["dw"].abs().max()))
        note(entry, "dw", hs, r, at); assert r <= 1.0, (at, "dw", r)
    if "border" in got:
        e = M.edge_mask(*gin.shape[2:])
        assert bool(torch.isnan(got["border"][:, :, ~e]).all()), "border scratch written off the image border"
        gb, rb_ = got["border"][:, :, e], ref["border"][:, :, e]
        bar = TOL * float(rb_.abs().max()) + (R.BF_EPS * rb_.abs() if hs else 0.0)        # bf16: one rounding of the stored value
        r = float(((gb - rb_).abs() / bar).max())
        note(entry, "border", hs, r, at); assert r <= 1.0, (at, "border", r)
    if "cols" in got:
        zero = torch.zeros((), dtype=F64)
        if not hs:
            dz = torch.where(pos, rg, zero)
            s_ref = torch.stack((dz.sum((0, 2, 3)), (dz * x).sum((0, 2, 3))), 1)
            s_abs = torch.stack((dz.abs().sum((0, 2, 3)), (dz * x).abs().sum((0, 2, 3))), 1)
            r = float(((got["cols"] - s_ref).abs() / (TOL * s_abs)).max())
        else:                                            # the sums of the STORED gradient (the fold's deltas are summed unrounded)
            dz = torch.where(pos, gin, zero)
            s_ref = torch.stack((dz.sum((0, 2, 3)), (dz * x).sum((0, 2, 3))), 1)
            r = float((got["cols"] - s_ref).abs().max()) / (BF16_SUMS * float(s_ref.abs().max()))
        note(entry, "sums", hs, r, at); assert r <= 1.0, (at, "sums", r)


@pytest.mark.parametrize("name,mode", M.PAIRS, ids=lambda v: str(v))
def test_random(L, hs, name, mode):
    case = M.BY_NAME[name]
    walk = M.wanted_walk(case)
    m = M.MODES[mode]
    inp = dict(M.random_inputs(name, hs))
    if m.formed:
        inp["y"], inp["coef_f"] = M.random_coef(inp, mode, hs)
    ref = M.expected(inp, mode, False, walk)             # float64 on the values the tensors hold
    yard = _yardstick(ref["a"], ref["dy"]) if not hs else None
    x = inp["x"].to(F64)
    pos = (x * inp["xs"].to(F64).view(1, -1, 1, 1) + inp["xsh"].to(F64).view(1, -1, 1, 1)) > 0 if m.sums else None
    op = Operands(L, inp, mode, hs)
    rc, o = launch(L, op)
    assert rc == 0
    got = collect(o, case.B, case.H, case.W)
    at = f"{name}/{mode}"
    _check_random(m.entry, hs, at, got, ref, yard, m, x, pos)
    rc, o2 = launch(L, op)
    assert rc == 0
    same_run(o, o2)
    if case.B > 1:
        chk = chunked(L, op, walk)
        independent_of_the_walk(walk, got, chk)
        _check_random(m.entry + " in chunks", hs, at, chk, ref, yard, m, x, pos)


# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(L, hs):
    case = M.BY_NAME["geo32"]
    inp = M.exact_inputs(case.name)

    def untouched(o):
        for k, v in o.items():
            assert bool(torch.isnan(v.ok(k).float()).all()), f"{k} was written by a refused call"

    # H or W below 32, or no multiple of 16
    for (H, W) in ((16, 32), (32, 16), (40, 32), (32, 72), (24, 24)):
        small = dict(inp)
        for k in ("x", "dy", "g", "y", "addend"):
            small[k] = torch.ones(1, C, H, W)
        small["dsr"], small["gp"] = torch.ones(1, H, W), torch.ones(1, C, H // 2, W // 2)
        assert M.stat_rows(1, H, W) == 0 and L.call("sifsr_conv3x3_bwd16_stat_rows", 1, H, W) == 0
        assert L.call("sifsr_conv3x3_bwd16_scratch_floats", 1, H, W) == 0
        for mode in ("a", "c", "e", "f"):
            op = Operands(L, small, mode, hs)
            # (the queries return 0 for a refused shape: give the call real buffers of the nearest legal size instead)
            m = op.m
            act = BF if hs else torch.float32
            o = dict(gin=Out((1, H, W, C), act), dw=Out((C, C, 3, 3)), scratch=Out((9 * 256 * 16,)), border=Out((1, H, W, C), act), rows=Out((64, C, 2)))
            bn = (ptr(op.x), ptr(op.xs), ptr(op.xsh), o["rows"].t.data_ptr()) if m.sums else (None,) * 4
            end = (o["scratch"].t.data_ptr(), o["dw"].t.data_ptr(), 1, H, W, S())
            brd = o["border"].t.data_ptr()
            lib = L.lib()
            if m.entry == "main":
                rc = lib.sifsr_conv3x3_bwd16(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.g), ptr(op.y), ptr(op.coef), brd if m.formed else None,
                                             ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), None, *bn, *end)
            elif m.entry == "pool":
                rc = lib.sifsr_conv3x3_bwd16_pool(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.g), ptr(op.gp), ptr(op.y), ptr(op.coef), brd,
                                                  ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), *bn, *end)
            else:
                rc = lib.sifsr_conv3x3_bwd16_tail(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.dsr), ptr(op.w_out), ptr(op.y), ptr(op.coef), brd,
                                                  ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), *bn, *end)
            torch.cuda.synchronize()
            assert rc == ERR_SHAPE, (H, W, mode, rc)
            untouched(o)

    # argument errors at a legal shape
    B, H, W = case.B, case.H, case.W
    act = BF if hs else torch.float32

    def outs():
        return dict(gin=Out((B, H, W, C), act), dw=Out((C, C, 3, 3)), scratch=Out((M.scratch_floats(B, H, W),)), border=Out((B, H, W, C), act),
                    rows=Out((M.stat_rows(B, H, W), C, 2)))

    lib = L.lib()
    pool, tail, cc, dd = Operands(L, inp, "e", hs), Operands(L, inp, "f", hs), Operands(L, inp, "c", hs), Operands(L, inp, "d", hs)
    # pool_gp or the tail without y / coef_f / border
    for drop in ("y", "coef", "border"):
        for op in (pool, tail):
            o = outs()
            y, coef, brd = (None if drop == "y" else ptr(op.y)), (None if drop == "coef" else ptr(op.coef)), (None if drop == "border" else o["border"].t.data_ptr())
            end = (ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), ptr(op.x), ptr(op.xs), ptr(op.xsh), o["rows"].t.data_ptr(), o["scratch"].t.data_ptr(),
                   o["dw"].t.data_ptr(), B, H, W, S())
            if op is pool:
                rc = lib.sifsr_conv3x3_bwd16_pool(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.g), ptr(op.gp), y, coef, brd, *end)
            else:
                rc = lib.sifsr_conv3x3_bwd16_tail(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.dsr), ptr(op.w_out), y, coef, brd, *end)
            torch.cuda.synchronize()
            assert rc == ERR_ARG, (drop, op.m.entry, rc)
            untouched(o)
    # sums whose bn_y / bn_scale / bn_shift are not x / x_scale / x_shift (equal values in other buffers), in each entry point
    for which in range(3):
        for op in (cc, pool, tail):
            o = outs()
            bn = [op.x, op.xs, op.xsh]
            bn[which] = bn[which].clone()
            end = (ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), o["rows"].t.data_ptr(), o["scratch"].t.data_ptr(), o["dw"].t.data_ptr(), B, H, W, S())
            brd = o["border"].t.data_ptr()
            if op is cc:
                rc = lib.sifsr_conv3x3_bwd16(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.g), ptr(op.y), ptr(op.coef), brd, ptr(op.wd), ptr(op.wwd),
                                             o["gin"].t.data_ptr(), None, *end)
            elif op is pool:
                rc = lib.sifsr_conv3x3_bwd16_pool(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.g), ptr(op.gp), ptr(op.y), ptr(op.coef), brd,
                                                  ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), *end)
            else:
                rc = lib.sifsr_conv3x3_bwd16_tail(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.dsr), ptr(op.w_out), ptr(op.y), ptr(op.coef), brd,
                                                  ptr(op.wd), ptr(op.wwd), o["gin"].t.data_ptr(), *end)
            torch.cuda.synchronize()
            assert rc == ERR_ARG, (which, op.m.entry, rc)
            untouched(o)
    # sums together with an addend
    o = outs()
    op = cc
    rc = lib.sifsr_conv3x3_bwd16(ptr(op.x), ptr(op.xs), ptr(op.xsh), ptr(op.g), ptr(op.y), ptr(op.coef), o["border"].t.data_ptr(), ptr(op.wd),
                                 ptr(op.wwd), o["gin"].t.data_ptr(), ptr(dd.addend), ptr(op.x), ptr(op.xs), ptr(op.xsh), o["rows"].t.data_ptr(),
                                 o["scratch"].t.data_ptr(), o["dw"].t.data_ptr(), B, H, W, S())
    torch.cuda.synchronize()
    assert rc == ERR_ARG, rc
    untouched(o)
