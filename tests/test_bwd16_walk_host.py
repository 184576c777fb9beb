"""CPU tests that pin tests/bwd16_reference.py, which tests/test_bwd16_walk_gpu.py holds conv3x3_bwd16_kernel against:
  * the mirror reproduces the regimes the cases were written for (grid, stride, tile index form, tiles per workgroup, interior tiles);
  * the float64 restatements equal float64 autograd of the PyTorch ops (zero-padded conv adjoint + replicate-border fold, bn_bwd4,
    the pooling adjoint, the outlay adjoint with the clamp), and the tile-level restatement assembles to the image-level one;
  * the exactness condition of every exact case: on the magnitudes of the operands no intermediate reaches 2^22 and every operand is
    a multiple of 2^-2 or coarser, so fp32 arithmetic in any order returns the float64 values;
  * the power of the exact comparison: every mutation of the restatement is rejected, and located where it was made."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bwd16_reference as M
from tests import storage_reference as R

F64 = torch.float64
C = 16


def conv_rep(a, w):
    return F.conv2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), w)


# ---- the mirror ----
@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_mirror_reproduces_the_case_table(case):
    wk = M.wanted_walk(case)
    assert M.applies(case.B, case.H, case.W)
    assert wk.grid == M.grid(case.B, case.H, case.W) and sum(wk.counts) == wk.ntiles
    assert M.scratch_floats(case.B, case.H, case.W) == wk.grid * 9 * 256
    assert M.stat_rows(case.B, case.H, case.W) == wk.grid + case.B * 2 * (case.W // 16 + (case.H - 2 + 15) // 16)
    assert case.B * case.H * case.W * C * 4 <= 17.1e6                       # the largest tensor is about 17 MB
    # interior: the predicate counts what the table says
    n_int = sum(wk.interior(ty, tx) for (b, ty, tx) in wk.where if b == 0)
    assert n_int == case.regime["interior"]


def test_mirror_details_of_the_walk_cases():
    w = M.wanted_walk(M.BY_NAME["walk32x129"])
    assert w.counts[:164] == [3] * 164 and w.counts[164:] == [2] * 12       # 3, 2 from workgroup 164 on
    assert w.tiles[5] == [w.tile_pos(5), w.tile_pos(5 + 176), w.tile_pos(5 + 352)]
    w = M.wanted_walk(M.BY_NAME["walk64x34"])                                # uneven within each XCD
    for k in range(8):
        assert {w.counts[g] for g in range(k, w.grid, 8)} == {2, 3}
    assert w.tiles[9] == [w.tile_pos(68 + 1 + 23 * j) for j in range(3)]    # workgroup 9: XCD 1 (tiles 68 .. 135), second of its 23
    w = M.wanted_walk(M.BY_NAME["walk32x193"])
    assert sorted(set(w.counts)) == [3, 4] and w.counts.index(3) == 772 - 3 * 200
    w = M.wanted_walk(M.BY_NAME["walk64x65"])
    assert set(w.counts) == {5}
    # the rotated power-of-two index against its definition; the generic one is row-major
    w = M.wanted_walk(M.BY_NAME["geo32x128"])
    assert w.tile_pos(16 + 8 + 3) == (1, 1, (27 + 1 + 1) & 7)
    w = M.wanted_walk(M.BY_NAME["geo48x80"])
    assert w.tile_pos(15 + 5 + 2) == (1, 1, 2)
    # refusals of the launcher
    for B, H, W in ((1, 16, 32), (1, 32, 16), (2, 40, 32), (1, 32, 72), (0, 32, 32)):
        assert not M.applies(B, H, W) and M.stat_rows(B, H, W) == 0 and M.scratch_floats(B, H, W) == 0


# ---- the restatements against float64 autograd ----
def _rand(rs, *s):
    return torch.from_numpy(rs.standard_normal(s))


def test_conv_adjoints_against_autograd():
    rs = np.random.RandomState(1)
    a = _rand(rs, 2, C, 32, 48).requires_grad_(True)
    w = _rand(rs, C, C, 3, 3).requires_grad_(True)
    dy = _rand(rs, 2, C, 32, 48)
    ga, gw = torch.autograd.grad(conv_rep(a, w), [a, w], dy)
    assert torch.allclose(M.dgrad_full(dy, w.detach()), ga, rtol=0, atol=1e-12)
    assert torch.allclose(M.wgrad(a.detach(), dy), gw, rtol=0, atol=1e-11)
    (gz,) = torch.autograd.grad(F.conv2d(a, w, padding=1), a, dy)
    assert torch.allclose(M.dgrad_zero(dy, w.detach()), gz, rtol=0, atol=1e-12)
    fold = M.dgrad_full(dy, w.detach()) - M.dgrad_zero(dy, w.detach())
    assert bool((fold[:, :, ~M.edge_mask(32, 48)] == 0).all()) and bool((fold[:, :, M.edge_mask(32, 48)] != 0).any())
    assert torch.allclose(M.dgrad_full(dy, w.detach()), R.conv3_rep_dgrad(dy, w.detach()), rtol=0, atol=1e-12)


def test_pool_and_outlay_adjoints_against_autograd():
    rs = np.random.RandomState(2)
    t = _rand(rs, 2, C, 32, 48).requires_grad_(True)
    gp = _rand(rs, 2, C, 16, 24)
    (g,) = torch.autograd.grad(F.avg_pool2d(t, 2, 2), t, gp)
    assert torch.equal(M.pool_adjoint(gp), g)
    w_out = _rand(rs, 1, C, 3, 3)
    dsr = _rand(rs, 2, 32, 48)
    (g,) = torch.autograd.grad(conv_rep(t, w_out), t, dsr.unsqueeze(1))
    assert torch.allclose(M.outlay_adjoint(dsr, w_out), g, rtol=0, atol=1e-12)
    # the tile form with its separable clamp adjoint, on every tile (all four borders and both corners of each)
    H, W = 32, 48
    for ty in range(2):
        for tx in range(3):
            gy, gx = ty * 16 - 1 + torch.arange(18), tx * 16 - 1 + torch.arange(18)
            dy_, dx_ = ty * 16 - 2 + torch.arange(20), tx * 16 - 2 + torch.arange(20)
            ins = ((dy_ >= 0) & (dy_ < H)).view(20, 1) & ((dx_ >= 0) & (dx_ < W)).view(1, 20)
            D = dsr[1][dy_.clamp(0, H - 1)][:, dx_.clamp(0, W - 1)] * ins
            got = M.tile_tail_g(D, gy, gx, H, W, w_out)
            oky, okx = (gy >= 0) & (gy < H), (gx >= 0) & (gx < W)
            assert torch.allclose(got[:, oky][:, :, okx], g[1][:, gy[oky]][:, :, gx[okx]], rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", ["c", "d", "e", "f"])
def test_formed_modes_against_autograd_of_the_layer(mode):
    """bn_bwd4 with coef_f from host statistics IS the backward of relu(batch_norm(y)); the whole restatement is the backward of the
    layer (and of pooling / outlay above it)"""
    m = M.MODES[mode]
    rs = np.random.RandomState(3)
    B, H, W = 2, 32, 48
    inp = dict(x=_rand(rs, B, C, H, W).float(), xs=torch.from_numpy(rs.uniform(0.5, 1.5, C)).float(), xsh=(0.3 * _rand(rs, C)).float(),
               w=(0.2 * _rand(rs, C, C, 3, 3)).float(), gamma=torch.from_numpy(rs.uniform(0.5, 1.5, C)).float(), beta=(0.5 * _rand(rs, C)).float(),
               g=_rand(rs, B, C, H, W).float(), gp=_rand(rs, B, C, H // 2, W // 2).float(), dsr=_rand(rs, B, H, W).float(),
               w_out=(0.2 * _rand(rs, 1, C, 3, 3)).float(), addend=_rand(rs, B, C, H, W).float())
    inp["y"], inp["coef_f"] = M.random_coef(inp, mode, False)
    a = M.operand(inp["x"], *((inp["xs"], inp["xsh"]) if m.folded else (None, None))).requires_grad_(True)
    w = inp["w"].double().requires_grad_(True)
    y = conv_rep(a, w)
    z = F.relu(F.batch_norm(y, None, None, inp["gamma"].double(), inp["beta"].double(), training=True, eps=1e-5))
    if m.entry == "tail":
        loss = (conv_rep(z, inp["w_out"].double()) * inp["dsr"].double().unsqueeze(1)).sum()
    elif m.entry == "pool":
        loss = (z * inp["g"].double()).sum() + (F.avg_pool2d(z, 2, 2) * inp["gp"].double()).sum()
    else:
        loss = (z * inp["g"].double()).sum()
    dy, ga, gw = torch.autograd.grad(loss, [y, a, w])
    # (y is stored as fp32 and coef_f as fp32: the statistics are those of the rounded y -- 1e-6 of the maximum, not 1e-12)
    e = M.expected(inp, mode, False)
    for got, ref in ((e["dy"], dy), (e["gin"], ga + (inp["addend"].double() if m.addend else 0.0)), (e["dw"], gw)):
        assert float((got - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    edge = M.edge_mask(H, W)
    assert bool(torch.isnan(e["border"][:, :, ~edge]).all()) and torch.equal(e["border"][:, :, edge], e["dy"][:, :, edge])


@pytest.mark.parametrize("hs", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", list(M.MODES))
def test_tiles_assemble_to_the_image(mode, hs):
    """the tile-level restatement (what the mutations act on) against the image-level one, every tile of geo48x80, bit for bit"""
    case = M.BY_NAME["geo48x80"]
    wk = M.wanted_walk(case)
    inp = M.exact_inputs(case.name)
    e = M.expected(inp, mode, hs, wk)
    dw = torch.zeros(C, C, 3, 3, dtype=F64)
    for (b, ty, tx) in wk.where:
        core, dwt, rows = M.tile_outputs(inp, mode, hs, b, ty, tx)
        assert torch.equal(core, e["main"][b, :, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]), (b, ty, tx)
        dw += dwt
        if rows is not None:
            assert torch.equal(rows, e["tile_rows"][b, ty, tx])
    assert torch.equal(dw, e["dw"])
    if M.MODES[mode].sums:
        assert torch.equal(e["rows_main"].sum(0) + e["rows_border"], e["cols"])


@pytest.mark.parametrize("name", ["geo48", "walk64x33"])
def test_the_bf16_roundings_are_exercised(name):
    """integers below 256 are bf16 numbers: the exact inputs are wide enough that gin passes 256, so the bf16 expectation differs from
    the fp32 one (the first rounding) and, on image-border pixels, from a single rounding of the folded sum (the second)"""
    case = M.BY_NAME[name]
    wk = M.wanted_walk(case)
    inp = M.exact_inputs(name)
    first = second = 0
    for mode in M.MODES:
        e0, e1 = M.expected(inp, mode, False, wk), M.expected(inp, mode, True, wk)
        assert torch.equal(e0["dw"], e1["dw"])                              # coef_f is an input: the bf16 weight gradient is exact as well
        first += int((e0["gin"] != e1["gin"]).sum())
        twice = M.rb(e0["main_pre"] + e0["fold"]) != e1["gin"]
        assert not bool(twice[:, :, ~M.edge_mask(case.H, case.W)].any())
        second += int(twice.sum())
    assert first >= 100 and second >= 1, (first, second)


# ---- the exactness condition and the power of the comparison, per exact case ----
@pytest.mark.parametrize("name,mode", M.PAIRS, ids=lambda v: str(v))
def test_exact_case_is_exact_and_its_comparison_has_power(name, mode):
    case = M.BY_NAME[name]
    wk = M.wanted_walk(case)
    inp = M.exact_inputs(name)
    worst, multiples, final = M.exactness(inp, mode, wk)
    print(f"{name}/{mode}: largest intermediate on the magnitudes 2^{np.log2(max(worst, 1)):.1f}, largest result 2^{np.log2(max(final, 1)):.1f}")
    assert multiples, "an operand is finer than 2^-2"
    assert worst < M.LIMIT, (worst, M.LIMIT)
    assert final < 2.0 ** 24
    for v in inp.values():                                                  # every activation is a bf16 number: both storage modes
        assert torch.equal(R.rb(v), v)
    for hs in (False, True):
        exp = M.expected(inp, mode, hs, wk)
        assert M.first_mismatch(wk, exp, exp) is None
        muts = M.mutants(inp, mode, hs, wk, exp)
        want = 2 + (1 if wk.interior_per_image else 0)
        assert len(muts) >= want
        for what, mut, pos in muts:
            rep = M.first_mismatch(wk, mut, exp)
            assert rep is not None, f"{name}/{mode}/{'bf16' if hs else 'fp32'}: the exact comparison does not see: {what}"
            if pos is not None:
                assert f"image {pos[0]}, tile (ty={pos[1]}, tx={pos[2]})" in rep, (what, rep)
                assert f"workgroup {wk.where[pos][0]}, position {wk.where[pos][1]} " in rep, (what, rep)
                assert ("interior tile" in rep) == wk.interior(pos[1], pos[2])
