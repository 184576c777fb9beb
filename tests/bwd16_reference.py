"""What tests/test_bwd16_walk_gpu.py holds conv3x3_bwd16_kernel (csrc/conv_bwd16.hip) against, and what tests/test_bwd16_walk_host.py
pins on the CPU: a mirror of the launch and of the persistent tile walk, float64 restatements of everything the kernel and the
border-fold kernel behind it compute, the case table, the inputs, the comparison and the mutations that show its power.

Exact cases.  Inputs are small integers (pool_gp multiples of 4, coef_f integers or powers of two), so every fp32 step of the kernel
-- the Winograd transforms, the quarter-integer packed weights, the MFMA sums, bn_bwd4, the tail's FMAs, the border fold -- is exact
and the float64 restatement is matched bit for bit.  That is a CONDITION: `exactness` runs the restatement on the magnitudes of the
inputs and reports the largest intermediate, the host module asserts it below 2^22 (and every operand a multiple of 2^-2) per case.
In bf16 storage the kernel rounds where `expected` rounds: the stored border dL/dy, gin after the main kernel (+ addend), and the
image-border pixels once more after the fold.

Random cases.  N(0,1) operands, the layer's own raw output as y, coef_f from float64 batch statistics on the host."""
from collections import namedtuple
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import storage_reference as R

C = 16
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the launch (conv3x3_bwd16_applies, conv3x3_bwd16_grid, launch_conv3x3_bwd16, dgrad_border_waves) and of the walk
# ---------------------------------------------------------------------------------------------------------------------------
def applies(B, H, W):
    return B >= 1 and H >= 32 and W >= 32 and H % 16 == 0 and W % 16 == 0 and B * H * W * 64 < (1 << 32) - 4096


def grid(B, H, W):
    ntiles = B * (H // 16) * (W // 16)
    gmax = 256
    if ntiles <= gmax:
        return ntiles
    rounds = (ntiles + gmax - 1) // gmax
    g = (ntiles + rounds - 1) // rounds
    g = (g + 7) & ~7
    return min(g, ntiles)


def border_waves(B, H, W):
    return B * (2 * ((W + 15) // 16) + 2 * ((H - 2 + 15) // 16))


def stat_rows(B, H, W):
    return grid(B, H, W) + border_waves(B, H, W) if applies(B, H, W) else 0


def scratch_floats(B, H, W):
    return grid(B, H, W) * 9 * 256 if applies(B, H, W) else 0


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def _lg(v):
    l = 0
    while (1 << l) < v:
        l += 1
    return l


class Walk:
    """tiles[w] = the ordered list of (b, ty, tx) workgroup w walks; where[(b, ty, tx)] = (w, position in its walk)"""

    def __init__(self, B, H, W, unrotated_image=None):
        self.B, self.H, self.W = B, H, W
        self.ty, self.tx = H // 16, W // 16
        self.ntiles = nt = B * self.ty * self.tx
        self.grid = G = grid(B, H, W)
        self.pow2 = _pow2(self.tx) and _pow2(self.ty)
        self.lgx = _lg(self.tx) if self.pow2 else -1
        self.lgy = _lg(self.ty) if self.pow2 else -1
        self.xcd = G % 8 == 0 and nt % 8 == 0
        self.tiles, self.where = [], {}
        for wg in range(G):
            t_lo = (wg % 8) * (nt // 8) if self.xcd else 0
            t_hi = t_lo + nt // 8 if self.xcd else nt
            t_step = G // 8 if self.xcd else G
            t = t_lo + (wg // 8 if self.xcd else wg)
            mine = []
            while t < t_hi:
                pos = self.tile_pos(t, unrotated_image)
                assert pos not in self.where
                self.where[pos] = (wg, len(mine))
                mine.append(pos)
                t += t_step
            self.tiles.append(mine)
        assert len(self.where) == nt                      # every tile is walked exactly once
        self.counts = [len(m) for m in self.tiles]
        self.tmin, self.tmax = min(self.counts), max(self.counts)

    def tile_pos(self, t, unrotated_image=None):
        if self.pow2:
            tyi = (t >> self.lgx) & (self.ty - 1)
            tb = t >> (self.lgx + self.lgy)
            txi = ((t if tb == unrotated_image else t + tyi + tb)) & (self.tx - 1)
        else:
            txi = t % self.tx
            r = t // self.tx
            tyi, tb = r % self.ty, r // self.ty
        return (tb, tyi, txi)

    def interior(self, ty, tx):
        return tx > 0 and ty > 0 and tx + 1 < self.tx and ty + 1 < self.ty

    @property
    def interior_per_image(self):
        return max(self.ty - 2, 0) * max(self.tx - 2, 0)

    def split(self):
        """'one', 'even' or e.g. '3/2' -- how many tiles the workgroups own"""
        if self.tmax == 1:
            return "one"
        return "even" if self.tmin == self.tmax else f"{self.tmax}/{self.tmin}"

    def regime(self):
        return dict(ntiles=self.ntiles, grid=self.grid, stride="XCD" if self.xcd else "plain", index="pow2" if self.pow2 else "generic",
                    lg=(self.lgy, self.lgx), tmin=self.tmin, tmax=self.tmax, interior=self.interior_per_image)

    def describe(self):
        return (f"{self.ntiles} tiles on {self.grid} workgroups ({self.tmin}..{self.tmax} each), {'XCD' if self.xcd else 'plain'} stride, "
                f"{'power-of-two' if self.pow2 else 'generic'} tile index, {self.interior_per_image} interior tiles per image")

    def locate(self, b, y, x):
        ty, tx = y // 16, x // 16
        wg, pos = self.where[(b, ty, tx)]
        return (f"image {b}, tile (ty={ty}, tx={tx}), pixel ({y % 16}, {x % 16}) of the tile, "
                f"{'interior' if self.interior(ty, tx) else 'border'} tile: workgroup {wg}, position {pos} of {self.counts[wg]} in its walk")


# ---------------------------------------------------------------------------------------------------------------------------
# cases.  regime: what the issue's tables state, reproduced by the mirror (test_bwd16_walk_host.py) and asserted before every launch.
# lim: half-widths of the integer ranges of the exact inputs (x, g / dL/dy, y, w, dsr, w_out, addend, pool_gp / 4, shifts), narrower
# where a workgroup sums more tiles or the batch is large, so that the exactness condition holds.
# ---------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name H W B regime lim")
WIDE = dict(x=2, dy=6, g=2, y=2, w=3, dsr=1, wo=1, add=3, gp=1, sh=2)
NARROW = dict(x=1, dy=4, g=1, y=2, w=3, dsr=1, wo=1, add=2, gp=1, sh=1)


def _reg(ntiles, grid_, stride, index, lg, tmin, tmax, interior):
    return dict(ntiles=ntiles, grid=grid_, stride=stride, index=index, lg=lg, tmin=tmin, tmax=tmax, interior=interior)


GEOMETRY_CASES = [
    Case("geo32", 32, 32, 1, _reg(4, 4, "plain", "pow2", (1, 1), 1, 1, 0), WIDE),           # every tile touches two image borders
    Case("geo48", 48, 48, 1, _reg(9, 9, "plain", "generic", (-1, -1), 1, 1, 1), WIDE),      # exactly one interior tile
    Case("geo48x80", 48, 80, 2, _reg(30, 30, "plain", "generic", (-1, -1), 1, 1, 3), WIDE),  # three interior tiles
    Case("geo64", 64, 64, 1, _reg(16, 16, "XCD", "pow2", (2, 2), 1, 1, 4), WIDE),            # rotated index, four interior tiles
    Case("geo32x128", 32, 128, 3, _reg(48, 48, "XCD", "pow2", (1, 3), 1, 1, 0), WIDE),       # lgy = 1, lgx = 3; image index from the shift
]
WALK_CASES = [
    Case("walk32x129", 32, 32, 129, _reg(516, 176, "plain", "pow2", (1, 1), 2, 3, 0), WIDE),     # 3, 2 from workgroup 164 on
    Case("walk64x33", 64, 64, 33, _reg(528, 176, "XCD", "pow2", (2, 2), 3, 3, 4), WIDE),
    Case("walk64x34", 64, 64, 34, _reg(544, 184, "XCD", "pow2", (2, 2), 2, 3, 4), WIDE),         # uneven within each XCD
    Case("walk48x64", 48, 48, 64, _reg(576, 192, "XCD", "generic", (-1, -1), 3, 3, 1), WIDE),
    Case("walk48x57", 48, 48, 57, _reg(513, 176, "plain", "generic", (-1, -1), 2, 3, 1), WIDE),
    Case("walk32x193", 32, 32, 193, _reg(772, 200, "plain", "pow2", (1, 1), 3, 4, 0), NARROW),
    Case("walk64x65", 64, 64, 65, _reg(1040, 208, "XCD", "pow2", (2, 2), 5, 5, 4), NARROW),
]
CASES = GEOMETRY_CASES + WALK_CASES
BY_NAME = {c.name: c for c in CASES}

# modes: (a) stored dL/dy, raw x, no extras; (b) stored dL/dy, folded x, fused sums; (c) dL/dy formed from (g, y, coef_f), border scratch,
# fused sums; (d) as (c), raw x, residual addend, no sums; (e) the pooled entry with sums; (f) the tail entry with sums.
Mode = namedtuple("Mode", "key entry formed folded sums addend")
MODES = {
    "a": Mode("a", "main", False, False, False, False),
    "b": Mode("b", "main", False, True, True, False),
    "c": Mode("c", "main", True, True, True, False),
    "d": Mode("d", "main", True, False, False, True),
    "e": Mode("e", "pool", True, True, True, False),
    "f": Mode("f", "tail", True, True, True, False),
}
# Nothing is thinned out: 12 cases x 6 modes x 2 storage modes.  Two cases that provably run the same code on the same regime do not
# exist in this table -- every case differs from every other in at least one of (tile index form, stride, split, interior tiles),
# and every mode instantiates another kernel or takes another branch of the staging / epilogue code.
PAIRS = [(c.name, m) for c in CASES for m in MODES]


def wanted_walk(case):
    """the mirror's walk of a case, checked against the regime the case was written for: a drifted case fails here, before any launch"""
    wk = Walk(case.B, case.H, case.W)
    assert wk.regime() == case.regime, (case.name, wk.regime(), case.regime)
    return wk


# ---------------------------------------------------------------------------------------------------------------------------
# float64 restatements (NCHW)
# ---------------------------------------------------------------------------------------------------------------------------
def _c(v):
    return v.to(F64).view(1, -1, 1, 1)


def rb(t):
    """round to nearest even to bf16 of values that fp32 holds exactly"""
    return t.float().to(torch.bfloat16).to(F64)


def operand(x, xs, xsh):
    """the forward input a_in = relu(x*xs + xsh), or x itself"""
    return x.to(F64) if xs is None else (x.to(F64) * _c(xs) + _c(xsh)).clamp_min(0.0)


def bn_bwd4(g, y, coef_f):
    """dL/dy = sc*g*[z > 0] + k1*z + k0, z = y*sc + sh (common.h bn_bwd4); coef_f = [sc | sh | k1 | k0]"""
    sc, sh, k1, k0 = (_c(v) for v in coef_f.to(F64).view(4, -1))
    z = y.to(F64) * sc + sh
    return sc * torch.where(z > 0, g.to(F64), torch.zeros((), dtype=F64)) + (k1 * z + k0)


def pool_adjoint(gp):
    """AvgPool2d(2, 2) adjoint: 0.25 * gp[y/2][x/2]"""
    return 0.25 * gp.to(F64).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def fold_pad(p):
    """adjoint of replicate padding by one pixel: (.., H+2, W+2) -> (.., H, W), every padded element added to the pixel it copies"""
    p = p.clone()
    p[..., 1, :] += p[..., 0, :]
    p[..., -2, :] += p[..., -1, :]
    p[..., :, 1] += p[..., :, 0]
    p[..., :, -2] += p[..., :, -1]
    return p[..., 1:-1, 1:-1].contiguous()


def dgrad_zero(dy, w):
    """the main kernel's input gradient: the adjoint of the ZERO-padded conv, out[i, q] = sum_{o,t} w[o,i,t] dy[o, q - t]"""
    return F.conv_transpose2d(dy.to(F64), w.to(F64), padding=1)


def dgrad_full(dy, w):
    """the adjoint of the replicate-padded conv: gradient w.r.t. the padded input, folded back onto the image border"""
    return fold_pad(F.conv_transpose2d(dy.to(F64), w.to(F64), padding=0))


def wgrad(a, dy):
    """dw[o,i,ky,kx] = sum dy[b,o,y,x] * a[b,i,clamp(y+ky-1),clamp(x+kx-1)]"""
    ap = F.pad(a.to(F64), (1, 1, 1, 1), mode="replicate")
    H, W = dy.shape[2:]
    dw = torch.empty(dy.shape[1], a.shape[1], 3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy.to(F64), ap[:, :, ky:ky + H, kx:kx + W])
    return dw


def outlay_adjoint(dsr, w_out):
    """g = input gradient of outlay (Conv2d(16, 1, 3), replicate padding) from dsr (B, H, W), clamp adjoint included"""
    return dgrad_full(dsr.to(F64).unsqueeze(1), w_out)


def edge_mask(H, W):
    e = torch.zeros(H, W, dtype=torch.bool)
    e[0] = e[-1] = True
    e[:, 0] = e[:, -1] = True
    return e


def form_dy(inp, mode):
    """dL/dy (B, 16, H, W) as the kernel stages it inside the image"""
    m = MODES[mode]
    if not m.formed:
        return inp["dy"].to(F64)
    if m.entry == "tail":
        g = outlay_adjoint(inp["dsr"], inp["w_out"])
    else:
        g = inp["g"].to(F64)
        if m.entry == "pool":
            g = g + pool_adjoint(inp["gp"])
    return bn_bwd4(g, inp["y"], inp["coef_f"])


def tile_sums(t):
    """(B, 16, H, W) -> (B, ty, tx, 16): per-tile channel sums"""
    B, Cc, H, W = t.shape
    return t.reshape(B, Cc, H // 16, 16, W // 16, 16).sum((3, 5)).permute(0, 2, 3, 1)


def per_workgroup(walk, per_tile):
    """(B, ty, tx, ...) -> (grid, ...): summed over the tiles the mirror gives each workgroup"""
    out = torch.zeros((walk.grid,) + tuple(per_tile.shape[3:]), dtype=per_tile.dtype)
    for wg, mine in enumerate(walk.tiles):
        for pos in mine:
            out[wg] += per_tile[pos]
    return out


def expected(inp, mode, hs, walk=None, absolute=False):
    """Everything one call returns.  hs: model the bf16 roundings of the storage mode (exact cases); absolute: the same maps on the
    magnitudes of the operands (for the exactness condition; masks kept).
    -> dict(gin, dw, border (NaN off the image border; None in the stored modes), dy, main (gin before the fold, as stored),
            fold, rows_main (grid, 16, 2) with a walk, rows_border (16, 2), cols (16, 2))"""
    m = MODES[mode]
    rnd = rb if hs else (lambda t: t)
    xs, xsh = (inp["xs"], inp["xsh"]) if m.folded else (None, None)
    x = inp["x"].to(F64)
    a = operand(x, xs, xsh)
    w = inp["w"].to(F64)
    dy = form_dy(inp, mode)
    if absolute:
        a, w, dy = a.abs(), w.abs(), dy.abs()
    dy_b = rnd(dy) if m.formed else dy                   # what the border-fold kernel reads: the (bf16) border scratch / the stored tensor
    main = dgrad_zero(dy, w)
    if m.addend:
        main = main + (inp["addend"].to(F64).abs() if absolute else inp["addend"].to(F64))
    main_pre = main
    main = rnd(main)
    fold = dgrad_full(dy_b, w) - dgrad_zero(dy_b, w)      # nonzero on image-border pixels only
    gin = rnd(main + fold)
    out = dict(gin=gin, dw=wgrad(a, dy), dy=dy, main=main, main_pre=main_pre, fold=fold, a=a, border=None)
    H, W = x.shape[2:]
    if m.formed:
        e = edge_mask(H, W)
        out["border"] = torch.where(e.view(1, 1, H, W), dy_b, torch.full((), float("nan"), dtype=F64))
    if m.sums:
        pos = (x * _c(xs) + _c(xsh)) > 0
        xv = x.abs() if absolute else x
        zero = torch.zeros((), dtype=F64)
        dz = torch.where(pos, main, zero)
        dzf = torch.where(pos, fold, zero)
        out["tile_rows"] = torch.stack((tile_sums(dz), tile_sums(dz * xv)), -1)           # (B, ty, tx, 16, 2)
        if walk is not None:
            out["rows_main"] = per_workgroup(walk, out["tile_rows"])
        out["rows_border"] = torch.stack((dzf.sum((0, 2, 3)), (dzf * xv).sum((0, 2, 3))), 1)
        out["cols"] = out["tile_rows"].sum((0, 1, 2)) + out["rows_border"]
    return out


# ---- one tile, as the kernel stages and contracts it (for the mutations, and pinned against the whole-image maps) ----
def tile_tail_g(D, gy, gx, H, W, w_out):
    """g on the 18x18 halo from the 20x20 d loss / d sr window D (zero outside the image), as write_stage forms it: the separable
    clamp adjoint on the 3x3 neighbourhood (12 FMAs), then 36 FMAs per channel quad.  gy, gx: image rows / columns of the halo."""
    ymf, ypf = (gy == 0).to(F64).view(18, 1), (gy == H - 1).to(F64).view(18, 1)
    xmf, xpf = (gx == 0).to(F64).view(1, 18), (gx == W - 1).to(F64).view(1, 18)
    n = [[D[1 + dy:19 + dy, 1 + dx:19 + dx] for dx in (-1, 0, 1)] for dy in (-1, 0, 1)]
    cx = [[xmf * n[d][1] + n[d][2], n[d][1], xpf * n[d][1] + n[d][0]] for d in range(3)]
    S = [None] * 9
    for t in range(3):
        S[0 + t] = ymf * cx[1][t] + cx[2][t]
        S[3 + t] = cx[1][t]
        S[6 + t] = ypf * cx[1][t] + cx[0][t]
    wo = w_out.to(F64).reshape(C, 9)
    return sum(wo[:, t].view(C, 1, 1) * S[t].view(1, 18, 18) for t in range(9))


def _flat_gather(t, b, y0, x0, pitch, scale=1):
    """an 18x18 halo read from the NHWC tensor of t (B, C, h, w) at origin (b, y0, x0) with row pitch `pitch` in place of w: what a
    staging path does that takes another path's pitch.  Indices wrap inside the tensor (the mutation stays a restatement)."""
    Bn, Cc, h, w_ = t.shape
    flat = t.permute(0, 2, 3, 1).reshape(-1, Cc)
    sp = torch.arange(18)
    if scale == 2:                                       # the pooled tensor: low-resolution pixel ((spy + 1) >> 1, (spx + 1) >> 1)
        sy, sx = (sp + 1) >> 1, (sp + 1) >> 1
    else:
        sy, sx = sp, sp
    idx = ((b * h + y0) * w_ + x0) + sy.view(18, 1) * pitch + sx.view(1, 18)
    return flat[idx.reshape(-1) % flat.shape[0]].reshape(18, 18, Cc).permute(2, 0, 1).to(F64)


def tile_stage(inp, mode, b, ty, tx, dsr_from=None, wrong_pitch=None, clamp_halo=False):
    """dL/dy on the 18x18 halo of tile (b, ty, tx), zero outside the image.  Mutations: dsr_from = (b', ty', tx') -- the tail's d loss /
    d sr window of another tile; wrong_pitch = 'g' | 'y' | 'gp' -- that operand gathered with the other resolution's row pitch;
    clamp_halo -- a halo pixel outside the image gets its clamped neighbour's dL/dy."""
    m = MODES[mode]
    H, W = inp["x"].shape[2:]
    gy, gx = ty * 16 - 1 + torch.arange(18), tx * 16 - 1 + torch.arange(18)
    inside = ((gy >= 0) & (gy < H)).view(18, 1) & ((gx >= 0) & (gx < W)).view(1, 18)
    gyc, gxc = gy.clamp(0, H - 1), gx.clamp(0, W - 1)

    def halo(t, name):
        if wrong_pitch == name:
            return _flat_gather(t, b, ty * 16 - 1, tx * 16 - 1, W // 2)
        return t[b][:, gyc][:, :, gxc].to(F64)

    if not m.formed:
        dy = halo(inp["dy"], "g")
    else:
        if m.entry == "tail":
            sb, sty, stx = dsr_from if dsr_from is not None else (b, ty, tx)
            dy_, dx_ = sty * 16 - 2 + torch.arange(20), stx * 16 - 2 + torch.arange(20)
            ins = ((dy_ >= 0) & (dy_ < H)).view(20, 1) & ((dx_ >= 0) & (dx_ < W)).view(1, 20)
            D = inp["dsr"][sb][dy_.clamp(0, H - 1)][:, dx_.clamp(0, W - 1)].to(F64) * ins
            g = tile_tail_g(D, gy, gx, H, W, inp["w_out"])
        else:
            g = halo(inp["g"], "g")
            if m.entry == "pool":
                gp = inp["gp"]
                if wrong_pitch == "gp":
                    q = _flat_gather(gp, b, ty * 8 - 1, tx * 8 - 1, W, scale=2)
                else:
                    q = gp[b][:, gyc >> 1][:, :, gxc >> 1].to(F64)
                g = g + 0.25 * q
        dy = bn_bwd4(g.unsqueeze(0), halo(inp["y"], "y").unsqueeze(0), inp["coef_f"])[0]
    return dy if clamp_halo else dy * inside


def tile_outputs(inp, mode, hs, b, ty, tx, dy_halo=None):
    """(gin core as the main kernel stores it (16, 16, 16), dw contribution (16, 16, 3, 3), statistic sums (16, 2) or None)"""
    m = MODES[mode]
    rnd = rb if hs else (lambda t: t)
    H, W = inp["x"].shape[2:]
    if dy_halo is None:
        dy_halo = tile_stage(inp, mode, b, ty, tx)
    w = inp["w"].to(F64)
    gyc, gxc = (ty * 16 - 1 + torch.arange(18)).clamp(0, H - 1), (tx * 16 - 1 + torch.arange(18)).clamp(0, W - 1)
    xh = inp["x"][b][:, gyc][:, :, gxc].to(F64)
    xs, xsh = (inp["xs"], inp["xsh"]) if m.folded else (None, None)
    ah = operand(xh.unsqueeze(0), xs, xsh)[0]
    core = F.conv_transpose2d(dy_halo.unsqueeze(0), w, padding=1)[0, :, 1:17, 1:17]
    if m.addend:
        core = core + inp["addend"][b, :, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].to(F64)
    core = rnd(core)
    dyc = dy_halo[:, 1:17, 1:17]
    dw = torch.empty(C, C, 3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("ohw,ihw->oi", dyc, ah[:, ky:ky + 16, kx:kx + 16])
    rows = None
    if m.sums:
        xc = xh[:, 1:17, 1:17]
        dz = torch.where((xc * xs.to(F64).view(-1, 1, 1) + xsh.to(F64).view(-1, 1, 1)) > 0, core, torch.zeros((), dtype=F64))
        rows = torch.stack((dz.sum((1, 2)), (dz * xc).sum((1, 2))), 1)
    return core, dw, rows


# ---- the exactness condition ----
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], dtype=F64)     # F(2x2,3x3) input / F(3x3,2x2) input
G3 = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=F64)              # F(2x2,3x3) weights
G2 = torch.tensor([[1, 0], [1, 1], [1, -1], [0, 1]], dtype=F64)                                # F(3x3,2x2) dL/dy patch
AT3 = torch.tensor([[1, .5, .5, 0], [0, .5, -.5, 0], [0, .5, .5, 1]], dtype=F64)               # F(3x3,2x2) output
LIMIT = float(2 ** 22)


def is_multiple(t, q):
    t = t.to(F64) / q
    return bool((t == t.round()).all())


def exactness(inp, mode, walk, chunk=16):
    """-> (largest intermediate magnitude, operands are multiples of 2^-2) with the maps run on the magnitudes of the operands:
    the dgrad transform-domain operands and products per output (|B^T| |dy| |B| against |G w G^T|, summed over the 16 channels),
    gin before rounding, the weight-gradient transform-domain sums and tap-domain slab per WORKGROUP over its walked tiles
    (sum over patches of |G g G^T| . |B^T d B|, then |A^T| . |A|), and the statistic sums per workgroup."""
    e = expected(inp, mode, False, walk, absolute=True)
    ex = expected(inp, mode, False, walk)
    w = inp["w"].to(F64)
    U = torch.einsum("ua,oiab,vb->oiuv", G3, w, G3)
    ok = (is_multiple(U, 0.25) and is_multiple(ex["dy"], 1.0) and is_multiple(ex["a"], 1.0) and is_multiple(ex["main_pre"], 1.0)
          and is_multiple(ex["fold"], 1.0) and is_multiple(ex["dw"], 1.0))
    if MODES[mode].entry == "pool":
        ok = ok and is_multiple(inp["gp"], 4.0)
    dy, a = e["dy"], e["a"]
    B, _, H, W = dy.shape
    worst = float(e["gin"].max())
    # dgrad: the 4x4 window of |dy| under |B^T| . |B| bounds every transformed operand; times sum_o |U| bounds the 64-MFMA sums
    dyp = F.pad(dy, (1, 1, 1, 1))
    win = F.avg_pool2d(dyp, 4, stride=1) * 16.0                                           # sum of |dy| over every 4x4 window
    worst = max(worst, float(win.max()), float(torch.einsum("bohw,oi->bihw", win, U.abs().amax((2, 3))).max()))
    # wgrad: per tile sum over its 64 patches, then per workgroup
    bt, g2, at = BT.abs(), G2.abs(), AT3.abs()
    rows = (2 * torch.arange(H // 2).view(-1, 1) + torch.arange(4).view(1, -1) - 1).clamp(0, H - 1)
    cols = (2 * torch.arange(W // 2).view(-1, 1) + torch.arange(4).view(1, -1) - 1).clamp(0, W - 1)
    per_tile = torch.empty(B, walk.ty, walk.tx, C, C, 16, dtype=F64)
    for b0 in range(0, B, chunk):
        d = a[b0:b0 + chunk][:, :, rows][:, :, :, :, cols]                                # (b, i, PH, 4, PW, 4)
        V = torch.einsum("ur,bcprqs,vs->bcpquv", bt, d, bt)
        gp = dy[b0:b0 + chunk].reshape(-1, C, H // 2, 2, W // 2, 2)
        Ug = torch.einsum("ua,bopaqc,vc->bopquv", g2, gp, g2)
        n = V.shape[0]
        V = V.reshape(n, C, walk.ty, 8, walk.tx, 8, 16)
        Ug = Ug.reshape(n, C, walk.ty, 8, walk.tx, 8, 16)
        per_tile[b0:b0 + chunk] = torch.einsum("boypxqk,bcypxqk->byxock", Ug, V)
    M = per_workgroup(walk, per_tile)                                                     # (grid, o, c, 16)
    slab = torch.einsum("iu,gocuv,jv->gocij", at, M.reshape(walk.grid, C, C, 4, 4), at)
    worst = max(worst, float(M.max()), float(slab.max()))
    if "rows_main" in e:
        worst = max(worst, float(e["rows_main"].max()), float(e["rows_border"].max()))
    # what leaves the reduction as fp32 has to be exact as well: the ACTUAL weight gradient and column sums
    final = float(ex["dw"].abs().max())
    if "cols" in ex:
        final = max(final, float(ex["cols"].abs().max()))
    return worst, ok, final


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _seed(name, salt):
    import zlib
    return zlib.crc32(f"{name}/{salt}".encode()) & 0x7FFFFFFF


def _ints(rs, shape, lim):
    return torch.from_numpy(rs.randint(-lim, lim + 1, size=shape).astype(np.float32))


@functools.lru_cache(maxsize=2)
def exact_inputs(name):
    """small-integer operands of a case (float32 NCHW; every value a bf16 number).  Each tile's values are their own draw, so no two
    tiles agree.  coef_f is made by hand: sc in {1, 2}, sh and k0 integers, k1 in {-1, 0, 1}, or +-1/2 where z = 2y + (even sh) is even."""
    c = BY_NAME[name]
    rs = np.random.RandomState(_seed(name, "exact"))
    B, H, W, L = c.B, c.H, c.W, c.lim
    sc = rs.randint(1, 3, C).astype(np.float64)
    sh = rs.randint(-L["sh"], L["sh"] + 1, C).astype(np.float64)
    k1 = rs.randint(-1, 2, C).astype(np.float64)
    half = (sc == 2) & (sh % 2 == 0)
    k1 = np.where(half & (rs.randint(0, 2, C) == 1), 0.5 * np.where(k1 == 0, 1.0, k1), k1)
    k0 = rs.randint(-L["sh"], L["sh"] + 1, C).astype(np.float64)
    inp = dict(
        x=_ints(rs, (B, C, H, W), L["x"]), xs=torch.from_numpy(rs.randint(1, 3, C).astype(np.float32)), xsh=_ints(rs, (C,), L["sh"]),
        w=_ints(rs, (C, C, 3, 3), L["w"]), dy=_ints(rs, (B, C, H, W), L["dy"]), g=_ints(rs, (B, C, H, W), L["g"]),
        y=_ints(rs, (B, C, H, W), L["y"]), gp=4.0 * _ints(rs, (B, C, H // 2, W // 2), L["gp"]), dsr=_ints(rs, (B, H, W), L["dsr"]),
        w_out=_ints(rs, (1, C, 3, 3), L["wo"]), addend=_ints(rs, (B, C, H, W), L["add"]),
        coef_f=torch.from_numpy(np.concatenate((sc, sh, k1, k0)).astype(np.float32)))
    return inp


@functools.lru_cache(maxsize=2)
def random_inputs(name, hs):
    """N(0,1) operands as test_conv3x3_bwd16_fused_dgrad_wgrad draws them; y = the layer's own raw output (as stored), coef_f per
    mode from float64 batch statistics on the host (`random_coef`).  hs: every activation tensor holds bf16 values."""
    c = BY_NAME[name]
    rs = np.random.RandomState(_seed(name, "random"))
    B, H, W = c.B, c.H, c.W
    st = (lambda t: R.rb(t)) if hs else (lambda t: t)
    rnd = lambda *s, scale=1.0: torch.from_numpy((rs.standard_normal(s) * scale).astype(np.float32))
    uni = lambda: torch.from_numpy(rs.uniform(0.5, 1.5, C).astype(np.float32))
    inp = dict(x=st(rnd(B, C, H, W)), xs=uni(), xsh=rnd(C, scale=0.3), w=rnd(C, C, 3, 3, scale=(2.0 / (9 * C)) ** 0.5),
               gamma=uni(), beta=rnd(C, scale=0.5), dy=st(rnd(B, C, H, W)), g=st(rnd(B, C, H, W)), gp=st(rnd(B, C, H // 2, W // 2)),
               dsr=rnd(B, H, W), w_out=rnd(1, C, 3, 3, scale=0.2), addend=st(rnd(B, C, H, W)))
    return inp


def random_coef(inp, mode, hs):
    """y (as stored) and coef_f (fp32 of the float64 values) of a formed mode: BatchNorm(training) statistics of y, then the sums of
    the BatchNorm+ReLU backward over the mode's upstream gradient, all in float64 on the host."""
    m = MODES[mode]
    xs, xsh = (inp["xs"], inp["xsh"]) if m.folded else (None, None)
    y = R.conv3_rep(operand(inp["x"], xs, xsh), inp["w"]).float()
    if hs:
        y = R.rb(y)
    y64 = y.to(F64)
    n = y64.shape[0] * y64.shape[2] * y64.shape[3]
    mean, var = y64.mean((0, 2, 3)), y64.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = inp["gamma"].to(F64) * invstd
    shift = inp["beta"].to(F64) - mean * scale
    scale, shift = scale.float(), shift.float()          # what the device holds
    if m.entry == "tail":
        g = outlay_adjoint(inp["dsr"], inp["w_out"])
    else:
        g = inp["g"].to(F64) + (pool_adjoint(inp["gp"]) if m.entry == "pool" else 0.0)
    z = y64 * _c(scale) + _c(shift)
    dz = torch.where(z > 0, g, torch.zeros((), dtype=F64))
    xhat = (y64 - _c(mean)) * _c(invstd)
    _, _, coef_f, _ = R.coef_from_sums(dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3)), scale, shift, mean, invstd, inp["beta"], n)
    return y, coef_f.float()


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """elementwise: equal as numbers (so +0 == -0), or both NaN"""
    a, b = a.to(F64), b.to(F64)
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def first_mismatch(walk, got, exp):
    """None, or the report of the first difference between what a call returned and `expected`: for the image-shaped outputs the
    first wrong image, tile, pixel within it, whether the tile is interior, and the workgroup and walk position from the mirror."""
    for key in ("gin", "border"):
        if exp.get(key) is None:
            continue
        bad = ~same_bits(got[key], exp[key])
        if bool(bad.any()):
            b, ch, y, x = (int(v) for v in bad.nonzero()[0])
            n_tiles = int(tile_sums(bad.to(F64)).sum(-1).gt(0).sum())
            return (f"{key}: {walk.locate(b, y, x)}; channel {ch}: got {float(got[key][b, ch, y, x])!r}, expected "
                    f"{float(exp[key][b, ch, y, x])!r}; {int(bad.sum())} elements in {n_tiles} tiles differ")
    if "rows_main" in exp and "rows_main" in got:
        bad = ~same_bits(got["rows_main"], exp["rows_main"])
        if bool(bad.any()):
            wg, ch, k = (int(v) for v in bad.nonzero()[0])
            return (f"statistic row of workgroup {wg} (tiles {walk.tiles[wg]}), channel {ch}, {'sum dz*y' if k else 'sum dz'}: got "
                    f"{float(got['rows_main'][wg, ch, k])!r}, expected {float(exp['rows_main'][wg, ch, k])!r}; "
                    f"{int(bad.any(-1).any(-1).sum())} rows differ")
    for key in ("rows_border", "cols", "dw"):
        if key in exp and key in got:
            bad = ~same_bits(got[key], exp[key])
            if bool(bad.any()):
                i = tuple(int(v) for v in bad.nonzero()[0])
                return f"{key}{list(i)}: got {float(got[key][i])!r}, expected {float(exp[key][i])!r}; {int(bad.sum())} elements differ"
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# mutations of the restatement: each returns (name, mutated copy of `exp`, (b, ty, tx) or None) -- what a kernel with that slip returns
# ---------------------------------------------------------------------------------------------------------------------------
def _with_tile(inp, mode, hs, walk, exp, pos, dy_halo):
    """`exp` with tile `pos` contracted from another staged dL/dy halo (the fold is left alone: it reads the border scratch)"""
    b, ty, tx = pos
    core0, dw0, rows0 = tile_outputs(inp, mode, hs, b, ty, tx)
    core1, dw1, rows1 = tile_outputs(inp, mode, hs, b, ty, tx, dy_halo)
    out = dict(exp)
    rnd = rb if hs else (lambda t: t)
    sl = (b, slice(None), slice(ty * 16, ty * 16 + 16), slice(tx * 16, tx * 16 + 16))
    out["gin"] = exp["gin"].clone()
    out["gin"][sl] = rnd(core1 + exp["fold"][sl])
    out["dw"] = exp["dw"] - dw0 + dw1
    if rows0 is not None:
        wg = walk.where[pos][0]
        out["rows_main"] = exp["rows_main"].clone()
        out["rows_main"][wg] += rows1 - rows0
        out["cols"] = exp["cols"] + rows1 - rows0
    return out


def mutants(inp, mode, hs, walk, exp):
    m = MODES[mode]
    out = []
    deep = max(range(walk.grid), key=lambda w: walk.counts[w])          # a workgroup with the longest walk
    tiles_i = [p for mine in walk.tiles for p in mine if walk.interior(p[1], p[2])]
    tiles_b = [p for mine in walk.tiles for p in mine if not walk.interior(p[1], p[2])]
    if m.entry == "tail":
        for ahead in (1, 2):                                            # the dtl slot confusion
            if walk.counts[deep] > ahead:
                pos, src = walk.tiles[deep][0], walk.tiles[deep][ahead]
                out.append((f"dsr of the tile {ahead} ahead", _with_tile(inp, mode, hs, walk, exp, pos, tile_stage(inp, mode, *pos, dsr_from=src)), pos))
    if tiles_i:
        pos = tiles_i[len(tiles_i) // 2]
        names = (["g"] if m.entry != "tail" else []) + (["y"] if m.formed else []) + (["gp"] if m.entry == "pool" else [])
        for nm in names:
            out.append((f"{nm} of an interior tile with the wrong row pitch",
                        _with_tile(inp, mode, hs, walk, exp, pos, tile_stage(inp, mode, *pos, wrong_pitch=nm)), pos))
    pos = walk.tiles[deep][-1]
    _, dw0, rows0 = tile_outputs(inp, mode, hs, *pos)
    e = dict(exp); e["dw"] = exp["dw"] - dw0
    out.append(("one tile missing from dw", e, None))
    if m.sums:
        e = dict(exp); e["rows_main"] = exp["rows_main"].clone(); e["rows_main"][deep] += rows0; e["cols"] = exp["cols"] + rows0
        out.append(("one tile counted twice in the statistic sums", e, None))
        if walk.pow2:
            b = walk.B // 2
            e = dict(exp); e["rows_main"] = per_workgroup(Walk(walk.B, walk.H, walk.W, unrotated_image=b), exp["tile_rows"])
            out.append(("tx left unrotated for one image", e, None))
    pos = tiles_b[len(tiles_b) // 2]
    out.append(("an out-of-image halo pixel with its clamped neighbour's dL/dy",
                _with_tile(inp, mode, hs, walk, exp, pos, tile_stage(inp, mode, *pos, clamp_halo=True)), pos))
    return out
