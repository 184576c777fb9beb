"""The 3x3 weight-gradient path (csrc/conv_wgrad.hip, csrc/conv_wgrad_wino.hip, wgrad_reduce_kernel<EL>) restated for the edge
tests: a mirror of the launch geometry, the float64 references with their yardsticks, the case table the GPU file runs, and the
mutations the bar must reject.  Plain Python, float64 on the CPU, NCHW; no measured constant.

Mirror (what cannot be observed from outside other than through the results): the 8x16-pixel tile grid, nblk clamped to the tile
count, which tiles a workgroup walks (tile, tile + nblk, ...), the tile index form (shifts and masks when both tile counts are
powers of two, % and / otherwise), which tiles take the interior path (one scalar offset, no clamps), which are partial, the Cin
chunking of both kernel families, the (NBO, NBI) template variant or the shape error, and EL / the group count of the reduction.

Reference and yardstick per form (the bar is storage_reference.BAR_SUM per element against the yardstick of the form under test):
  tap         conv3_rep_wgrad(a, dy)            against  conv3_rep_wgrad(|a|, |dy|)
  fused       dy = bn_bwd(g, y, ...)["dy"]      against  conv3_rep_wgrad(|a|, bn_bwd(...)["dy_abs"])
  bf16        a, dy = the values the bf16 tensors hold (rb); with a folded BatchNorm+ReLU the operand is the fp32 fma, ReLU'd and
              rounded to bf16 as the kernel rounds it when it feeds the matrix core.  Products of bf16 values are exact in fp32.
  wino        the same reference; yardstick |A^T| [ sum_P (|G| |g_P| |G^T|) . (|B^T| |d_P| |B|) ] |A| -- F(3x3, 2x2) of the kernel
              header in float64 with the absolute value of every transform matrix and operand: what the fp32 rounding of the
              Winograd algorithm scales with."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

from tests import storage_reference as R

ERR_SHAPE, ERR_ARG = 1001, 1002
TILE_H, TILE_W = 8, 16


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the launch geometry
# ---------------------------------------------------------------------------------------------------------------------------
def tile_grid(H, W):
    """(tiles_y, tiles_x): the last row / column of tiles may be partial"""
    return (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def tap_nbi_chunk(C0, C1):
    """wgrad_nbi_chunk: 16-channel blocks per Cin chunk of the tap kernels.  A chunk never straddles the two sources and the
    chunks tile Cin exactly."""
    cin = C0 + C1
    if cin < 32 or (cin // 16) % 2:
        return 1
    if C1 and (C0 // 16) % 2:
        return 1
    return 2


def wino_nbi_chunk(cin):
    """wgrad_wino_nbi_chunk: a 32-channel chunk may straddle the two sources (cat(16, 16))"""
    return 1 if (cin < 32 or (cin // 16) % 2) else 2


TAP_VARIANTS = ((1, 1), (1, 2), (2, 1), (2, 2), (4, 2))
WINO_VARIANTS = ((1, 1, 1), (1, 2, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2))     # (NBO, NBI, halves): 64 outputs run as two halves of 32


def tap_variant(C0, C1, cout):
    """-> (NBO, NBI, chunks), or None where launch_conv3x3_wgrad returns SIFSR_ERR_SHAPE before any launch"""
    cin = C0 + C1
    if cin % 16 or cout % 16 or not _pow2(C0) or (C1 and not _pow2(C1)):
        return None
    nbi, nbo = tap_nbi_chunk(C0, C1), cout // 16
    if (cin // 16) % nbi or (nbo, nbi) not in TAP_VARIANTS:
        return None
    return nbo, nbi, (cin // 16) // nbi


def wino_variant(C0, C1, cout, H, W):
    """-> (NBO, NBI, halves, chunks) of the Winograd kernel, or None (SIFSR_ERR_SHAPE: odd size, no such variant)"""
    cin = C0 + C1
    if H < 2 or W < 2 or H % 2 or W % 2 or cin % 16 or cout % 16 or not _pow2(C0) or (C1 and not _pow2(C1)):
        return None
    nbi, nbo = wino_nbi_chunk(cin), cout // 16
    if (cin // 16) % nbi:
        return None
    for vo, vi, halves in WINO_VARIANTS:
        if nbo == vo * halves and nbi == vi:
            return vo, vi, halves, (cin // 16) // nbi
    return None


def wino_straddles(C0, C1):
    """does a 32-channel chunk of the Winograd kernel take one block from each source?"""
    nbi = wino_nbi_chunk(C0 + C1)
    return nbi == 2 and C1 > 0 and (C0 // 16) % 2 == 1


def reduce_el(cin, cout):
    """(EL, groups): slab elements per workgroup of wgrad_reduce_kernel<EL> and its 256 / EL slab groups"""
    n = 9 * cin * cout
    el = 4 if n <= 2304 else 8 if n <= 4608 else 16 if n <= 9216 else 32
    return el, 256 // el


class Launch:
    """One weight-gradient launch over B images of H x W with `nblk` requested workgroups (per Cin chunk)."""

    def __init__(self, B, H, W, nblk):
        self.B, self.H, self.W = B, H, W
        ty, tx = tile_grid(H, W)
        self.ty, self.tx = ty, tx
        self.ntiles = nt = B * ty * tx
        self.nblk = g = min(nblk, nt)
        self.pow2 = _pow2(tx) and _pow2(ty)                      # lgx >= 0
        lgx, lgy = tx.bit_length() - 1, ty.bit_length() - 1
        self.where, self.counts = {}, []
        self.kinds = {"interior": 0, "border": 0, "partial": 0}  # border = full tile on the clamped path; partial tiles clamp too
        for wg in range(g):
            t, r = wg, 0
            while t < nt:
                if self.pow2:
                    txi = t & (tx - 1); tyi = (t >> lgx) & (ty - 1); b = t >> (lgx + lgy)
                else:
                    txi = t % tx; q = t // tx; tyi = q % ty; b = q // ty
                assert (b, tyi, txi) not in self.where and b < B
                self.where[(b, tyi, txi)] = (r, wg)
                self.kinds[self.kind(tyi, txi)] += 1
                t += g; r += 1
            self.counts.append(r)
        assert len(self.where) == nt                             # every tile is walked exactly once
        self.tmin, self.tmax = min(self.counts), max(self.counts)

    def kind(self, tyi, txi):
        if txi > 0 and tyi > 0 and txi + 1 < self.tx and tyi + 1 < self.ty:
            return "interior"                                    # (an interior tile is always full)
        full = txi * TILE_W + TILE_W <= self.W and tyi * TILE_H + TILE_H <= self.H
        return "border" if full else "partial"

    def terms_per_workgroup(self):
        """products one workgroup accumulates per weight element: 128 pixels per tile it walks"""
        return self.tmax * TILE_H * TILE_W

    def describe(self):
        k = self.kinds
        return (f"{self.ntiles} tiles ({self.ty}x{self.tx} per image: {k['interior']} interior, {k['border']} border, {k['partial']} "
                f"partial) on {self.nblk} workgroups, {self.tmin}..{self.tmax} tiles each, "
                f"{'power-of-two' if self.pow2 else 'generic'} tile index")


def worst_element(got, ref, yard, C0, C1):
    """where the largest error / yardstick sits, in the kernels' terms: for a failure message"""
    ratio = (got.double() - ref).abs() / yard.clamp_min(1e-300)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    cin = C0 + C1
    co, ci, t = i // (9 * cin), (i // 9) % cin, i % 9
    blk = ci // 16
    return (f"dw[{co}][{ci}][{t // 3}][{t % 3}] (cout block {co // 16}; cin block {blk} = source {0 if blk < C0 // 16 else 1}, tap chunk "
            f"{blk // tap_nbi_chunk(C0, C1)}, Winograd chunk {blk // wino_nbi_chunk(cin)}): got {float(got.flatten()[i]):.9g}, "
            f"reference {float(ref.flatten()[i]):.9g}, yardstick {float(yard.flatten()[i]):.6g}; "
            f"{int((ratio > R.BAR_SUM).sum())} of {ratio.numel()} elements over the bar")


def nblk_values(ntiles, groups):
    """{label: requested workgroup count}: the counts a case is launched with, as far as its tile count allows them"""
    v = {"one": 1, "ntiles": ntiles, "clamped": ntiles + 5}
    uneven = [n for n in range(2, ntiles) if ntiles % n]
    if uneven:
        v["uneven"] = uneven[0]
    if 2 <= min(3, ntiles - 1) < groups:
        v["below_groups"] = min(3, ntiles - 1)
    if groups + 3 < ntiles:
        v["ragged_groups"] = groups + 3                          # above the group count and no multiple of it
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], dtype=torch.float64)
G = torch.tensor([[1, 0], [1, 1], [1, -1], [0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, .5, .5, 0], [0, .5, -.5, 0], [0, .5, .5, 1]], dtype=torch.float64)


def wino_wgrad(a, g, absolute=False):
    """dW = A^T [ sum_P (G g_P G^T) . (B^T d_P B) ] A over the 2x2 output patches P of an even-sized image, d_P the replicate-
    clamped 4x4 input window of the patch.  absolute: every matrix and operand by its absolute value (the yardstick)."""
    a, g = a.double(), g.double()
    H, W = a.shape[2:]
    assert H % 2 == 0 and W % 2 == 0 and H >= 2 and W >= 2
    bt, gm, at = (BT, G, AT) if not absolute else (BT.abs(), G.abs(), AT.abs())
    if absolute:
        a, g = a.abs(), g.abs()
    rows = (2 * torch.arange(H // 2).view(-1, 1) + torch.arange(4).view(1, -1) - 1).clamp(0, H - 1)      # [PH, 4]
    cols = (2 * torch.arange(W // 2).view(-1, 1) + torch.arange(4).view(1, -1) - 1).clamp(0, W - 1)
    d = a[:, :, rows][:, :, :, :, cols]                                                                  # [B, Ci, PH, 4, PW, 4]
    V = torch.einsum("ur,bcprqs,vs->bcpquv", bt, d, bt)
    gp = g.reshape(g.shape[0], g.shape[1], H // 2, 2, W // 2, 2)
    U = torch.einsum("ua,bopaqc,vc->bopquv", gm, gp, gm)
    n = U.shape[0] * U.shape[2] * U.shape[3]
    M = torch.einsum("onk,cnk->ock", U.permute(1, 0, 2, 3, 4, 5).reshape(U.shape[1], n, 16),
                     V.permute(1, 0, 2, 3, 4, 5).reshape(V.shape[1], n, 16)).reshape(U.shape[1], V.shape[1], 4, 4)
    return torch.einsum("iu,ocuv,jv->ocij", at, M, at)


def operand(xs, scs, shs, bf16=False):
    """the convolution's input as the kernels stage it: per source relu(x*sc + sh) (or x itself), concatenated -> (a, |a|).
    bf16: x holds bf16 values; the fp32 fma result is ReLU'd and rounded to bf16 when it feeds the matrix core."""
    parts = []
    for x, sc, sh in zip(xs, scs, shs):
        a, _ = R.bnrelu(x, sc, sh)
        parts.append(R.rb(a.float()).double() if bf16 else a)
    a = torch.cat(parts, 1)
    return a, a.abs()


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
# aff: one letter per source, "a" = folded BatchNorm+ReLU (scale, shift), "-" = stored activations (already post-ReLU)
Case = namedtuple("Case", "C0 C1 cout aff B H W")

# channel configurations: name -> (C0, C1, cout, aff).  Tap variant (NBO, NBI) / Winograd variant / EL in the comments.
CONFIGS = {
    "16>16": (16, 0, 16, "a"),          # (1,1) / (1,1) / EL 4
    "32>16": (32, 0, 16, "-"),          # (1,2) / (1,2) / EL 8, single raw source
    "16>32": (16, 0, 32, "a"),          # (2,1) / (2,1) / EL 8
    "32>32": (32, 0, 32, "a"),          # (2,2) / (2,2) / EL 16
    "64>64": (64, 0, 64, "a"),          # (4,2) / two halves of (2,2) / EL 32
    "32>64": (32, 0, 64, "-"),          # (4,2), one chunk
    "32+32>32": (32, 32, 32, "aa"),     # (2,2), the second chunk is the second source
    "64+64>64": (64, 64, 64, "a-"),     # (4,2) / halves, four chunks
    "16+16>16": (16, 16, 16, "aa"),     # tap nbi 1: (1,1); Winograd (1,2) with the chunk straddling the sources
    "16+16>32": (16, 16, 32, "-a"),     # tap (2,1); Winograd (2,2) straddling
    "64+32>32": (64, 32, 32, "aa"),     # C0 != C1: the shift lgc differs per source; (2,2), three chunks
    "16+32>16": (16, 32, 16, "-a"),     # C0 != C1, affine on the second only; odd block count: nbi 1 in both families
    "16+64>32": (16, 64, 32, "aa"),     # C0 != C1; five blocks: (2,1)
}
# cat(32, 16): the block count is odd while the first source's is even -- the chunking once rounded the last block away
GUARD_CONFIGS = {"32+16>16": (32, 16, 16, "aa"), "32+16>32": (32, 16, 32, "a-")}

MAIN_SHAPES = [(3, 20, 40), (3, 32, 64), (1, 30, 60)]
SMALL_SHAPES = [(1, 8, 16), (3, 10, 18), (3, 6, 14), (3, 2, 2), (1, 2, 18), (3, 10, 2)]
MORE_SHAPES = [(1, 24, 48), (3, 30, 60), (3, 8, 16)]
TAP_ONLY_SHAPES = [(3, 1, 1), (1, 1, 17), (3, 9, 1), (1, 7, 15), (3, 9, 17), (1, 21, 37)]


def _cases():
    out = []
    names = list(CONFIGS)
    for i, name in enumerate(names):
        cfg = CONFIGS[name]
        shapes = list(MAIN_SHAPES) + [SMALL_SHAPES[(2 * i) % len(SMALL_SHAPES)], SMALL_SHAPES[(2 * i + 1) % len(SMALL_SHAPES)]]
        shapes.append(MORE_SHAPES[i % len(MORE_SHAPES)])
        shapes.append(TAP_ONLY_SHAPES[i % len(TAP_ONLY_SHAPES)])
        if i < len(TAP_ONLY_SHAPES) - 1:
            shapes.append(TAP_ONLY_SHAPES[(i + 3) % len(TAP_ONLY_SHAPES)])
        out += [Case(*cfg, *s) for s in shapes]
    # 68 tiles: the only way to more workgroups than the 64 slab groups of EL = 4 within 8192 pixels
    out.append(Case(*CONFIGS["16>16"], 17, 10, 18))
    out.append(Case(*CONFIGS["16>32"], 1, 32, 64))               # B = 1 on the power-of-two grid: image index 0 from the shift
    return out


CASES = _cases()
GUARD_CASES = [Case(*cfg, *s) for cfg in GUARD_CONFIGS.values() for s in ((3, 20, 40), (1, 10, 18))]
GUARD_WINO_CASES = [Case(*CONFIGS["16+32>16"], 3, 20, 40), Case(16, 32, 32, "aa", 1, 10, 18)]


def case_id(c):
    return f"{c.C0}+{c.C1}>{c.cout}-{c.aff}-B{c.B}-{c.H}x{c.W}"


def forms_of(c):
    """the entry points a case runs through"""
    f = []
    if tap_variant(c.C0, c.C1, c.cout):
        f += ["tap", "fused", "bf16"]
    if wino_variant(c.C0, c.C1, c.cout, c.H, c.W):
        f += ["wino", "wino_fused"]
    return f


def _rng(c):
    return np.random.RandomState(zlib.crc32(repr(tuple(c)).encode()) % 2**31)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


class Data:
    """Inputs of a case (float32, NCHW) and, per form, what the kernel is given and what it must return."""

    def __init__(self, c):
        self.c = c
        rs = _rng(c)
        B, H, W, cout = c.B, c.H, c.W, c.cout
        self.xs, self.scs, self.shs = [], [], []
        for C, aff in zip((c.C0, c.C1), c.aff):
            if not C:
                continue
            x = _f32(rs.standard_normal((B, C, H, W)))
            sc, sh = _f32(rs.uniform(0.5, 1.5, C)), _f32(0.3 * rs.standard_normal(C) + 0.2)
            if aff == "a":
                self.xs.append(x); self.scs.append(sc); self.shs.append(sh)
            else:      # a stored activation: post-ReLU values
                self.xs.append(R.bnrelu(x, sc, sh)[0].float()); self.scs.append(None); self.shs.append(None)
        self.dy = _f32(rs.standard_normal((B, cout, H, W)))
        # the layer's own BatchNorm + ReLU backward: upstream gradient g on relu(bn(y)), raw conv output y
        self.g = _f32(rs.standard_normal((B, cout, H, W)))
        self.y = _f32(1.5 * rs.standard_normal((B, cout, H, W)) + 0.4)
        gamma, beta = _f32(rs.uniform(0.5, 1.5, cout)), _f32(0.5 * rs.standard_normal(cout))
        n = B * H * W
        self.mean = self.y.double().mean((0, 2, 3)).float()
        self.invstd = (1.0 / torch.sqrt(self.y.double().var((0, 2, 3), unbiased=False) + 1e-5)).float()
        self.scale = gamma * self.invstd
        self.shift = beta - self.mean * self.scale
        self.bn = R.bn_bwd(self.g, self.y, self.scale, self.shift, self.mean, self.invstd)
        _, _, coef_f, _ = R.coef_from_sums(self.bn["dbeta"], self.bn["dgamma"], self.scale, self.shift, self.mean, self.invstd, beta, n)
        self.coef_f = coef_f.float()                             # [sc | sh | k1f | k0f], what the finalize kernels leave
        self._forms = {}

    def inputs(self, form):
        """(xs, dy-or-g) as the device tensors of `form` hold them"""
        if form == "bf16":
            return [R.rb(x) for x in self.xs], R.rb(self.dy)
        return self.xs, (self.g if form in ("fused", "wino_fused") else self.dy)

    def operands(self, form, scs=None, shs=None):
        """float64 (a, |a|, dy, |dy|) of `form`; scs / shs: other affines than the case's (a mutation)"""
        scs = self.scs if scs is None else scs
        shs = self.shs if shs is None else shs
        xs, dyv = self.inputs(form)
        a, a_abs = operand(xs, scs, shs, bf16=form == "bf16")
        if form in ("fused", "wino_fused"):
            return a, a_abs, self.bn["dy"], self.bn["dy_abs"]
        return a, a_abs, dyv.double(), dyv.double().abs()

    def expect(self, form):
        """(reference, yardstick), float64 [cout, cin, 3, 3]"""
        if form not in self._forms:
            base = {"wino": "tap", "wino_fused": "fused"}.get(form)
            a, a_abs, dyv, dy_abs = self.operands(form)
            if base is None:
                self._forms[form] = (R.conv3_rep_wgrad(a, dyv), R.conv3_rep_wgrad(a_abs, dy_abs))
            else:
                self._forms[form] = (self.expect(base)[0], wino_wgrad(a_abs, dy_abs, absolute=True))
        return self._forms[form]


@functools.lru_cache(maxsize=4)
def data(c):
    return Data(c)


# ---------------------------------------------------------------------------------------------------------------------------
# mutations: what a subtly wrong kernel would return
# ---------------------------------------------------------------------------------------------------------------------------
def _tap_outer(gvec, a, b, y, x):
    """[cout, cin, 3, 3] contribution of a dy vector sitting at pixel (y, x) of image b (the pixel may lie outside the image: the
    halo it meets is clamped)"""
    H, W = a.shape[2:]
    ys, xs = (torch.arange(3) + y - 1).clamp(0, H - 1), (torch.arange(3) + x - 1).clamp(0, W - 1)
    return gvec.view(-1, 1, 1, 1) * a[b][:, ys][:, :, xs].unsqueeze(0)


def mutants(d, form):
    """(name, float64 gradient) of every mutation that applies to the case: each differs from the reference as a kernel with that
    defect would.  Not applicable: a clamp to the wrong side where both sides are the same pixel (1x1); the second source's affine
    without a second source or without any affine; an out-of-image pixel where every tile is full or the stray address lies
    beyond the tensor."""
    c = d.c
    ref, _ = d.expect(form)
    a, _, dyv, _ = d.operands(form)
    B, H, W = c.B, c.H, c.W
    # one dropped pixel of one tile
    b, y, x = B - 1, H // 2, W // 2
    yield "dropped pixel", ref - _tap_outer(dyv[b, :, y, x], a, b, y, x)
    # one border column clamped to the wrong side: the left halo column of the first tile takes the image's last column
    if W > 1:
        m = ref.clone()
        for yy in range(min(TILE_H, H)):
            ys = (torch.arange(3) + yy - 1).clamp(0, H - 1)
            m[:, :, :, 0] += dyv[0, :, yy, 0].view(-1, 1, 1) * (a[0][:, ys, W - 1] - a[0][:, ys, 0]).unsqueeze(0)
        yield "wrong-side clamp", m
    elif H > 1:
        m = ref.clone()
        for xx in range(min(TILE_W, W)):
            xs = (torch.arange(3) + xx - 1).clamp(0, W - 1)
            m[:, :, 0, :] += dyv[0, :, 0, xx].view(-1, 1, 1) * (a[0][:, H - 1, xs] - a[0][:, 0, xs]).unsqueeze(0)
        yield "wrong-side clamp", m
    # the second source's affine taken from the first
    if c.C1 and c.aff != "--":
        idx = torch.arange(c.C1) % c.C0
        sc1 = None if d.scs[0] is None else d.scs[0][idx]
        sh1 = None if d.shs[0] is None else d.shs[0][idx]
        a_m = d.operands(form, [d.scs[0], sc1], [d.shs[0], sh1])[0]
        m = ref.clone()
        m[:, c.C0:] = R.conv3_rep_wgrad(a_m[:, c.C0:], dyv)
        yield "second source's affine from the first", m
    # the last 16-channel block dropped
    m = ref.clone()
    m[:, -16:] = 0.0
    yield "last block dropped", m
    # dL/dy of a partial tile's out-of-image pixel not zeroed: the linear address runs on into the next row
    if W % TILE_W:
        oy, ox = 0, W
    elif H % TILE_H:
        oy, ox = H, 0
    else:
        return
    p = oy * W + ox                                              # image 0
    if p < B * H * W:
        pb, py, px = p // (H * W), (p // W) % H, p % W
        yield "stray out-of-image pixel", ref + _tap_outer(dyv[pb, :, py, px], a, 0, oy, ox)
