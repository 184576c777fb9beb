"""The persistent tile walk of the 3x3 convolution kernels, at operator level.

conv3x3_mfma_kernel (tap-domain fp32 / bf16, Winograd NB == 1 with and without the weights in LDS) and conv3x3_wino8_kernel
(32 / 64 output channels) launch conv3x3_grid_blocks() workgroups, each of which walks a list of 16x16 tiles.  Only when
ntiles > grid does a workgroup see a SECOND tile: the producers then prefetch the next tile under the consumers' MFMAs, the
staging map switches between its interior and its border / partial-tile path, the BatchNorm statistic partials accumulate
over tiles, and (fused dL/dy) border pixels are written from several tiles.  The other operator tests stay at a handful of
tiles; here every case is a launch with two or three rounds, in each combination of the walk's three switches:

  XCD-contiguous or plain stride  x  rotated power-of-two or generic (% and /) tile index  x  even or uneven tile counts

A small Python mirror of conv3x3_grid_blocks() and of the kernels' walk says which regime a launch is in; every case asserts
the regime it was written for BEFORE launching, so a case that drifts out of it fails instead of passing trivially.

Checks per case:
  * walk independence, no tolerance: the same tensors run again in batch chunks small enough for one tile per workgroup (same
    tile geometry, so the same kernel variant and tile index form) must give bit-identical outputs -- a tile's arithmetic
    does not depend on which workgroup ran it or after which other tile.  Outputs start NaN-filled: an unwritten tile shows.
  * float64 CPU reference (F.conv2d on the replicate-padded input, autograd for the gradients): fp32 kernels to 1e-4 of the
    tensor's maximum (the project's bar); bf16 kernels to one rounding of the result, as tests/test_bf16_gpu.py holds them.
  * statistic partials: one finite row per workgroup; their float64 sum within 1e-4 * sum|y| and 1e-4 * sum y*y of the
    reference per channel, and within the same bound of the chunked runs' summed partials (the grouping differs).
A failure names the first wrong image, its tile (ty, tx), and the round and workgroup in which the mirror walks that tile."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-4   # BASELINE.json north_star: within 1e-4 relative fp32
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the launch geometry (csrc/conv_mfma.hip: conv3x3_grid_blocks, conv3x3_use_wino, conv3x3_wino_kind,
# launch_conv3x3_mfma) and of the kernels' tile walk
# ---------------------------------------------------------------------------------------------------------------------------
def tile_grid(H, W):
    return (H + 15) // 16, (W + 15) // 16


def grid_blocks(B, H, W, cout, wino=0):
    """-> (workgroups launched, gmax): conv3x3_grid_blocks(B, H, W, cout, wino)"""
    ty, tx = tile_grid(H, W)
    ntiles = B * ty * tx
    per_cu = (2 if wino == 2 else 1) if wino else (1 if cout >= 64 else 2)
    gmax = 256 * per_cu
    if ntiles <= gmax:
        return ntiles, gmax
    rounds = (ntiles + gmax - 1) // gmax
    g = (ntiles + rounds - 1) // rounds
    g = (g + 7) & ~7
    return min(g, ntiles), gmax


def use_wino(kout, nq, H, W):
    """conv3x3_use_wino for an fp32 call that passes a Winograd pack: kout = channels the kernel writes, nq = 16-channel blocks it reads"""
    return kout <= 64 and H % 2 == 0 and W % 2 == 0 and (kout > 16 or nq <= 2)


def wino_kind(kout, nq, H, W, zero_pad):
    if not use_wino(kout, nq, H, W):
        return 0
    return 2 if (kout == 16 and not zero_pad) else 1


def launch_grid(entry, cin, cout, B, H, W):
    """(workgroups, gmax) of the main kernel behind a public entry point for a layer cin -> cout.  The input-gradient entry
    points run the same kernels with the roles swapped: they read cout channels and write cin."""
    if entry in ("fwd", "fwd_bf16"):
        return grid_blocks(B, H, W, cout, 0)
    if entry == "fwd_wino":
        return grid_blocks(B, H, W, cout, wino_kind(cout, cin // 16, H, W, 0))
    if entry in ("dgrad", "dgrad_bf16", "fused_tap"):
        return grid_blocks(B, H, W, cin, 0)
    if entry in ("dgrad_wino", "fused_wino"):
        if cin == 128 and use_wino(64, cout // 16, H, W):      # two Winograd launches of 64 channels each
            return grid_blocks(B, H, W, 64, 1)
        return grid_blocks(B, H, W, cin, wino_kind(cin, cout // 16, H, W, 1))
    raise ValueError(entry)


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


class Walk:
    """Which workgroup runs which tile in which round, for a launch of `grid` workgroups over B images of H x W."""

    def __init__(self, B, H, W, grid):
        self.B, self.H, self.W, self.grid = B, H, W, grid
        ty, tx = tile_grid(H, W)
        self.ntiles = nt = B * ty * tx
        self.xcd = grid % 8 == 0 and nt % 8 == 0
        self.pow2 = _pow2(tx) and _pow2(ty)
        lgx, lgy = tx.bit_length() - 1, ty.bit_length() - 1
        self.where = {}                      # (image, tyi, txi) -> (round, workgroup)
        self.counts = []
        for wg in range(grid):
            if self.xcd:
                lo = (wg % 8) * (nt // 8); hi = lo + nt // 8; step = grid // 8; t = lo + wg // 8
            else:
                hi = nt; step = grid; t = wg
            r = 0
            while t < hi:
                if self.pow2:
                    tyi = (t >> lgx) & (ty - 1); tb = t >> (lgx + lgy); txi = (t + tyi + tb) & (tx - 1)
                else:
                    txi = t % tx; q = t // tx; tyi = q % ty; tb = q // ty
                assert (tb, tyi, txi) not in self.where
                self.where[(tb, tyi, txi)] = (r, wg)
                t += step; r += 1
            self.counts.append(r)
        assert len(self.where) == nt         # every tile is walked exactly once
        self.tmin, self.tmax = min(self.counts), max(self.counts)

    def regime(self):
        return (self.grid, self.xcd, self.pow2, self.tmin, self.tmax)

    def label(self):
        """(a) XCD map, even split; (b) XCD map, uneven; (c) plain stride, uneven; d: three rounds"""
        s = ("a" if self.tmin == self.tmax else "b") if self.xcd else ("c" if self.tmin < self.tmax else "-")
        return s + ("d" if self.tmax >= 3 else "")

    def describe(self):
        return (f"{self.ntiles} tiles on {self.grid} workgroups, {self.tmin}..{self.tmax} tiles per workgroup, "
                f"{'XCD' if self.xcd else 'plain'} walk, {'power-of-two' if self.pow2 else 'generic'} tile index [{self.label()}]")

    def locate(self, b, y, x):
        r, wg = self.where[(b, y // 16, x // 16)]
        return f"image {b}, tile (ty={y // 16}, tx={x // 16}) at pixel ({y}, {x}): round {r} of workgroup {wg}"


# name -> (gmax, H, W, B, expected Walk.regime() = (grid, xcd_map, power-of-two index, min, max tiles per workgroup)).
# 36x36 and 35x37: 3x3 tiles, generic index, one interior tile, partial right and bottom (35x37: odd, the Winograd entry points
# fall back to the taps).  52x52: 4x4 tiles, rotated power-of-two index, four interior tiles.  20x20: 2x2 tiles, the only
# power-of-two grid whose tile count is not a multiple of 8 (plain walk).  8x8: one partial all-border tile per image.
CELLS = {
    "256/36a": (256, 36, 36, 32, (144, True, False, 2, 2)),
    "256/36b": (256, 36, 36, 40, (184, True, False, 1, 2)),
    "256/36c": (256, 36, 36, 29, (136, False, False, 1, 2)),
    "256/36d": (256, 36, 36, 57, (176, False, False, 2, 3)),
    "256/52a": (256, 52, 52, 17, (136, True, True, 2, 2)),
    "256/52bd": (256, 52, 52, 34, (184, True, True, 2, 3)),
    "256/20b": (256, 20, 20, 66, (136, True, True, 1, 2)),
    "256/20c": (256, 20, 20, 65, (136, False, True, 1, 2)),
    "256/8d": (256, 8, 8, 520, (176, True, True, 2, 3)),
    "256/35a": (256, 35, 37, 32, (144, True, False, 2, 2)),
    "256/35b": (256, 35, 37, 40, (184, True, False, 1, 2)),
    "256/35c": (256, 35, 37, 29, (136, False, False, 1, 2)),
    "512/36a": (512, 36, 36, 64, (288, True, False, 2, 2)),
    "512/36b": (512, 36, 36, 72, (328, True, False, 1, 2)),
    "512/36c": (512, 36, 36, 57, (264, False, False, 1, 2)),
    "512/36d": (512, 36, 36, 114, (344, False, False, 2, 3)),
    "512/52a": (512, 52, 52, 33, (264, True, True, 2, 2)),
    "512/52bd": (512, 52, 52, 65, (352, True, True, 2, 3)),
    "512/20b": (512, 20, 20, 134, (272, True, True, 1, 2)),
    "512/20c": (512, 20, 20, 129, (264, False, True, 1, 2)),
    "512/8d": (512, 8, 8, 1040, (352, True, True, 2, 3)),
    "512/35a": (512, 35, 37, 64, (288, True, False, 2, 2)),
    "512/35b": (512, 35, 37, 72, (328, True, False, 1, 2)),
    "512/35c": (512, 35, 37, 57, (264, False, False, 1, 2)),
}


def enter_regime(entry, cin, cout, cell):
    """The walk of `entry` for a layer cin -> cout in `cell`, after asserting that the launch really is in the cell's regime,
    and the chunk size at which the same tensors get one tile per workgroup."""
    gmax_c, H, W, B, expect = CELLS[cell]
    grid, gmax = launch_grid(entry, cin, cout, B, H, W)
    assert gmax == gmax_c, f"{entry} {cin}->{cout} at {H}x{W} runs at most {gmax} workgroups, the cell was written for {gmax_c}"
    walk = Walk(B, H, W, grid)
    assert grid < walk.ntiles, f"{entry} {cin}->{cout} {cell}: {walk.describe()} -- no workgroup gets a second tile"
    assert walk.regime() == expect, f"{entry} {cin}->{cout} {cell}: {walk.describe()}, expected (grid, xcd, pow2, min, max) = {expect}"
    ty, tx = tile_grid(H, W)
    bc = gmax // (ty * tx)
    assert launch_grid(entry, cin, cout, bc, H, W)[0] == bc * ty * tx       # one tile per workgroup in every chunk
    print(f"\n[tile walk] {entry} {cin}->{cout} B={B} {H}x{W}: {walk.describe()}; chunks of {bc} images")
    return walk, H, W, B, bc


def chunks(B, bc):
    return [(b0, min(B, b0 + bc)) for b0 in range(0, B, bc)]


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import sifsr  # noqa: F401
    from sifsr import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return _lib


def S():
    return torch.cuda.current_stream().cuda_stream


def rng(case):
    return np.random.RandomState(zlib.crc32(repr(case).encode()) % 2**31)


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


def uni(rs, n):
    return torch.from_numpy(rs.uniform(0.5, 1.5, n).astype(np.float32))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rb(t):
    return t.to(BF).float()


def conv_rep(x, w):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _first(mask_bhw):
    B, H, W = mask_bhw.shape
    i = int(torch.nonzero(mask_bhw.flatten())[0])
    return i // (H * W), (i // W) % H, i % W


def assert_walk_independent(what, multi, parts, walk, only=None):
    """NHWC output of the multi-round launch == concatenation of the one-tile-per-workgroup chunk runs, bit for bit.
    `only`: H x W mask of the pixels the kernel writes (the rest must still hold the NaN fill)."""
    multi, single = multi.cpu(), torch.cat([p.cpu() for p in parts], 0)
    if only is not None:
        assert torch.isnan(multi[:, ~only]).all() and torch.isnan(single[:, ~only]).all(), f"{what}: pixels outside the mask were written"
        same = torch.equal(multi[:, only], single[:, only])
    else:
        same = torch.equal(multi, single)
    if same:
        return
    bad = ~(multi == single)                     # (NaN: an unwritten pixel counts as wrong)
    if only is not None:
        bad &= only[None, :, :, None]
    b, y, x = _first(bad.any(-1))
    n_bad = int(bad.any(-1).sum())
    raise AssertionError(f"{what}: the multi-round launch differs from one tile per workgroup at {n_bad} pixels; first: "
                         f"{walk.locate(b, y, x)} -- got {multi[b, y, x].flatten()[:4].tolist()}, "
                         f"single-tile {single[b, y, x].flatten()[:4].tolist()} ({walk.describe()})")


def _err_map(got, ref, only):
    err = (got.cpu().double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if only is not None:
        m = only[None, :, :, None]
        err, ref = torch.where(m, err, torch.zeros_like(err)), torch.where(m, ref, torch.zeros_like(ref))
    return err, ref


def assert_close_ref(what, got, ref, walk, only=None):
    """fp32 NHWC output against the float64 NHWC reference: max|a-b| / max|b| < 1e-4"""
    err, ref = _err_map(got, ref, only)
    e = float(err.max() / ref.abs().max())
    print(f"[tile walk]   {what}: rel err {e:.2e}")
    if not e < TOL:
        b, y, x = _first((err == err.max()).any(-1))
        raise AssertionError(f"{what}: rel err {e:.3e} >= {TOL}; worst: {walk.locate(b, y, x)} ({walk.describe()})")


def assert_bf16_close_ref(what, got, ref, walk, edge=None):
    """bf16-stored NHWC output against the float64 reference on the same bf16 operands: one rounding of the result, the
    bound of tests/test_bf16_gpu.py::assert_bf16_close (4e-3 of the maximum and a mean error of 2.5e-3 of the mean magnitude).
    edge: H x W mask of the image-border pixels, to report their error apart from the interior's."""
    err, ref = _err_map(got.float(), ref, None)
    scale, emax, emean, rmean = float(ref.abs().max()), float(err.max()), float(err.mean()), float(ref.abs().mean())
    print(f"[tile walk]   {what}: max err {emax / scale:.2e} of the maximum, mean err {emean / rmean:.2e} of the mean magnitude")
    if edge is not None:
        print(f"[tile walk]   {what}: max err on the image border {float(err[:, edge].max()) / scale:.2e}, "
              f"inside {float(err[:, ~edge].max()) / scale if (~edge).any() else 0.0:.2e} of the maximum")
    if not (emax <= 4e-3 * scale and emean <= 2.5e-3 * rmean):
        b, y, x = _first((err == err.max()).any(-1))
        raise AssertionError(f"{what}: max err {emax:.3e} (bound {4e-3 * scale:.3e}), mean err {emean:.3e} (bound {2.5e-3 * rmean:.3e}); "
                             f"worst: {walk.locate(b, y, x)} ({walk.describe()})")


def assert_stat_partials(what, part, parts_single, y_ref, walk):
    """part: [grid][cout][2] of the multi-round launch; y_ref: float64 NHWC values the statistics describe"""
    assert part.shape[0] == walk.grid
    p = part.cpu().double()
    rows = torch.nonzero(~torch.isfinite(p).all(-1).all(-1)).flatten().tolist()
    assert not rows, f"{what}: statistic rows of workgroups {rows[:8]} are not finite ({walk.describe()})"
    ps = p.sum(0)
    single = sum(q.cpu().double().sum(0) for q in parts_single)
    s1, sa, s2 = y_ref.sum((0, 1, 2)), y_ref.abs().sum((0, 1, 2)), (y_ref * y_ref).sum((0, 1, 2))
    for k, (want, bound, name) in enumerate(((s1, TOL * sa, "sum y"), (s2, TOL * s2, "sum y*y"))):
        for got, other, versus in ((ps, want, "the reference"), (single, want, "the reference (one-tile-per-workgroup runs)"),
                                   (ps, single[:, k], "the one-tile-per-workgroup runs")):
            ok = (got[:, k] - other).abs() <= bound
            assert ok.all(), (f"{what}: {name} against {versus} off in channels {torch.nonzero(~ok).flatten().tolist()[:8]}: "
                              f"{got[~ok, k][:4].tolist()} vs {other[~ok][:4].tolist()} ({walk.describe()})")


def pack(L, w, cin, cout):
    dw = w.cuda()
    wf = torch.empty(9 * cin * cout, device="cuda"); wd = torch.empty(4 * 9 * cin * cout, device="cuda")
    L.call("sifsr_pack_conv_weights", dw, cin, cout, wf, wd, S())
    wwf = torch.empty(16 * cin * cout, device="cuda"); wwd = torch.empty(16 * cin * cout, device="cuda")
    L.call("sifsr_pack_conv_weights_wino", dw, cin, cout, wwf, wwd, S())
    return dw, wf, wd, wwf, wwd


def weights(rs, cin, cout):
    return rnd(rs, cout, cin, 3, 3, scale=(2.0 / (9 * cin)) ** 0.5)


def dgrad_ref(w64, dy64, H, W):
    """float64 autograd of the replicate-padded convolution w.r.t. its input (includes the border fold)"""
    a = torch.zeros(dy64.shape[0], w64.shape[1], H, W, dtype=torch.float64, requires_grad=True)
    (ga,) = torch.autograd.grad(conv_rep(a, w64), a, dy64)
    return ga


# ---------------------------------------------------------------------------------------------------------------------------
# 1 + 2: forward, tap-domain and Winograd-domain, with statistic partials.  (entry, C0, C1, cout, cell)
# ---------------------------------------------------------------------------------------------------------------------------
FWD_CASES = [
    # tap-domain fp32 kernel: NB = 1, 2 (512 workgroups), 4, 8 (256)
    ("fwd", 16, 0, 16, "512/36a"), ("fwd", 16, 0, 16, "512/20c"), ("fwd", 16, 0, 16, "512/8d"), ("fwd", 16, 0, 16, "512/35b"),
    ("fwd", 32, 0, 32, "512/36b"), ("fwd", 32, 0, 32, "512/52a"), ("fwd", 32, 0, 32, "512/36d"),
    ("fwd", 32, 32, 32, "512/36c"), ("fwd", 32, 32, 32, "512/52bd"), ("fwd", 32, 32, 32, "512/20b"),
    ("fwd", 64, 0, 64, "256/36a"), ("fwd", 64, 0, 64, "256/20c"), ("fwd", 64, 0, 64, "256/8d"), ("fwd", 64, 0, 64, "256/35c"),
    ("fwd", 64, 0, 128, "256/36c"), ("fwd", 64, 0, 128, "256/52a"), ("fwd", 64, 0, 128, "256/36b"), ("fwd", 64, 0, 128, "256/20b"),
    # Winograd forward, 16 output channels: weights in LDS, two workgroups per CU (512)
    ("fwd_wino", 16, 0, 16, "512/36a"), ("fwd_wino", 16, 0, 16, "512/20c"), ("fwd_wino", 16, 0, 16, "512/8d"),
    ("fwd_wino", 16, 0, 16, "512/35c"),                      # odd size: the taps
    ("fwd_wino", 32, 0, 16, "512/36b"), ("fwd_wino", 32, 0, 16, "512/52bd"), ("fwd_wino", 32, 0, 16, "512/36d"),
    ("fwd_wino", 32, 0, 16, "512/20b"), ("fwd_wino", 32, 0, 16, "512/36c"), ("fwd_wino", 32, 0, 16, "512/52a"),
    # the wino8 kernel (256)
    ("fwd_wino", 16, 0, 32, "256/36a"), ("fwd_wino", 16, 0, 32, "256/20c"), ("fwd_wino", 16, 0, 32, "256/8d"),
    ("fwd_wino", 64, 0, 32, "256/36b"), ("fwd_wino", 64, 0, 32, "256/52a"), ("fwd_wino", 64, 0, 32, "256/36d"),
    ("fwd_wino", 64, 0, 64, "256/36c"), ("fwd_wino", 64, 0, 64, "256/52bd"), ("fwd_wino", 64, 0, 64, "256/20b"),
    ("fwd_wino", 64, 0, 64, "256/35a"),                      # odd size: the taps, NB = 4
    ("fwd_wino", 64, 64, 64, "256/36c"), ("fwd_wino", 64, 64, 64, "256/52a"),
]


def _id(case):
    return "-".join(str(v) for v in case)


@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_forward_tile_walk(L, case):
    entry, C0, C1, cout, cell = case
    cin = C0 + C1
    walk, H, W, B, bc = enter_regime(entry, cin, cout, cell)
    rs = rng(case)
    # folded BatchNorm + ReLU on every source, as the producing layers leave them (tests/test_ops_gpu.py::_mk_inputs)
    xs, scs, shs = [], [], []
    for C in (C0, C1):
        if C:
            xs.append(rnd(rs, B, C, H, W)); scs.append(uni(rs, C)); shs.append(rnd(rs, C, scale=0.3))
    a64 = torch.cat([F.relu(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)) for x, sc, sh in zip(xs, scs, shs)], 1)
    w = weights(rs, cin, cout)
    y_ref = nhwc(conv_rep(a64, w.double()))
    _, wf, _, wwf, _ = pack(L, w, cin, cout)
    d = [nhwc(x).cuda() for x in xs] + [None]
    dsc = [t.cuda() for t in scs] + [None]
    dsh = [t.cuda() for t in shs] + [None]

    def run(b0, b1):
        n = b1 - b0
        nblk = (L.call("sifsr_conv3x3_stat_blocks", n, H, W, cout) if entry == "fwd"
                else L.call("sifsr_conv3x3_stat_blocks_wino", n, H, W, cin, cout))
        assert nblk == launch_grid(entry, cin, cout, n, H, W)[0], "the mirror disagrees with the library about the grid"
        y, part = nan(n, H, W, cout), nan(nblk, cout, 2)
        src1 = d[1][b0:b1] if C1 else None
        if entry == "fwd":
            L.call("sifsr_conv3x3_fwd", d[0][b0:b1], C0, dsc[0], dsh[0], src1, C1, dsc[1], dsh[1], wf, y, cout, part, n, H, W, S())
        else:
            L.call("sifsr_conv3x3_fwd_wino", d[0][b0:b1], C0, dsc[0], dsh[0], src1, C1, dsc[1], dsh[1], wf, wwf, y, cout, part, n, H, W, S())
        return y, part

    y, part = run(0, B)
    single = [run(b0, b1) for b0, b1 in chunks(B, bc)]
    torch.cuda.synchronize()
    assert_walk_independent("y", y, [s[0] for s in single], walk)
    assert_close_ref("y", y, y_ref, walk)
    assert_stat_partials("statistic partials", part, [s[1] for s in single], y_ref, walk)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: input gradient, tap-domain and Winograd-domain.  (entry, C0, C1, cout, addend, cell): the layer is C0 + C1 -> cout, the
# gradient goes to split destinations when C1 > 0
# ---------------------------------------------------------------------------------------------------------------------------
DGRAD_CASES = [
    # tap-domain: the kernel writes cin channels -> 512 workgroups for cin < 64, 256 from 64 on
    ("dgrad", 16, 0, 16, False, "512/36a"), ("dgrad", 16, 0, 16, False, "512/20c"), ("dgrad", 16, 0, 16, True, "512/8d"),
    ("dgrad", 16, 0, 16, False, "512/35a"),
    ("dgrad", 32, 0, 32, False, "512/36b"), ("dgrad", 32, 0, 32, False, "512/52a"),
    ("dgrad", 32, 0, 16, False, "512/36d"), ("dgrad", 16, 0, 32, False, "512/52bd"),
    ("dgrad", 16, 0, 32, False, "512/36c"), ("dgrad", 32, 0, 16, False, "512/20b"),
    ("dgrad", 32, 32, 32, False, "256/36c"), ("dgrad", 32, 32, 32, False, "256/20b"),
    ("dgrad", 64, 0, 64, False, "256/36a"), ("dgrad", 64, 0, 64, False, "256/20c"), ("dgrad", 64, 0, 64, False, "256/35b"),
    ("dgrad", 64, 0, 128, False, "256/36b"), ("dgrad", 64, 0, 128, False, "256/8d"),
    ("dgrad", 64, 0, 32, True, "256/36c"), ("dgrad", 64, 0, 32, False, "256/52a"), ("dgrad", 64, 0, 32, False, "256/36d"),
    ("dgrad", 64, 0, 32, False, "256/52bd"),
    ("dgrad", 128, 0, 64, False, "256/20b"), ("dgrad", 128, 0, 64, False, "256/36a"),
    ("dgrad", 64, 64, 64, False, "256/36c"), ("dgrad", 64, 64, 64, False, "256/20c"),
    # Winograd-domain (one workgroup per CU: 256).  cin = 16: conv3x3_mfma_kernel NB == 1; 32 / 64: the wino8 kernel
    ("dgrad_wino", 16, 0, 16, False, "256/36a"), ("dgrad_wino", 16, 0, 16, False, "256/20c"), ("dgrad_wino", 16, 0, 16, True, "256/52bd"),
    ("dgrad_wino", 16, 0, 32, False, "256/36b"), ("dgrad_wino", 16, 0, 32, False, "256/8d"),
    ("dgrad_wino", 32, 0, 32, False, "256/36c"), ("dgrad_wino", 32, 0, 32, False, "256/52a"),
    ("dgrad_wino", 32, 0, 32, False, "512/35c"),             # odd size: the taps, NB = 2
    ("dgrad_wino", 32, 0, 16, False, "256/36d"), ("dgrad_wino", 32, 0, 16, False, "256/20b"),
    ("dgrad_wino", 64, 0, 64, True, "256/36a"), ("dgrad_wino", 64, 0, 64, False, "256/52bd"),
    ("dgrad_wino", 64, 0, 32, False, "256/36b"), ("dgrad_wino", 64, 0, 32, False, "256/8d"),
    ("dgrad_wino", 64, 0, 128, False, "256/36c"), ("dgrad_wino", 64, 0, 128, False, "256/20c"),
    # 128 channels to write: two Winograd launches of 64 each (ub1.convbloc.bloc.0, cin = 128, cout = 64)
    ("dgrad_wino", 128, 0, 64, False, "256/36a"), ("dgrad_wino", 128, 0, 64, False, "256/20b"), ("dgrad_wino", 128, 0, 64, False, "256/52a"),
    ("dgrad_wino", 128, 0, 64, False, "256/35a"),            # odd size: the taps, NB = 8
    ("dgrad_wino", 32, 32, 32, False, "256/36b"), ("dgrad_wino", 32, 32, 32, False, "256/52a"),
    ("dgrad_wino", 64, 64, 64, False, "256/36c"), ("dgrad_wino", 64, 64, 64, False, "256/8d"),
]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=_id)
def test_input_gradient_tile_walk(L, case):
    entry, C0, C1, cout, with_add, cell = case
    cin = C0 + C1
    walk, H, W, B, bc = enter_regime(entry, cin, cout, cell)
    rs = rng(case)
    w = weights(rs, cin, cout)
    dy = rnd(rs, B, cout, H, W)
    add = rnd(rs, B, cin, H, W) if with_add else None
    g_ref = nhwc(dgrad_ref(w.double(), dy.double(), H, W) + (add.double() if with_add else 0.0))
    dw, _, wd, _, wwd = pack(L, w, cin, cout)
    ddy = nhwc(dy).cuda()
    dadd = nhwc(add).cuda() if with_add else None

    def run(b0, b1):
        n = b1 - b0
        g0 = nan(n, H, W, C0)
        g1 = nan(n, H, W, C1) if C1 else None
        L.call("sifsr_conv3x3_" + entry, ddy[b0:b1], cout, wd, dw if entry == "dgrad" else wwd, cin, g0, C0, g1, C1,
               dadd[b0:b1] if with_add else None, n, H, W, S())
        return g0, g1

    g0, g1 = run(0, B)
    single = [run(b0, b1) for b0, b1 in chunks(B, bc)]
    torch.cuda.synchronize()
    assert_walk_independent("g0", g0, [s[0] for s in single], walk)
    assert_close_ref("g0", g0, g_ref[..., :C0], walk)
    if C1:
        assert_walk_independent("g1", g1, [s[1] for s in single], walk)
        assert_close_ref("g1", g1, g_ref[..., C0:], walk)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: input gradient with the layer's BatchNorm + ReLU backward formed while staging (dL/dy never stored, except on the image
# border).  (entry, C, cell): C -> C layer, tap-domain (no Winograd pack passed) or Winograd-domain
# ---------------------------------------------------------------------------------------------------------------------------
FUSED_CASES = [
    ("fused_tap", 16, "512/36a"), ("fused_tap", 16, "512/20c"), ("fused_tap", 16, "512/8d"), ("fused_tap", 16, "512/35b"),
    ("fused_tap", 32, "512/36b"), ("fused_tap", 32, "512/52a"), ("fused_tap", 32, "512/36d"), ("fused_tap", 32, "512/36c"),
    ("fused_tap", 32, "512/52bd"), ("fused_tap", 32, "512/20b"),
    ("fused_tap", 64, "256/36a"), ("fused_tap", 64, "256/36b"), ("fused_tap", 64, "256/36c"), ("fused_tap", 64, "256/52a"),
    ("fused_tap", 64, "256/20b"), ("fused_tap", 64, "256/20c"), ("fused_tap", 64, "256/8d"),
    ("fused_wino", 16, "256/36a"), ("fused_wino", 16, "256/20c"), ("fused_wino", 16, "256/8d"), ("fused_wino", 16, "256/36d"),
    ("fused_wino", 32, "256/36b"), ("fused_wino", 32, "256/52a"), ("fused_wino", 32, "256/20b"), ("fused_wino", 32, "256/36c"),
    ("fused_wino", 64, "256/36c"), ("fused_wino", 64, "256/52bd"), ("fused_wino", 64, "256/36a"), ("fused_wino", 64, "256/8d"),
    ("fused_wino", 64, "256/35c"),                           # odd size: the taps, NB = 4
]


@pytest.mark.parametrize("case", FUSED_CASES, ids=_id)
def test_fused_dy_input_gradient_tile_walk(L, case):
    """z = relu(bn_train(conv(a))) with upstream gradient g on z, as test_bn_relu_backward_fused_into_dgrad_and_wgrad builds
    it: the coefficients come from sifsr_bn_relu_bwd_coef over the whole batch, so the chunked runs use the same ones."""
    entry, C, cell = case
    walk, H, W, B, bc = enter_regime(entry, C, C, cell)
    rs = rng(case)
    a = rnd(rs, B, C, H, W)
    w = weights(rs, C, C)
    gamma, beta = uni(rs, C), rnd(rs, C, scale=0.5)
    g = rnd(rs, B, C, H, W)
    # float64 reference on the float32 conv output the device is given
    y = conv_rep(a.double(), w.double()).float()
    y64 = y.double().requires_grad_(True)
    z64 = F.relu(F.batch_norm(y64, None, None, gamma.double(), beta.double(), training=True, eps=1e-5))
    (dy64,) = torch.autograd.grad(z64, y64, g.double())
    g_ref = nhwc(dgrad_ref(w.double(), dy64, H, W))
    dy_ref = nhwc(dy64)
    mean = y.double().mean((0, 2, 3)); var = y.double().var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale, shift = gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd

    _, _, wd, _, wwd = pack(L, w, C, C)
    dg, dyv = nhwc(g).cuda(), nhwc(y).cuda()
    npix = B * H * W
    nb = max(1, min(1024, npix // 256))
    partials = torch.empty(1024 * C * 2, device="cuda")
    dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    coef = torch.empty(3 * C, dtype=torch.float64, device="cuda")
    coef_f = torch.empty(4 * C, device="cuda")
    L.call("sifsr_bn_relu_bwd_coef", dg, dyv, scale.float().cuda(), shift.float().cuda(), mean.float().cuda(), invstd.float().cuda(),
           beta.cuda(), C, npix, partials, nb, dgam, dbet, coef, coef_f, None, H, W, S())

    def run(b0, b1):
        n = b1 - b0
        gin, border = nan(n, H, W, C), nan(n, H, W, C)
        L.call("sifsr_conv3x3_dgrad_fused", dg[b0:b1], dyv[b0:b1], coef_f, C, wd, wwd if entry == "fused_wino" else None, C,
               gin, C, None, 0, None, border, n, H, W, S())
        return gin, border

    gin, border = run(0, B)
    single = [run(b0, b1) for b0, b1 in chunks(B, bc)]
    torch.cuda.synchronize()
    edge = torch.zeros(H, W, dtype=torch.bool); edge[0] = edge[-1] = True; edge[:, 0] = edge[:, -1] = True
    assert_walk_independent("g0", gin, [s[0] for s in single], walk)
    assert_walk_independent("border", border, [s[1] for s in single], walk, only=edge)
    assert_close_ref("g0", gin, g_ref, walk)
    assert_close_ref("border", border, dy_ref, walk, only=edge)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: bf16 operands and bf16 activation storage: forward (with statistic partials) and input gradient of a C -> C layer
# ---------------------------------------------------------------------------------------------------------------------------
BF16_CASES = [
    (16, "512/36a"), (16, "512/36b"), (16, "512/36c"), (16, "512/36d"), (16, "512/52a"), (16, "512/52bd"), (16, "512/20b"),
    (16, "512/20c"), (16, "512/8d"), (16, "512/35a"),
    (64, "256/36a"), (64, "256/36b"), (64, "256/36c"), (64, "256/52a"), (64, "256/20b"), (64, "256/20c"), (64, "256/8d"),
    (64, "256/35b"),
    (16, "512/36c", "addend"), (64, "256/20b", "addend"),    # the input gradient with the residual addend
]


@pytest.mark.parametrize("case", BF16_CASES, ids=_id)
def test_bf16_tile_walk(L, case):
    """Three of these cases are regression tests: 16-512/36b, 16-512/8d and 64-256/20c missed the one-rounding bound of
    tests/test_bf16_gpu.py on the input gradient (4.10e-3, 4.19e-3 and 4.01e-3 of the tensor's maximum against 4e-3), each time
    at an image-border pixel -- over the first 18 cases the largest error was 1.8e-3 to 2.3e-3 inside the image and 3.4e-3 to
    4.2e-3 on its border (the test prints both).  Not the walk (the chunked runs gave the same bits): sifsr_conv3x3_dgrad_bf16
    rounded image-border pixels TWICE -- the main kernel stored rn(zero-padded sum + addend) as bf16, then dgrad_border_kernel
    read that back, added the replicate-border fold and rounded again.  The entry point now forms its border pixels whole and
    rounds them once (dgrad_border_whole_bf16_kernel)."""
    C, cell = case[:2]
    with_add = len(case) > 2
    walk, H, W, B, bc = enter_regime("fwd_bf16", C, C, cell)
    assert enter_regime("dgrad_bf16", C, C, cell)[0].regime() == walk.regime()
    rs = rng(case)
    x = rb(rnd(rs, B, C, H, W))                              # what the bf16 tensors hold
    sc, sh = uni(rs, C), rnd(rs, C, scale=0.3)
    w = weights(rs, C, C)
    dy = rb(rnd(rs, B, C, H, W))
    a_in = rb(F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)))     # operand after the fp32 transform, rounded
    y_ref = nhwc(conv_rep(a_in.double(), rb(w).double()))
    add = rb(rnd(rs, B, C, H, W)) if with_add else None
    g_ref = nhwc(dgrad_ref(rb(w).double(), dy.double(), H, W) + (add.double() if with_add else 0.0))
    _, _, wd, _, _ = pack(L, w, C, C)
    dx, ddy = nhwc(x).to(BF).cuda(), nhwc(dy).to(BF).cuda()
    dadd = nhwc(add).to(BF).cuda() if with_add else None
    dsc, dsh = sc.cuda(), sh.cuda()

    def run(b0, b1):
        n = b1 - b0
        nblk = L.call("sifsr_conv3x3_stat_blocks", n, H, W, C)
        assert nblk == launch_grid("fwd_bf16", C, C, n, H, W)[0], "the mirror disagrees with the library about the grid"
        y, gx, part = nan(n, H, W, C, dtype=BF), nan(n, H, W, C, dtype=BF), nan(nblk, C, 2)
        L.call("sifsr_conv3x3_fwd_bf16", dx[b0:b1], C, dsc, dsh, None, 0, None, None, wd, y, C, part, n, H, W, S())
        L.call("sifsr_conv3x3_dgrad_bf16", ddy[b0:b1], C, wd, C, gx, C, None, 0, dadd[b0:b1] if with_add else None, n, H, W, S())
        return y, gx, part

    y, gx, part = run(0, B)
    single = [run(b0, b1) for b0, b1 in chunks(B, bc)]
    torch.cuda.synchronize()
    assert_walk_independent("y (bf16)", y, [s[0] for s in single], walk)
    assert_walk_independent("input gradient (bf16)", gx, [s[1] for s in single], walk)
    assert_bf16_close_ref("y (bf16)", y, y_ref, walk)
    edge = torch.zeros(H, W, dtype=torch.bool); edge[0] = edge[-1] = True; edge[:, 0] = edge[:, -1] = True
    assert_bf16_close_ref("input gradient (bf16)", gx, g_ref, walk, edge=edge)
    # the statistics describe the STORED (rounded) values
    assert_stat_partials("statistic partials (bf16)", part, [s[2] for s in single], y.cpu().double(), walk)


# ---------------------------------------------------------------------------------------------------------------------------
# the regimes the cases above cover
# ---------------------------------------------------------------------------------------------------------------------------
def coverage():
    """{family: {(index form, regime letter): number of cases}} from the mirror alone"""
    fam = {}
    rows = ([("fwd tap", c[0], c[1] + c[2], c[3], c[4]) for c in FWD_CASES if c[0] == "fwd"]
            + [("fwd wino", c[0], c[1] + c[2], c[3], c[4]) for c in FWD_CASES if c[0] == "fwd_wino"]
            + [("dgrad / dgrad_wino", c[0], c[1] + c[2], c[3], c[5]) for c in DGRAD_CASES]
            + [("dgrad_fused", c[0], c[1], c[1], c[2]) for c in FUSED_CASES]
            + [("bf16 fwd + dgrad", e, c[0], c[0], c[1]) for c in BF16_CASES for e in ("fwd_bf16", "dgrad_bf16")])
    for name, entry, cin, cout, cell in rows:
        _, H, W, B, _ = CELLS[cell]
        walk = Walk(B, H, W, launch_grid(entry, cin, cout, B, H, W)[0])
        for letter in walk.label():
            key = ("pow2" if walk.pow2 else "generic", letter)
            fam.setdefault(name, {}).setdefault(key, 0)
            fam[name][key] += 1
    return fam


def test_every_family_covers_every_regime(L):
    """Each kernel family has at least one case in each of (a) XCD even, (b) XCD uneven, (c) plain uneven, (d) three rounds,
    for the generic and for the power-of-two tile index; and the mirror agrees with the library's public grid queries."""
    for cell, (gmax, H, W, B, expect) in CELLS.items():
        for n in (1, gmax // (tile_grid(H, W)[0] * tile_grid(H, W)[1]), B):
            for cout in (16, 32, 64, 128):
                assert L.call("sifsr_conv3x3_stat_blocks", n, H, W, cout) == grid_blocks(n, H, W, cout, 0)[0], (cell, n, cout)
                for cin in (16, 32, 64, 128):
                    assert (L.call("sifsr_conv3x3_stat_blocks_wino", n, H, W, cin, cout)
                            == launch_grid("fwd_wino", cin, cout, n, H, W)[0]), (cell, n, cin, cout)
    fam = coverage()
    cols = [(i, r) for i in ("generic", "pow2") for r in "abcd"]
    print("\n[tile walk] cases per regime          " + "  ".join(f"{i[:3]}-{r}" for i, r in cols))
    for name, cnt in fam.items():
        print(f"[tile walk] {name:28s}" + "  ".join(f"{cnt.get(c, 0):5d}" for c in cols))
    for name, cnt in fam.items():
        for c in cols:
            assert cnt.get(c, 0) >= 1, f"{name}: no case with the {c[0]} tile index in regime ({c[1]})"
