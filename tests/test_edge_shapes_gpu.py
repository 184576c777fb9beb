"""GPU parity of the kernels beside the hot path at the shapes where they can go wrong: the input pipeline and the
train-time metrics (csrc/pipeline.hip), the Fourier evaluation (csrc/fourier.hip), the loss operators (csrc/loss.hip)
and the optimizer (csrc/adam.hip).  tests/test_ops_gpu.py, test_pipeline_gpu.py and test_fourier.py hold each of them at
one or two friendly sizes; here: sizes below one tile, tiles with an empty interior, ragged last blocks, every grid-stride
loop past its cap, every window the launchers accept, inputs with a closed-form answer.

Every reference is the oracle (oracle/sif_oracle.py), NumPy or PyTorch on the CPU, in float64 wherever the oracle takes
it.  The bars are the ones the friendly-size tests already hold; where a shape needs a looser one it is
max(bar, 4 x the float32-vs-float64 gap of the ORACLE at that shape), the gap measured on the CPU and written next to the
constant -- never a figure the kernels produced.  Every buffer the wrappers allocate (outputs and scratch) is handed out
NaN-filled, so an element a kernel does not write fails its comparison."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sif_oracle as O
from tests.conftest import rel_err
from tests.test_ops_gpu import L, S, TOL, dev, rnd  # noqa: F401  (L is the library fixture)

pytestmark = pytest.mark.gpu

STATS = {"mean_lst": 307.2378, "std_lst": 5.5698, "mean_ndvi": 0.6452, "std_ndvi": 0.1683}
NAN = float("nan")


@pytest.fixture(scope="module")
def sifsr(L):
    import sifsr as pkg
    return pkg


@pytest.fixture(autouse=True)
def nan_prefill(monkeypatch):
    """The Python wrappers allocate outputs and scratch with torch.empty / torch.empty_like: fill those with NaN (all-ones
    bytes for the uint8 scratch: NaN as float32 and as float64) before the kernels see them."""
    real_empty, real_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_cuda:
            t.fill_(NAN) if t.is_floating_point() else t.fill_(255 if t.dtype == torch.uint8 else -1)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: poison(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: poison(real_like(*a, **k)))


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------
# 1. PSNR / SSIM
# ---------------------------------------------------------------------------------------------------------------------
def metric_pair(seed, shape, noise=0.3):
    """A smooth-ish target and a noisy prediction of it, as in test_pipeline_gpu.test_psnr_ssim (not Kelvin-scaled);
    ``noise`` is a scalar or one level per image."""
    rs = np.random.RandomState(seed)
    t = rs.standard_normal(shape).astype(np.float32)
    t = (t + np.roll(t, 1, 2) + np.roll(t, 1, 3) + np.roll(t, (1, 1), (2, 3))) / 2
    lvl = np.asarray(noise, dtype=np.float32).reshape(-1, 1, 1, 1)
    return t + lvl * rs.standard_normal(shape).astype(np.float32), t


def check_metrics(sifsr, p, t):
    psnr_ref, ssim_ref = O.psnr_skimage(p, t), O.ssim_skimage(p, t)
    psnr, ssim = sifsr.metrics.psnr_ssim(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda())
    psnr, ssim = float(psnr), float(ssim)
    print(f"psnr {psnr!r} ref {psnr_ref!r} rel {abs(psnr - psnr_ref) / abs(psnr_ref):.2e}; "
          f"ssim {ssim!r} ref {ssim_ref!r} rel {abs(ssim - ssim_ref) / abs(ssim_ref):.2e}")
    assert abs(psnr - psnr_ref) < 1e-4 * abs(psnr_ref)
    assert abs(ssim - ssim_ref) < 1e-4 * abs(ssim_ref)
    return psnr_ref, ssim_ref


# (B,H,W): 7x7 is ONE window-valid pixel; 33x38 and 39x71 end in a tile column whose interior is empty / one pixel wide;
# 32x32 is exactly one tile, 38x38 a second tile that holds only the last three interior rows / columns
@pytest.mark.parametrize("shape", [(2, 7, 7), (1, 8, 9), (3, 7, 40), (2, 33, 38), (2, 39, 71), (1, 32, 32), (1, 38, 38)])
def test_psnr_ssim_small_and_ragged(sifsr, shape):
    B, H, W = shape
    p, t = metric_pair(100 * H + W, (B, 1, H, W))
    check_metrics(sifsr, p, t)


def test_psnr_ssim_more_images_than_threads(sifsr):
    """B = 257: thread 0 of the final kernel owns images 0 and 256.  Image 256 is ten times noisier than the rest, so a
    mean without it is far off."""
    B = 257
    noise = np.full(B, 0.1, dtype=np.float32)
    noise[256] = 3.0
    p, t = metric_pair(257, (B, 1, 7, 9), noise)
    psnr_ref, ssim_ref = check_metrics(sifsr, p, t)
    # the case does its job: the same means without image 256 miss the bar by far
    rng = float(t.max() - t.min())
    each = [10 * np.log10(rng ** 2 / np.mean((t[i, 0] - p[i, 0]) ** 2, dtype=np.float64)) for i in range(B)]
    assert abs(np.mean(each[:256]) - psnr_ref) > 10 * 1e-4 * abs(psnr_ref)


def test_psnr_ssim_minmax_sweep_past_one_pass(sifsr):
    """17 x 512 x 512 > 256 * 64 * 256 elements: the min / max partial kernel runs its capped grid.  The target's global
    minimum and maximum sit in the LAST image: a sweep that stops early returns a smaller data range."""
    p, t = metric_pair(17, (17, 1, 512, 512))
    assert t.size > 256 * 64 * 256
    lo, hi = float(t.min()), float(t.max())
    t[16, 0, 500, 37] = lo - 3.0
    t[16, 0, 11, 490] = hi + 3.0
    p[16, 0, 500, 37], p[16, 0, 11, 490] = lo - 3.2, hi + 2.9
    assert t[:16].min() > t.min() + 2 and t[:16].max() < t.max() - 2
    check_metrics(sifsr, p, t)


def test_psnr_ssim_identical_images(sifsr):
    _, t = metric_pair(16, (1, 1, 16, 16))
    with np.errstate(divide="ignore"):
        assert O.psnr_skimage(t, t) == math.inf and abs(O.ssim_skimage(t, t) - 1.0) < 1e-6
    x = torch.from_numpy(t).cuda()
    psnr, ssim = sifsr.metrics.psnr_ssim(x, x.clone())
    assert float(psnr) == math.inf
    assert abs(float(ssim) - 1.0) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 2. Tiles
# ---------------------------------------------------------------------------------------------------------------------
def tile_inputs(seed, T, win):
    """LST tiles in Kelvin and NDVI tiles of which more than a quarter lies outside [-1, 1], exact +-1 and their float32
    neighbours included."""
    rs = np.random.RandomState(seed)
    lst = rnd(rs, T, 1, win, win, scale=5.5) + 307.0
    ndvi = rnd(rs, T, 1, 4 * win, 4 * win, scale=1.2) + 0.1
    edge = torch.tensor([1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)),
                         np.nextafter(np.float32(-1), np.float32(-2)), np.nextafter(np.float32(-1), np.float32(0))])
    flat = ndvi.view(T, -1)
    flat[:, 3:3 + 2 * len(edge):2] = edge          # odd columns of the first row of every tile
    flat[:, -len(edge):] = edge                    # ... and the end of its last row
    assert ((ndvi.abs() > 1).float().mean() > 0.25) and (ndvi == 1).any() and (ndvi == -1).any()
    return lst, ndvi


# win = 4: one 16-row band, 16 of 256 threads live; 8: one half-filled wave; 20, 36, 60: a partly filled last wave and a last
# band whose staged source rows are clamped at the tile's bottom edge
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("win", [4, 8, 20, 36, 60])
def test_prepare_tiles_every_window(sifsr, win, T):
    lst, ndvi = tile_inputs(1000 * T + win, T, win)
    for stats in (STATS, None):
        for clip in (True, False):
            ref = O.prepare_tiles(lst.double(), ndvi.double(), stats, clip)
            x = sifsr.pipeline.prepare_tiles(lst.cuda(), ndvi.cuda(), stats, clip)
            assert x.shape == ref.shape
            err, bar = (x.cpu().double() - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())
            print(f"win {win} T {T} stats {stats is not None} clip {clip}: err {err:.3e} bar {bar:.3e}")
            assert err < bar, (stats is not None, clip)     # (a NaN fails)
            if clip:                                        # the clip is exact: +-1 and everything beyond land on one value
                for s in (1.0, -1.0):
                    v = x[:, 1][(ndvi[:, 0] * s >= 1).cuda()]
                    assert v.numel() > 0 and (v == v[0]).all()


@pytest.mark.parametrize("win", [20, 4])
def test_granule_to_tiles_equals_batch_form(sifsr, win):
    """44 x 28 granule: 2 x 1 tiles of 20 (ragged on both axes), 11 x 7 tiles of 4.  The granule strides and the batch
    strides feed the same per-tile body: bit-equal."""
    rs = np.random.RandomState(44 + win)
    h, w = 44, 28
    lst_g = rnd(rs, h, w, scale=5.5) + 307.0
    ndvi_g = rnd(rs, 4 * h, 4 * w, scale=1.2) + 0.1
    x, (ty, tx) = sifsr.pipeline.granule_to_tiles(lst_g.cuda(), ndvi_g.cuda(), STATS, window=win)
    assert (ty, tx) == (h // win, w // win) and x.shape == (ty * tx, 2, 4 * win, 4 * win)
    lb = torch.stack([lst_g[i * win:(i + 1) * win, j * win:(j + 1) * win] for i in range(ty) for j in range(tx)])[:, None]
    nb = torch.stack([ndvi_g[4 * i * win:4 * (i + 1) * win, 4 * j * win:4 * (j + 1) * win]
                      for i in range(ty) for j in range(tx)])[:, None]
    want = sifsr.pipeline.prepare_tiles(lb.contiguous().cuda(), nb.contiguous().cuda(), STATS, True)
    assert not torch.isnan(x).any() and torch.equal(x, want)


def check_paste(sifsr, seed, win, tiles, extra):
    ty, tx = tiles
    hr, lst_w = 4 * win, tx * win + extra
    rs = np.random.RandomState(seed)
    sr = rnd(rs, ty * tx, 1, hr, hr)
    out = nans(ty * hr, 4 * lst_w)
    got = sifsr.pipeline.tiles_to_granule(sr.cuda(), out, tiles, win, STATS)
    assert got is out
    out = out.cpu()
    std, mean = np.float32(STATS["std_lst"]), np.float32(STATS["mean_lst"])
    tiled = sr.view(ty, tx, hr, hr).permute(0, 2, 1, 3).reshape(ty * hr, tx * hr)
    # float32 sr*std + mean in the kernel's order: one fused multiply-add (the float32 product is exact in float64), or the
    # product rounded first where the compiler does not contract -- one of the two, on every pixel
    fused = (tiled.double() * float(std) + float(mean)).float()
    split = tiled * torch.tensor(std) + torch.tensor(mean)
    pasted = out[:, :tx * hr]
    assert torch.equal(pasted, fused) or torch.equal(pasted, split), (pasted - fused).abs().max()
    assert torch.isnan(out[:, tx * hr:]).all() and out[:, tx * hr:].numel() == ty * hr * 4 * extra


def test_tiles_to_granule_ragged_margin(sifsr):
    check_paste(sifsr, 5, 4, (3, 2), 3)          # lst_w = 11 > tiles_x * win = 8: a 12-column margin stays untouched


def test_tiles_to_granule_past_the_grid_cap(sifsr):
    assert 33 * 256 * 256 > 8192 * 256           # 33 tiles of 64: the smallest count whose pixels need a second sweep
    check_paste(sifsr, 6, 64, (3, 11), 1)


@pytest.mark.parametrize("shape", [(3, 4, 4), (2, 8, 12), (1, 36, 20), (1, 4096, 4100)])
def test_l4pool4(sifsr, shape):
    """(1,4096,4100): 1024 x 1025 outputs > 4096 * 256, the grid-stride path."""
    B, H, W = shape
    rs = np.random.RandomState(H + W)
    x = rnd(rs, B, 1, H, W, scale=5.5) + 307.0
    ref = O.downsampling_l4(x.double())
    got = sifsr.pipeline.l4pool4(x.cuda())
    assert got.shape == ref.shape
    print(f"l4pool4 {shape}: {rel_err(got, ref):.2e}")
    assert rel_err(got, ref) < 1e-6              # the bar of tests/test_scale_invariance.py (NaN fails)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Fourier
# ---------------------------------------------------------------------------------------------------------------------
# 4x4: nr = 1; a side of 2048: 1024-thread workgroups; 16x512, 2048x8, 8x2048: extreme aspect; 1024x1024: nr = 511, a thread
# of the ring kernels owns two rings
@pytest.mark.parametrize("hw", [(4, 4), (4, 8), (8, 4), (16, 512), (2048, 8), (8, 2048), (512, 512), (1024, 1024)])
def test_fft_and_spectra_sizes(sifsr, hw):
    H, W = hw
    rs = np.random.RandomState(H * 3 + W)
    img = rs.standard_normal((H, W)).astype(np.float32) + np.float32(0.5)
    ref = O.fft2_magnitude_shifted(img)
    x = torch.from_numpy(img).cuda()
    mag = sifsr.fourier.fft2_magnitude(x).cpu().numpy()
    assert mag.shape == ref.shape
    print(f"fft {hw}: {np.abs(mag - ref).max() / ref.max():.2e}")
    assert np.abs(mag - ref).max() < 1e-6 * ref.max()
    spec_ref = np.asarray(O.attenuation_spectrum(ref))
    spec = sifsr.fourier.attenuation_spectra(x).cpu().numpy()
    assert spec.shape == spec_ref.shape == (min(H // 2, W // 2),)
    print(f"spectrum {hw}: {np.abs(spec - spec_ref).max():.2e} dB")
    assert np.allclose(spec, spec_ref, rtol=0, atol=2e-4), np.abs(spec - spec_ref).max()


@pytest.mark.parametrize("hw", [(8, 16), (64, 64)])
def test_fft_closed_form(sifsr, hw):
    H, W = hw
    # a unit impulse away from the origin: |FFT| = 1 everywhere
    for y0, x0 in ((0, 1), (H - 1, W // 2 + 1), (3, 0), (H // 2, W - 3)):
        img = torch.zeros(H, W)
        img[y0, x0] = 1.0
        mag = sifsr.fourier.fft2_magnitude(img.cuda()).cpu().double()
        assert (mag - 1.0).abs().max().item() <= 1e-12, (y0, x0)
    # one plane wave: two conjugate bins of H*W/2.  Phases that are multiples of pi/2 make the float32 image exact
    # (0, +-1), so nothing but the transform's own error is left in the other bins: below 1e-9 H W
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    exact = [(H // 4, W // 4), (H // 2, W // 4), (3 * H // 4, W // 2), (0, 3 * W // 4)]
    general = [(1, 0), (3, 5), (H // 2 - 1, W - 1)]      # float32 samples are rounded: the FFT magnitude bar, 1e-6 max
    for (ky, kx), bar in [(k, 1e-9 * H * W) for k in exact] + [(k, 1e-6 * H * W / 2) for k in general]:
        img = np.cos(2 * np.pi * (ky * yy / H + kx * xx / W)).astype(np.float32)
        mag = sifsr.fourier.fft2_magnitude(torch.from_numpy(img).cuda()).cpu().double().numpy()
        peaks = {((ky + H // 2) % H, (kx + W // 2) % W), ((H - ky + H // 2) % H, (W - kx + W // 2) % W)}
        assert len(peaks) == 2
        rest = np.ones((H, W), dtype=bool)
        for py, px in peaks:
            assert abs(mag[py, px] - H * W / 2) <= max(bar, 1e-6 * H * W / 2), (ky, kx, mag[py, px])
            rest[py, px] = False
        assert mag[rest].max() < bar, (ky, kx, mag[rest].max())     # (NaN fails: max propagates it)


def test_fft_batch_rows_equal_single_calls(sifsr):
    rs = np.random.RandomState(3)
    x = (rnd(rs, 3, 32, 64) * torch.tensor([1.0, 5.5, 0.01]).view(3, 1, 1) + torch.tensor([0.0, 307.0, 0.3]).view(3, 1, 1)).cuda()
    mag, spec = sifsr.fourier.fft2_magnitude(x), sifsr.fourier.attenuation_spectra(x)
    assert not torch.isnan(mag).any() and not torch.isnan(spec).any()
    for i in range(3):
        assert torch.equal(mag[i], sifsr.fourier.fft2_magnitude(x[i]))
        assert torch.equal(spec[i], sifsr.fourier.attenuation_spectra(x[i]))
    assert not torch.equal(mag[0], mag[1]) and not torch.equal(mag[1], mag[2])


# ---------------------------------------------------------------------------------------------------------------------
# 4. Loss operators
# ---------------------------------------------------------------------------------------------------------------------
def loss_inputs(seed, B, H, W):
    rs = np.random.RandomState(seed)
    sr = rnd(rs, B, 1, H, W) * 1.3               # |e| > 1 on a fraction: both Huber branches
    lst = rnd(rs, B, 1, H // 4, W // 4)
    ndvi = rnd(rs, B, 1, H, W).clamp(-3, 3)
    return sr, lst, ndvi


MEAN, STD = 307.2378, 5.5698


# both reflect zones of the 9-tap blur (and of its adjoint) inside ONE partial 32x32 tile, on one axis or both
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(12, 12), (12, 36), (36, 12), (44, 20), (16, 68)])
@pytest.mark.parametrize("kind,gamma", [("sr2", -0.25), ("sr1", -0.5)])
@pytest.mark.parametrize("alpha", [0.5, 0.99])
def test_fused_sif_loss_small(sifsr, alpha, kind, gamma, hw, B):
    H, W = hw
    sr, lst, ndvi = loss_inputs(7 * H + W + B, B, H, W)
    s64 = sr.double().requires_grad_(True)
    ref = O.LOSSES[kind](s64, lst.double(), ndvi.double(), MEAN, STD, alpha, gamma)
    (g_ref,) = torch.autograd.grad(ref[2], s64)
    srd = sr.cuda().requires_grad_(True)
    ds, pl, loss = sifsr.sif_loss(kind, srd, lst.cuda(), ndvi.cuda(), MEAN, STD, alpha, gamma)
    (g,) = torch.autograd.grad(loss, srd)
    for name, got, want in zip(("ds", "pl", "loss"), (ds, pl, loss), ref):
        got, want = float(got.detach()), float(want.detach())
        print(f"{kind} {hw} B{B} a{alpha} {name}: {abs(got - want) / abs(want):.2e}")
        assert abs(got - want) < TOL * abs(want), (name, got, want)
    print(f"{kind} {hw} B{B} a{alpha} grad: {rel_err(g, g_ref):.2e}")
    assert rel_err(g, g_ref) < TOL
    ds2, pl2, loss2, g2 = sifsr.sif_ops.sif_loss_with_grad(kind, sr.cuda(), lst.cuda(), ndvi.cuda(), MEAN, STD, alpha, gamma)
    assert torch.equal(torch.stack([ds2, pl2, loss2]), torch.stack([ds, pl, loss]).detach()) and torch.equal(g2, g)


def check_operator(name, fo, fh, inp):
    a = inp.double().requires_grad_(True)
    yo = fo(a)
    wgt = rnd(np.random.RandomState(sum(inp.shape)), *yo.shape)
    (go,) = torch.autograd.grad((yo * wgt.double()).sum(), a)
    b = inp.clone().cuda().requires_grad_(True)
    yh = fh(b)
    (gh,) = torch.autograd.grad((yh * wgt.cuda()).sum(), b)
    assert yh.shape == yo.shape and gh.shape == go.shape
    print(f"{name} {tuple(inp.shape)}: fwd {rel_err(yh, yo):.2e} grad {rel_err(gh, go):.2e}")
    assert rel_err(yh, yo) < TOL, name
    assert rel_err(gh, go) < TOL, name


# 10 is the smallest side the launchers take: the two 4-pixel reflect zones of the adjoint touch; 17, 33, 11: odd, one past a tile
@pytest.mark.parametrize("hw", [(10, 10), (10, 17), (17, 10), (11, 33)])
def test_blur_and_sobel_smallest(sifsr, hw):
    x = rnd(np.random.RandomState(hw[0] * 50 + hw[1]), 2, 1, *hw)
    check_operator("ftm", lambda t: O.get_output_ftm(t, mtf=0.25), lambda t: sifsr.get_output_ftm(t, mtf=0.25), x)
    check_operator("sobel", O.sobel_bank, sifsr.sobel_bank, x)


@pytest.mark.parametrize("hw", [(12, 12), (12, 36)])
def test_downscale_smallest(sifsr, hw):
    x = rnd(np.random.RandomState(hw[1]), 2, 1, *hw) * STD + MEAN
    check_operator("downscale", O.downscale_LST_SR_to_LR, sifsr.downscale_LST_SR_to_LR, x)


def test_sobel_past_the_grid_cap(sifsr):
    assert 9 * 512 * 512 > 8192 * 256
    check_operator("sobel", O.sobel_bank, sifsr.sobel_bank, rnd(np.random.RandomState(9), 9, 1, 512, 512))


# 1: one element; 255 / 257: a ragged wave around one workgroup; 4097: a ragged second partial block; 1024*4096+5: past the
# 1024-block cap of the partial sums and the 8192*256 elementwise grid of the backward
@pytest.mark.parametrize("n", [1, 255, 257, 4097, 1024 * 4096 + 5])
def test_huber_sizes_and_kinks(sifsr, n):
    rs = np.random.RandomState(n % 9973)
    a, t, scale = rnd(rs, n) * 1.5, rnd(rs, n), -0.5
    # |e| = 1 exactly and 1 -+ 2^-20, both signs, e = a - scale*t formed without rounding: t = 2, a = e - 1
    kinks = torch.tensor([1.0, -1.0, 1 + 2.0 ** -20, 1 - 2.0 ** -20, -1 - 2.0 ** -20, -1 + 2.0 ** -20])[:n]
    at = torch.linspace(0, n - 1, len(kinks)).long()
    t[at], a[at] = 2.0, kinks - 1.0
    assert torch.equal((a[at].double() - scale * t[at].double()), kinks.double())
    a64 = a.double().requires_grad_(True)
    lo = O.huber(a64, scale * t.double())
    (go,) = torch.autograd.grad(lo * 1.7, a64)
    ad = a.cuda().requires_grad_(True)
    lh = sifsr.huber_loss(ad, t.cuda(), scale)
    (gh,) = torch.autograd.grad(lh * 1.7, ad)
    print(f"huber n={n}: value {abs(float(lh) - float(lo)) / abs(float(lo)):.2e} grad {rel_err(gh, go):.2e}")
    assert abs(float(lh.detach()) - float(lo.detach())) < TOL * abs(float(lo.detach()))
    assert rel_err(gh, go) < TOL
    assert rel_err(gh.cpu()[at], go[at]) < TOL           # the planted elements alone (|clamp(e)| = 1 or 1 - 2^-20)


# ---------------------------------------------------------------------------------------------------------------------
# 5. Adam
# ---------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def adam_problem(seed, n, steps=5):
    """Parameters at the scale of the network's weights (|p| < 0.5: a float32 ulp of p is below 1e-4 of one update) and
    gradients at the scale of the model's."""
    rs = np.random.RandomState(seed)
    return rnd(rs, n, scale=0.1), [rnd(rs, n, scale=0.01) for _ in range(steps)]


@pytest.mark.parametrize("n", [1, 255, 257, 10007])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_adam_flat_vs_torch_float64(L, weight_decay, grad_scale, n):
    p0, grads = adam_problem(n + int(100 * weight_decay) + int(8 * grad_scale), n)
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=weight_decay)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step, g in enumerate(grads, 1):
        ref.grad = g.double()
        opt.step()
        L.call("sifsr_adam_flat", p, dev(g / grad_scale), m, v, n, LR, B1, B2, EPS, weight_decay, step, grad_scale, S())
    torch.cuda.synchronize()
    st = opt.state[ref]
    errs = (rel_err(p, ref), rel_err(p.cpu() - p0, ref.detach() - p0.double()), rel_err(m, st["exp_avg"]), rel_err(v, st["exp_avg_sq"]))
    print(f"adam n={n} wd={weight_decay} gs={grad_scale}: p {errs[0]:.2e} update {errs[1]:.2e} m {errs[2]:.2e} v {errs[3]:.2e}")
    assert errs[0] < 1e-6
    assert errs[1] < 1e-4
    # the first moment at the bar of the parameter (float32 rounding alone); the second at the bar of the update: its
    # (1 - beta2) is formed from the float32 beta2 of the C ABI, 1.3e-5 relative from 1 - 0.999 in float64 (the bias
    # correction uses the same float32 beta2, so the update does not see it)
    assert errs[2] < 1e-6 and errs[3] < 1e-4


def test_adam_flat_late_step(L):
    """step = 1000 on a running state: both bias corrections are near 1 (0.632 for beta2), against the float64 formula in
    the header of csrc/adam.hip."""
    n, step, wd, gs = 4099, 1000, 1e-2, 0.25
    rs = np.random.RandomState(1000)
    p0, g = rnd(rs, n, scale=0.1), rnd(rs, n, scale=0.01)
    m0, v0 = rnd(rs, n, scale=0.005), (rnd(rs, n, scale=0.01) ** 2 + 1e-6)
    gi = g.double() + wd * p0.double()
    m_ref = m0.double() + (1 - B1) * (gi - m0.double())
    v_ref = B2 * v0.double() + (1 - B2) * gi * gi
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    upd_ref = -(LR / bc1) * m_ref / (v_ref.sqrt() / math.sqrt(bc2) + EPS)
    p, m, v = dev(p0), dev(m0), dev(v0)
    L.call("sifsr_adam_flat", p, dev(g / gs), m, v, n, LR, B1, B2, EPS, wd, step, gs, S())
    torch.cuda.synchronize()
    errs = (rel_err(p, p0.double() + upd_ref), rel_err(p.cpu() - p0, upd_ref), rel_err(m, m_ref), rel_err(v, v_ref))
    print(f"adam late step: p {errs[0]:.2e} update {errs[1]:.2e} m {errs[2]:.2e} v {errs[3]:.2e}")
    assert errs[0] < 1e-6 and errs[1] < 1e-4 and errs[2] < 1e-6 and errs[3] < 1e-4


@pytest.mark.parametrize("n", [1, 10007])
def test_adam_flat_dev_replays_equal_host_steps(L, n):
    """The device-resident step count: 5 replays from a zeroed counter == sifsr_adam_flat with steps 1..5, bit for bit."""
    wd, gs = 1e-2, 0.25
    p0, grads = adam_problem(n + 5, n)
    ph, mh, vh = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pd, md, vd = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    coef2 = nans(2)
    for step, g in enumerate(grads, 1):
        gd = dev(g / gs)
        L.call("sifsr_adam_flat", ph, gd, mh, vh, n, LR, B1, B2, EPS, wd, step, gs, S())
        L.call("sifsr_adam_flat_dev", pd, gd, md, vd, n, LR, B1, B2, EPS, wd, counter, coef2, gs, S())
    torch.cuda.synchronize()
    assert int(counter.item()) == 5
    assert not torch.isnan(pd).any() and not torch.equal(pd, dev(p0))
    assert torch.equal(pd, ph) and torch.equal(md, mh) and torch.equal(vd, vh)
