"""GPU: Fourier scores for rasters of any size (include/sifsr_spectra.h, sifsr/spectra.py) against the reference's
values in tests/golden/golden_spectra_v1.json and the float64 oracle (np.fft.fft2).

Sizes: those of tests/golden/make_golden_spectra.py, the smallest at which each part of the chirp-z kernel can go wrong (primes,
2^k + 1 and 2^k - 1, even non-powers, one radix-2 axis beside one chirp axis in both orders, a typical crop, n ~ 1000 for the
integer phase reduction and the LDS maximum, a power-of-two side above 512 beside a chirp side).

Bars, all of them the existing ones of tests/test_fourier.py: magnitude within 1e-6 of the largest bin (a float32 output of a float64
transform); spectra within 2e-4 dB of the REFERENCE's values; scores within rtol 1e-4 / atol 1e-6.  A float64 NumPy model of this
algorithm stays within 2.3e-8 dB of np.fft.fft2 over such sizes, so the dB bar is four orders of magnitude above what the method
needs; a float32 dB value near -100 carries 4e-6 dB of its own.  Every test prints what it measures."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests.golden.make_golden_spectra import CASES, SCORES, fourier_case
from tests.contract import L, S, execute, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import Plain, bit_equal

pytestmark = pytest.mark.gpu
SHAPE_ERR, ARG_ERR, WORKSPACE_ERR = 1001, 1002, 1003
DB_TOL = 2e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_spectra_v1.json")))


_IMAGES = {}


def images(seed, H, W):
    """the three images of a case and their float64 magnitudes, computed once and left unchanged"""
    if (seed, H, W) not in _IMAGES:
        imgs = fourier_case(seed, H, W)
        mags = [O.fft2_magnitude_shifted(im) for im in imgs]
        for a in (*imgs, *mags):
            a.setflags(write=False)
        _IMAGES[(seed, H, W)] = (imgs, mags)
    return _IMAGES[(seed, H, W)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the golden cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{h}x{w}" for _, h, w in CASES])
def test_golden_case(sifsr, idx):
    c = GOLD["cases"][idx]
    assert (c["seed"], c["H"], c["W"]) == CASES[idx]
    imgs, refs = images(*CASES[idx])
    x = dev(np.stack(imgs))
    mag = sifsr.spectra.fft2_magnitude(x).cpu().numpy()
    spec = sifsr.spectra.attenuation_spectra(x).cpu().numpy()
    assert mag.shape == x.shape and mag.dtype == np.float32 and spec.shape == (3, min(c["H"] // 2, c["W"] // 2))
    d_mag = max(float(np.abs(mag[i] - refs[i]).max() / refs[i].max()) for i in range(3))
    d_db = max(float(np.abs(spec[i] - np.array(c["spectra"][i])).max()) for i in range(3))
    rb, xb, pb = spec
    got = sifsr.spectra.scores_from_spectra(rb, xb, pb)
    want = np.array([c[k] for k in SCORES])
    print(f"{c['H']}x{c['W']}: max |mag - ref| / max ref = {d_mag:.3e}, max |dB - reference| = {d_db:.3e} "
          f"(min dB {min(min(s) for s in c['spectra']):.1f}), scores {got.tolist()} vs {want.tolist()}")
    assert d_mag < 1e-6                                            # float32 output of a float64 transform
    assert d_db <= DB_TOL
    assert np.allclose(got, want, rtol=1e-4, atol=1e-6)


# ---- 2. closed forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(41, 53), (1000, 48)])
def test_closed_forms(sifsr, hw):
    H, W = hw
    imp = torch.zeros((H, W), device="cuda")
    imp[H // 3, W - 2] = 1.0                                       # off the origin: every bin is a pure phase
    mag = sifsr.spectra.fft2_magnitude(imp)
    spec = sifsr.spectra.attenuation_spectra(imp)
    d_imp = float((mag.double() - 1).abs().max())
    c = 300.25
    const = torch.full((H, W), c, device="cuda")
    m = sifsr.spectra.fft2_magnitude(const).double().cpu()
    centre = float(m[H // 2, W // 2])
    m[H // 2, W // 2] = 0
    print(f"{H}x{W}: impulse max ||X| - 1| = {d_imp:.3e}, max |dB| = {float(spec[1:].abs().max()):.3e}; constant: centre {centre} vs "
          f"{H * W * c}, largest other bin / centre = {float(m.max()) / centre:.3e}")
    assert d_imp < 1e-6 and float(spec[0]) == 1.0 and float(spec[1:].abs().max()) <= DB_TOL
    assert abs(centre - H * W * c) <= 1e-6 * H * W * c and float(m.max()) <= 1e-6 * centre


# ---- 3. bit equality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(64, 128), (256, 256)])
def test_power_of_two_shapes_give_the_bits_of_sifsr_fourier(sifsr, hw):
    x = dev(np.stack(fourier_case(31, *hw)))
    assert torch.equal(sifsr.spectra.fft2_magnitude(x), sifsr.fourier.fft2_magnitude(x))
    assert torch.equal(sifsr.spectra.attenuation_spectra(x), sifsr.fourier.attenuation_spectra(x))
    assert torch.equal(sifsr.spectra.attenuation_spectra(x[1]), sifsr.fourier.attenuation_spectra(x[1]))


@pytest.mark.parametrize("hw", [(41, 53), (100, 256), (33, 65)])
def test_a_batch_row_is_its_own_call(sifsr, hw):
    x = dev(np.stack(fourier_case(32, *hw)))
    mag, spec = sifsr.spectra.fft2_magnitude(x), sifsr.spectra.attenuation_spectra(x)
    for i in range(3):
        assert torch.equal(sifsr.spectra.fft2_magnitude(x[i]), mag[i]) and torch.equal(sifsr.spectra.attenuation_spectra(x[i:i + 1])[0], spec[i])
    assert torch.equal(sifsr.spectra.fft2_magnitude(x), mag)        # and the same bits on a second run


def test_a_list_of_mixed_sizes_is_the_per_raster_calls(sifsr):
    sizes = [(41, 53), (64, 128), (41, 53), (48, 100), (53, 41)]
    rasters = [dev(fourier_case(40 + i, h, w)[i % 3]) for i, (h, w) in enumerate(sizes)]
    mags, specs = sifsr.spectra.fft2_magnitude(rasters), sifsr.spectra.attenuation_spectra(rasters)
    assert isinstance(mags, list) and isinstance(specs, list) and len(mags) == len(specs) == len(sizes)
    for r, m, s in zip(rasters, mags, specs):
        assert m.shape == r.shape and s.shape == (min(r.shape[0] // 2, r.shape[1] // 2),)
        assert torch.equal(m, sifsr.spectra.fft2_magnitude(r)) and torch.equal(s, sifsr.spectra.attenuation_spectra(r))
    assert not torch.equal(mags[0], mags[2])                        # two rasters of one shape went down together and stayed apart


# ---- 4. the scores of whole pairs -----------------------------------------------------------------------------------------------
def test_spectral_scores_of_pairs(sifsr):
    sizes = [(41, 53), (48, 100), (100, 64)]
    aster, bic, preds, want = [], [], [], []
    for i, (h, w) in enumerate(sizes):
        t, b, p = fourier_case(50 + i, h, w)
        p2 = (0.5 * (t + p)).astype(np.float32)
        aster.append(dev(t)); bic.append(dev(b))
        preds.append(dev(np.stack((p, p2))) if i != 1 else [dev(p), dev(p2)])          # a stack, or a list of K rasters
        rb, xb = (np.array(O.attenuation_spectrum(O.fft2_magnitude_shifted(v))) for v in (t, b))
        rows = []
        for q in (p, p2):
            pb = np.array(O.attenuation_spectrum(O.fft2_magnitude_shifted(q)))
            frr, fro, fru = O.frr_fro_fru(pb, rb, xb)
            pfr = np.maximum(rb - xb, 0).sum()
            rows.append([pfr, frr * pfr, frr, fro, fru, np.sqrt(np.mean((pb - rb) ** 2))])
        want.append(rows)
    want = np.array(want)
    got = sifsr.spectra.spectral_scores(aster, bic, preds)
    print("max relative deviation per score:", (np.abs(got - want) / np.maximum(np.abs(want), 1e-12)).max(axis=(0, 1)).tolist())
    assert got.shape == (3, 2, 6) and got.dtype == np.float64
    assert np.allclose(got, want, rtol=1e-4, atol=1e-6)
    one = sifsr.spectra.spectral_scores(aster[0], bic[0], preds[0])
    assert one.shape == (1, 2, 6) and np.array_equal(one[0], got[0])
    rows = sifsr.spectra.summary_rows(got[:, :, 2:], ddof=0)
    assert rows.shape == (7, 2, 4) and np.allclose(rows[0], got[:, :, 2:].mean(axis=0)) and np.allclose(rows[1], got[:, :, 2:].std(axis=0))
    with pytest.raises(sifsr.SifsrError):
        sifsr.spectra.spectral_scores(aster[0], bic[1], preds[0])                      # sizes of one pair must agree


# ---- 5. the C entry point: errors, memory contract -------------------------------------------------------------------------------
def test_errors_launch_nothing(sifsr, L):
    fn, size = L.lib().sifsrf_fft2_attenuation, L.lib().sifsrf_fft2_attenuation_scratch_bytes
    B, H, W = 1, 41, 53
    need = size(B, H, W)
    img = torch.full((B, 1025, 64), 77.0, device="cuda")                               # large enough for every shape tried below
    mag = torch.full((B, 1025, 64), 77.0, device="cuda")
    spec = torch.full((B, 64), 77.0, device="cuda")
    ws = torch.full((size(1, 1024, 64) + 16,), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    args = lambda **kw: [kw.get("img", p(img)), kw.get("B", B), kw.get("H", H), kw.get("W", W), kw.get("ws", p(ws)),
                         kw.get("nbytes", ws.numel()), kw.get("mag", p(mag)), kw.get("spec", p(spec)), S()]
    for bad in (dict(H=3, W=64), dict(H=1025, W=64), dict(H=64, W=1025), dict(H=64, W=3), dict(B=0), dict(H=3000, W=64)):
        assert fn(*args(**bad)) == SHAPE_ERR, bad
    for bad in (dict(img=None), dict(ws=None), dict(mag=None, spec=None)):
        assert fn(*args(**bad)) == ARG_ERR, bad
    for bad in (dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=L.lib().sifsr_fft2_attenuation_scratch_bytes(B, H, W))):
        assert fn(*args(**bad)) == WORKSPACE_ERR, bad                                  # a short scratch buffer is refused
    torch.cuda.synchronize()
    for t in (img, mag, spec, ws):
        assert (t == 77).all()
    assert fn(*args(nbytes=need)) == 0
    torch.cuda.synchronize()
    assert (img == 77).all() and (ws[need:] == 77).all() and (mag.flatten()[H * W:] == 77).all() and (spec.flatten()[20:] == 77).all()
    for call in (lambda: sifsr.spectra.fft2_magnitude(torch.zeros(41, 53)), lambda: sifsr.spectra.attenuation_spectra([torch.zeros(41, 53)]),
                 lambda: sifsr.spectra.fft2_magnitude(torch.zeros(1, 3, 64).cuda()), lambda: sifsr.spectra.fft2_magnitude(torch.zeros(1025, 64).cuda()),
                 lambda: sifsr.spectra.fft2_magnitude(torch.zeros(41, 53, dtype=torch.float64).cuda())):
        with pytest.raises(sifsr.SifsrError):
            call()


# (B, H, W, mag, spectrum)
CONTRACT_SHAPES = [(b, h, w, m, s) for (b, h, w) in ((2, 41, 53), (1, 100, 256), (1, 33, 65))
                   for (m, s) in ((True, True), (True, False), (False, True))]


def contract_input(i):
    B, H, W = CONTRACT_SHAPES[i][:3]
    return np.stack(fourier_case(60 + i // 3, H, W)[:B])            # one input per shape, whichever outputs are asked for


def spectra_case(i):
    def make(k):
        B, H, W, want_mag, want_spec = CONTRACT_SHAPES[i]
        img = k.t("img", torch.from_numpy(contract_input(i)))
        mag = k.o("mag", B, H, W) if want_mag else None
        spec = k.o("spectrum", B, min(H // 2, W // 2)) if want_spec else None
        need = k.L.call("sifsrf_fft2_attenuation_scratch_bytes", B, H, W)
        ws = k.A.scratch(need, "scratch")                           # poisoned scratch: nothing of it may reach the outputs
        call = lambda: k.L.call("sifsrf_fft2_attenuation", img, B, H, W, ws, need, mag, spec, S())
        outs = {}
        if want_mag:
            outs["mag"] = mag
        if want_spec:
            outs["spectrum"] = spec
        return call, outs
    return make


CONTRACT = {"sifsrf_fft2_attenuation": [spectra_case(i) for i in range(len(CONTRACT_SHAPES))]}


@pytest.mark.parametrize("idx", range(len(CONTRACT_SHAPES)), ids=["%dx%dx%d-mag%d-spec%d" % s for s in CONTRACT_SHAPES])
def test_memory_contract(L, idx):
    """mag and spectrum written in full and nowhere else -- bit-identical and NaN-free under every poison of the outputs and of the
    scratch buffer (the zero padding up to M, the filter spectra and the ring partials are written before they are read) --, img
    untouched, nothing outside the stated scratch bytes written, the same bits on ordinary allocations and with the other output
    absent, and the result is the oracle's."""
    cases = CONTRACT["sifsrf_fft2_attenuation"]
    first = run_contract(L, cases[idx], seed=1977 + idx, capacity=16 << 20)
    B, H, W, want_mag, want_spec = CONTRACT_SHAPES[idx]
    x = contract_input(idx)
    if not (want_mag and want_spec):                    # an output does not depend on whether the other one was asked for
        j = CONTRACT_SHAPES.index((B, H, W, True, True))
        both = execute(L, Plain("cuda"), cases[j], seed=1977 + j)
        for n, v in first.items():
            assert bit_equal(v, both[n]), n
    for b in range(B):
        ref = O.fft2_magnitude_shifted(x[b])
        if want_mag:
            assert np.abs(first["mag"][b].cpu().numpy() - ref).max() < 1e-6 * ref.max()
        if want_spec:
            assert np.abs(first["spectrum"][b].cpu().numpy() - np.array(O.attenuation_spectrum(ref))).max() <= DB_TOL
