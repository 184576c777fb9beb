"""Host-side half of the weight-gradient edge tests (tests/wgrad_reference.py, tests/test_wgrad_edge_gpu.py): the float64
restatements against autograd, the mirror of the launch geometry against hand-computed values, and the power of the bar -- every
mutation a subtly wrong kernel could produce must fail the check the GPU file applies, for every case it runs."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests import storage_reference as R
from tests import wgrad_reference as WR

CSRC = next(Path(__file__).resolve().parents[1].glob("*_amd")) / "csrc"


def autograd_wgrad(a, g, cout):
    w = torch.zeros(cout, a.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(a.double(), (1, 1, 1, 1), mode="replicate"), w)
    (gw,) = torch.autograd.grad(y, w, g.double())
    return gw


RESTATE_SHAPES = [(1, 1, 1), (2, 2, 2), (1, 1, 17), (2, 9, 1), (3, 7, 15), (2, 2, 18), (1, 10, 2), (2, 6, 14), (1, 20, 40), (2, 9, 17)]


@pytest.mark.parametrize("shape", RESTATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatements_match_autograd(shape):
    B, H, W = shape
    gen = torch.Generator().manual_seed(100 * H + W)
    a = torch.randn(B, 5, H, W, generator=gen, dtype=torch.float64)
    g = torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64)
    ref = autograd_wgrad(a, g, 3)
    scale = R.conv3_rep_wgrad(a.abs(), g.abs())
    assert bool(((R.conv3_rep_wgrad(a, g) - ref).abs() <= 1e-13 * scale).all())
    if H % 2 == 0 and W % 2 == 0:
        assert bool(((WR.wino_wgrad(a, g) - ref).abs() <= 1e-13 * WR.wino_wgrad(a, g, absolute=True)).all())
        # the Winograd yardstick dominates the tap-domain one: |sum of transformed products| <= sum of |...|
        assert bool((WR.wino_wgrad(a, g, absolute=True) >= scale * (1 - 1e-13)).all())
    else:
        with pytest.raises(AssertionError):
            WR.wino_wgrad(a, g)


def test_mirror_on_the_models_layers_at_64x64():
    """hand-computed: the four levels of a 64x64 patch, B = 64 (BASELINE.json's batch)"""
    L = WR.Launch(64, 64, 64, 1536)                 # 8x4 tiles of 8x16: 32 per image, 6x2 interior
    assert (L.ty, L.tx, L.ntiles, L.nblk, L.pow2) == (8, 4, 2048, 1536, True)
    assert L.kinds == {"interior": 64 * 12, "border": 64 * 20, "partial": 0} and (L.tmin, L.tmax) == (1, 2)
    L = WR.Launch(64, 32, 32, 384)                  # 4x2 tiles: no tile has a neighbour on both sides in x
    assert (L.ty, L.tx, L.ntiles, L.pow2) == (4, 2, 512, True) and L.kinds == {"interior": 0, "border": 512, "partial": 0}
    assert (L.tmin, L.tmax, L.terms_per_workgroup()) == (1, 2, 256)
    L = WR.Launch(64, 16, 16, 4096)                 # 2x1 tiles; the request is clamped
    assert (L.ty, L.tx, L.ntiles, L.nblk, L.pow2) == (2, 1, 128, 128, True) and L.kinds["border"] == 128
    L = WR.Launch(64, 8, 8, 16)                     # one half-wide tile per image
    assert (L.ty, L.tx, L.ntiles, L.pow2) == (1, 1, 64, True) and L.kinds == {"interior": 0, "border": 0, "partial": 64}
    assert (L.tmin, L.tmax) == (4, 4)
    # (C0, C1, cout) of the model's 3x3 layers -> tap (NBO, NBI, chunks), Winograd (NBO, NBI, halves, chunks), EL
    layers = {
        (16, 0, 16): ((1, 1, 1), (1, 1, 1, 1), 4), (16, 0, 32): ((2, 1, 1), (2, 1, 1, 1), 8), (32, 0, 32): ((2, 2, 1), (2, 2, 1, 1), 16),
        (32, 0, 64): ((4, 2, 1), (2, 2, 2, 1), 32), (64, 0, 64): ((4, 2, 2), (2, 2, 2, 2), 32), (64, 64, 64): ((4, 2, 4), (2, 2, 2, 4), 32),
        (64, 0, 32): ((2, 2, 2), (2, 2, 1, 2), 32), (32, 32, 32): ((2, 2, 2), (2, 2, 1, 2), 32), (32, 0, 16): ((1, 2, 1), (1, 2, 1, 1), 8),
        (16, 16, 16): ((1, 1, 2), (1, 2, 1, 1), 8),
    }
    for (C0, C1, cout), (tap, wino, el) in layers.items():
        assert WR.tap_variant(C0, C1, cout) == tap, (C0, C1, cout)
        assert WR.wino_variant(C0, C1, cout, 64, 64) == wino, (C0, C1, cout)
        assert WR.reduce_el(C0 + C1, cout) == (el, 256 // el), (C0, C1, cout)
    assert WR.wino_straddles(16, 16) and not WR.wino_straddles(32, 32) and not WR.wino_straddles(16, 32)


def test_mirror_index_forms_and_tile_kinds():
    """the regimes of the issue's shape table, by hand"""
    expect = {   # (H, W): (ty, tx, pow2, interior, border, partial) for one image
        (20, 40): (3, 3, False, 1, 3, 5), (24, 48): (3, 3, False, 1, 8, 0), (32, 64): (4, 4, True, 4, 12, 0),
        (30, 60): (4, 4, True, 4, 5, 7), (8, 16): (1, 1, True, 0, 1, 0), (10, 18): (2, 2, True, 0, 1, 3),
        (6, 14): (1, 1, True, 0, 0, 1), (2, 2): (1, 1, True, 0, 0, 1), (2, 18): (1, 2, True, 0, 0, 2), (10, 2): (2, 1, True, 0, 0, 2),
        (1, 1): (1, 1, True, 0, 0, 1), (21, 37): (3, 3, False, 1, 3, 5), (9, 17): (2, 2, True, 0, 1, 3),
    }
    for (H, W), (ty, tx, pow2, ni, nb, npart) in expect.items():
        L = WR.Launch(1, H, W, 1)
        assert (L.ty, L.tx, L.pow2) == (ty, tx, pow2), (H, W)
        assert L.kinds == {"interior": ni, "border": nb, "partial": npart}, (H, W, L.kinds)
    # generic walk of 3 images of 3x3 tiles on 4 workgroups: tile 13 = image 1, row 1, column 1 -- the interior one
    L = WR.Launch(3, 20, 40, 4)
    assert L.where[(1, 1, 1)] == (3, 1) and L.counts == [7, 7, 7, 6]
    # power-of-two walk, 3 images of 4x4: tile 37 = image 2, row 1, column 1
    L = WR.Launch(3, 32, 64, 48 + 5)
    assert L.nblk == 48 and L.where[(2, 1, 1)] == (0, 37) and (L.tmin, L.tmax) == (1, 1)
    assert WR.nblk_values(48, 16) == {"one": 1, "ntiles": 48, "clamped": 53, "uneven": 5, "below_groups": 3, "ragged_groups": 19}
    assert WR.nblk_values(1, 64) == {"one": 1, "ntiles": 1, "clamped": 6}
    assert WR.nblk_values(2, 8) == {"one": 1, "ntiles": 2, "clamped": 7}


def test_chunking_tiles_cin_for_every_pair_of_sources():
    """nbi_chunk and chunks for every (C0, C1) the GPU file uses and every power-of-two pair up to 128: the chunks cover Cin exactly
    and a tap chunk lies in one source."""
    pairs = {(c.C0, c.C1) for c in WR.CASES + WR.GUARD_CASES + WR.GUARD_WINO_CASES}
    pairs |= {(a, b) for a in (16, 32, 64, 128) for b in (0, 16, 32, 64, 128)}
    for C0, C1 in sorted(pairs):
        cin = C0 + C1
        nbi = WR.tap_nbi_chunk(C0, C1)
        assert (cin // 16) % nbi == 0, (C0, C1)
        for q0 in range(0, cin // 16, nbi):
            assert (q0 < C0 // 16) == (q0 + nbi - 1 < C0 // 16) or not C1, (C0, C1, q0)
        assert (cin // 16) % WR.wino_nbi_chunk(cin) == 0, (C0, C1)
    hand = {(16, 0): (1, 1), (32, 0): (2, 2), (64, 0): (2, 2), (32, 32): (2, 2), (64, 64): (2, 2), (16, 16): (1, 2), (64, 32): (2, 2),
            (16, 32): (1, 1), (16, 64): (1, 1), (32, 16): (1, 1), (64, 16): (1, 1)}
    for (C0, C1), (tap, wino) in hand.items():
        assert (WR.tap_nbi_chunk(C0, C1), WR.wino_nbi_chunk(C0 + C1)) == (tap, wino), (C0, C1)


def test_guard_cases_in_the_mirror():
    """cat(32, 16) and cat(16, 32): 16-channel chunks, so three chunks that tile the 48 channels; where no kernel variant exists for
    the resulting (NBO, NBI) the launchers return the shape error before any launch"""
    assert WR.tap_variant(32, 16, 16) == (1, 1, 3) and WR.tap_variant(32, 16, 32) == (2, 1, 3)
    assert WR.tap_variant(32, 16, 64) is None and WR.tap_variant(64, 16, 64) is None        # no (4, 1) kernel
    assert WR.wino_variant(16, 32, 16, 20, 40) == (1, 1, 1, 3) and WR.wino_variant(16, 32, 32, 10, 18) == (2, 1, 1, 3)
    assert WR.wino_variant(16, 32, 64, 20, 40) is None                                       # no NBO = 4, NBI = 1 kernel
    assert WR.wino_variant(16, 0, 16, 21, 40) is None and WR.tap_variant(48, 0, 16) is None


def test_mirror_agrees_with_the_sources():
    """the chunk functions and the guards the mirror restates are the ones in the kernels' launchers"""
    tap, wino = (CSRC / "conv_wgrad.hip").read_text(), (CSRC / "conv_wgrad_wino.hip").read_text()
    assert re.search(r"int wgrad_nbi_chunk\(const WgradArgs& a, int cin\) \{\s*if \(cin < 32 \|\| \(cin / 16\) % 2\) return 1;", tap)
    assert "int wgrad_wino_nbi_chunk(int cin) { return (cin < 32 || (cin / 16) % 2) ? 1 : 2; }" in wino
    for src in (tap, wino):
        assert "if ((cin / 16) % nbi) return SIFSR_ERR_SHAPE;" in src
    assert [tuple(map(int, m)) for m in re.findall(r"SIFSR_WG\((\d), (\d)\)", tap)][-5:] == list(WR.TAP_VARIANTS)
    assert [tuple(map(int, m)) for m in re.findall(r"SIFSR_XW\((\d), (\d), (\d)\)", wino)] == list(WR.WINO_VARIANTS)
    # the engine's batched reduction takes nbi_chunk from the same two functions
    eng = (CSRC / "engine.hip").read_text()
    assert "const int nbi = wino ? wgrad_wino_nbi_chunk(L.cin) : wgrad_nbi_chunk(a, L.cin);" in eng and "j.nbi_chunk = nbi;" in eng


def test_case_table_covers_the_matrix():
    """what the issue asks of the case table, from the mirror alone"""
    by_form = {}
    els = {}
    for c in WR.CASES:
        assert c.B * c.H * c.W <= 8192, c
        nt = WR.Launch(c.B, c.H, c.W, 1).ntiles
        el, groups = WR.reduce_el(c.C0 + c.C1, c.cout)
        els.setdefault(el, set()).update(WR.nblk_values(nt, groups))
        tv = WR.tap_variant(c.C0, c.C1, c.cout)
        wv = WR.wino_variant(c.C0, c.C1, c.cout, c.H, c.W)
        assert tv is not None, c
        for form in WR.forms_of(c):
            key = (form, tv[:2]) if form in ("tap", "fused", "bf16") else (form, wv[:3])
            by_form.setdefault(key, set()).add((c.H, c.W))
    small = {(8, 16), (10, 18), (6, 14), (2, 2), (2, 18), (10, 2)}
    for form in ("tap", "fused", "bf16"):
        for v in WR.TAP_VARIANTS:
            s = by_form.get((form, v), set())
            assert {(20, 40), (32, 64), (30, 60)} <= s and len(s & small) >= 2, (form, v, sorted(s))
    for form in ("wino", "wino_fused"):
        for v in WR.WINO_VARIANTS:
            s = by_form.get((form, v), set())
            assert {(20, 40), (32, 64), (30, 60)} <= s and len(s & small) >= 2, (form, v, sorted(s))
    shapes = {(c.H, c.W) for c in WR.CASES}
    assert small | {(24, 48), (1, 1), (1, 17), (9, 1), (7, 15), (9, 17), (21, 37)} <= shapes
    assert {c.B for c in WR.CASES} >= {1, 3}
    assert any(c.B == 3 and WR.Launch(c.B, c.H, c.W, 1).pow2 and (c.H, c.W) == (32, 64) for c in WR.CASES)
    for el in (4, 8, 16, 32):
        assert els[el] == {"one", "ntiles", "clamped", "uneven", "below_groups", "ragged_groups"}, (el, els[el])
    srcs = {(c.C0, c.C1) for c in WR.CASES}
    assert {(32, 32), (64, 64), (16, 16), (64, 32), (16, 32), (16, 64)} <= srcs
    assert any(c.C1 == 0 and c.aff == "-" for c in WR.CASES) and any(c.C1 == 0 and c.aff == "a" for c in WR.CASES)
    assert any(c.C1 and c.C0 != c.C1 and c.aff in ("a-", "-a") for c in WR.CASES)
    assert any(WR.wino_straddles(c.C0, c.C1) and "wino" in WR.forms_of(c) for c in WR.CASES)


@pytest.mark.parametrize("case", WR.CASES + WR.GUARD_CASES + WR.GUARD_WINO_CASES, ids=WR.case_id)
def test_the_bar_rejects_every_mutation(case):
    """A condition, not a measurement: each mutant of the float64 reference, rounded to fp32, must fail check_sum at BAR_SUM
    against the yardstick of every form the case is compared under -- Winograd's (the largest) included.  The unmutated
    reference, rounded to fp32, must pass."""
    d = WR.data(case)
    forms = WR.forms_of(case)
    assert forms, case
    seen = set()
    for form in forms:
        ref, yard = d.expect(form)
        assert bool((yard >= ref.abs() * (1 - 1e-12)).all())
        R.check_sum(ref.float(), ref, yard, R.BAR_SUM, (form, "the reference itself"))
        for name, m in WR.mutants(d, form):
            seen.add(name)
            assert m.shape == ref.shape
            with pytest.raises(AssertionError):
                R.check_sum(m.float(), ref, yard, R.BAR_SUM, (form, name))
    assert {"dropped pixel", "last block dropped"} <= seen
    assert ("wrong-side clamp" in seen) == (case.H > 1 or case.W > 1)
    assert ("second source's affine from the first" in seen) == bool(case.C1)
    stray = case.W if case.W % 16 else case.H * case.W if case.H % 8 else None      # the pixel the stray address lands on
    assert ("stray out-of-image pixel" in seen) == (stray is not None and stray < case.B * case.H * case.W), (case, seen)
