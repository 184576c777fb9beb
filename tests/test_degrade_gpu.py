"""GPU: the sensor model at any ratio (include/sifsr_degrade.h, sifsr/degrade.py) against the float64 NumPy
restatement tests/degrade_reference.py (held to the reference's recorded outputs by tests/test_degrade_host.py) and against those
outputs themselves (tests/golden/golden_degrade_v1.npz).

TOL, device against restatement: 2e-4 K, the bar sifsr.conserve is held to for the same operator family at the same magnitudes.  The
kernels accumulate in float64 and round to fp32 once, so the floor is half an fp32 ulp at 300 K, 1.5e-5 K.  Measured on an MI355X
over every case of this file (printed by each test): the largest |device - restatement| is 1.66e-5 K (fine_61x83), the largest
|device - reference| 3.05e-4 K (coarse_97x131) and the largest |degrade(x, 4, crop) - downscale_LST_SR_to_LR| 9.2e-5 K.  Against the
reference's fp32 outputs the bar is the host bar of tests/test_degrade_host.py (6.2e-4 K) plus TOL.

Shapes, the smallest at which each part can go wrong: the golden cases (12 x 12 and 4 x 4 are the minimum for their half widths:
both reflections and both clamps meet in one stencil), 12 x 2048 and 2048 x 12 strips (many workgroups along one axis, one stencil
covering the whole other axis), rasters whose width, output width and output height are one less than, equal to and one more than
the kernels' tile (BX = 64 lanes along a row, BY = 4 output rows per workgroup, read from csrc/degrade.hip), the 4 x 3415 strip on
which the fp32 source coordinate first floors differently from the float64 one, and one 700 x 830 scene for both ASTER factors."""
import os
import re

import numpy as np
import pytest
import torch

from tests import degrade_reference as R
from tests.contract import L, S, bits, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal
from tests.test_degrade_host import HOST_BAR

pytestmark = pytest.mark.gpu
TOL = 2e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_degrade_v1.npz")
_SRC = open(os.path.join(ROOT, "land-surface-temperature-super-resolution-with-a-scale-invariance-free-neural-approach_amd", "csrc",
                         "degrade.hip")).read()
BX = int(re.search(r"constexpr int BX = (\d+);", _SRC).group(1))
BY = int(re.search(r"constexpr int BY = (\d+);", _SRC).group(1))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(sifsr, x, factor, mtf=0.1, hkw=None, crop=False, valid=None, fill_value=float("nan")):
    """-> (out fp32, out_valid uint8) as numpy"""
    out, ov = sifsr.degrade.degrade(dev(x), factor, mtf=mtf, hkw=hkw, crop=crop, valid=dev(valid), fill_value=fill_value,
                                    return_valid=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ov.cpu().numpy()


def against_restatement(sifsr, tag, x, factor, mtf=0.1, hkw=None, crop=False, valid=None):
    out, ov = run(sifsr, x, factor, mtf, hkw, crop, valid, fill_value=-1.0)
    ref, rv = R.degrade_ref(x, factor, mtf, hkw, crop, valid, fill_value=-1.0)
    assert out.shape == ref.shape and out.dtype == np.float32 and ov.dtype == np.uint8
    assert np.array_equal(ov.astype(bool), np.broadcast_to(rv, ov.shape)), f"{tag}: out_valid differs"
    d = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"{tag}: {x.shape} -> {out.shape}, {int(rv.sum())} of {rv.size} outputs valid, max |device - restatement| = {d:.3e} K")
    assert d <= TOL, tag
    return out, ov, ref


def side_for(count, factor, hkw=None):
    """the smallest side whose output has `count` entries"""
    n = R.half_width(factor, hkw) + 1
    while R.out_side(n, factor, hkw) < count:
        n += 1
    assert R.out_side(n, factor, hkw) == count
    return n


# ---- 1. values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c[0])
def test_golden_cases(sifsr, gold, case):
    """the device against the restatement (TOL) and against the reference's recorded output (the host bar + TOL)"""
    name, kind, shape, factor, mtf, hkw, crop, _ = case
    x = R.case_input(name)
    out, ov, _ = against_restatement(sifsr, name, x, factor, mtf, hkw, crop)
    ref = gold[name + "_out"]
    d = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"{name}: max |device - reference| = {d:.3e} K")
    assert out.shape == ref.shape and d <= HOST_BAR + TOL
    if name == "fine_4x3415":                                  # its last output's fp32 coordinate floors one higher than the float64 one
        assert out.shape[-1] == R.FP32_FLOOR_SPLIT + 1


@pytest.mark.parametrize("mtf", [0.1, 0.25])
@pytest.mark.parametrize("shape", [(2, 1, 40, 52), (1, 1, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_consistent_with_the_div4_kernel(sifsr, shape, mtf):
    x = dev(R.make_field(shape, 40 + shape[-1]))
    a = sifsr.degrade.degrade(x, 4, mtf=mtf, crop=True)
    b = sifsr.downscale_LST_SR_to_LR(x, mtf=mtf)
    d = float((a.double() - b.double()).abs().max())
    print(f"{shape} mtf {mtf}: max |degrade(4, crop) - downscale_LST_SR_to_LR| = {d:.3e} K")
    assert a.shape == b.shape == shape[:2] + (shape[2] // 4, shape[3] // 4) and d <= TOL


def seam_cases():
    c, f = R.COARSE, R.FINE
    out = [("coarse strip 12x2048", (12, 2048), c, None), ("coarse strip 2048x12", (2048, 12), c, None),
           ("fine strip 4x2048", (4, 2048), f, None)]
    for d in (-1, 0, 1):
        out.append((f"fine: width BX{d:+d}, height for BY{d:+d} output rows", (side_for(BY + d, f), BX + d), f, None))
        out.append((f"fine: BX{d:+d} output columns, BY{d:+d} + BY output rows", (side_for(2 * BY + d, f), side_for(BX + d, f)), f, None))
        out.append((f"generic: BX{d:+d} output columns", (7, side_for(BX + d, 2.0, 3)), 2.0, 3))
    out.append((f"coarse: width 2 BX + 1, BY + 1 output rows", (side_for(BY + 1, c), 2 * BX + 1), c, None))
    return out


@pytest.mark.parametrize("case", seam_cases(), ids=lambda c: c[0])
def test_shapes_at_the_kernels_seams(sifsr, case):
    tag, shape, factor, hkw = case
    x = R.make_field(shape, 7 + shape[0] + shape[1])
    against_restatement(sifsr, tag, x, factor, 0.1, hkw)
    against_restatement(sifsr, tag + " with a map", x, factor, 0.1, hkw, valid=R.quad_valid(*shape))


@pytest.mark.parametrize("factor", [R.COARSE, R.FINE], ids=["coarse", "fine"])
def test_one_scene(sifsr, factor):
    x = R.make_field((700, 830), 70)
    valid = R.quad_valid(700, 830)
    out, ov, _ = against_restatement(sifsr, "scene", x, factor, valid=valid)
    assert out.shape == ((70, 82) if factor == R.COARSE else (274, 324)) and 0.3 < ov.mean() < 0.6
    fn = sifsr.degrade.aster_to_coarse if factor == R.COARSE else sifsr.degrade.aster_to_fine
    o2, v2 = fn(dev(x), dev(valid))
    assert np.array_equal(bits(o2)[ov == 1], bits(out)[ov == 1]) and np.array_equal(v2.cpu().numpy(), ov) and torch.isnan(o2[v2 == 0]).all()


# ---- 2. validity -------------------------------------------------------------------------------------------------------------------
CONFIGS = [(R.FINE, None, False), (2.0, 3, False), (R.COARSE, None, False), (4.0, None, True), (3.0, None, True)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"f{c[0]:.3g}_hkw{c[1]}_crop{int(c[2])}")
def test_validity_and_invalid_pixel_independence(sifsr, cfg):
    """out_valid is the restatement's exactly; invalid outputs hold fill_value; NaN, 0 or 1e30 in the invalid pixels leave every valid
    output bit-equal"""
    factor, hkw, crop = cfg
    shape = (97, 131) if factor == R.COARSE else (40, 52)
    x, valid = R.make_field(shape, 3), R.quad_valid(*shape)
    out, ov, _ = against_restatement(sifsr, "quadrilateral", x, factor, 0.1, hkw, crop, valid)
    assert 0 < ov.sum() < ov.size
    nan_out, nan_ov = run(sifsr, x, factor, 0.1, hkw, crop, valid)                       # the default fill value
    assert np.array_equal(nan_ov, ov) and np.isnan(nan_out[ov == 0]).all() and np.array_equal(bits(nan_out)[ov == 1], bits(out)[ov == 1])
    for junk in (np.nan, 0.0, 1e30):
        p = x.copy()
        p[valid == 0] = junk
        o2, v2 = run(sifsr, p, factor, 0.1, hkw, crop, valid, fill_value=-1.0)
        assert np.array_equal(v2, ov) and np.array_equal(bits(o2), bits(out)), junk
    # without a map: every value computed, the ring still marked
    free, fv = run(sifsr, x, factor, 0.1, hkw, crop)
    _, rv = R.degrade_ref(x, factor, 0.1, hkw, crop)
    assert np.isfinite(free).all() and np.array_equal(fv.astype(bool), rv) and np.array_equal(bits(free)[ov == 1], bits(out)[ov == 1])
    # a bool map, and one map per image
    o3, v3 = sifsr.degrade.degrade(dev(np.stack([x, x])), factor, hkw=hkw, crop=crop, valid=dev(np.stack([valid, np.ones_like(valid)])).bool(),
                                   fill_value=-1.0, return_valid=True)
    assert np.array_equal(bits(o3[0]), bits(out)) and np.array_equal(v3[1].cpu().numpy(), fv) and np.array_equal(bits(o3[1]), np.where(fv == 1, bits(free), np.float32(-1.0).view(np.uint32)))


def test_batch_independence_and_determinism(sifsr):
    x = R.make_field((5, 61, 83), 9)
    valid = np.stack([np.roll(R.quad_valid(61, 83), 3 * b, axis=1) for b in range(5)])
    for factor in (R.FINE, R.COARSE):
        a = sifsr.degrade.degrade(dev(x), factor, valid=dev(valid), return_valid=True)
        b = sifsr.degrade.degrade(dev(x), factor, valid=dev(valid), return_valid=True)
        assert bit_equal(a[0], b[0]) and bit_equal(a[1], b[1])
        for i in range(5):
            one = sifsr.degrade.degrade(dev(x[i]), factor, valid=dev(valid[i]), return_valid=True)
            assert bit_equal(one[0], a[0][i]) and bit_equal(one[1], a[1][i]), i
        four = sifsr.degrade.degrade(dev(x)[:, None], factor)                             # (B,C,H,W), and the shared (H,W) map
        assert four.shape[:2] == (5, 1) and bit_equal(four[:, 0], sifsr.degrade.degrade(dev(x), factor))
        shared = sifsr.degrade.degrade(dev(x), factor, valid=dev(valid[0]))
        assert bit_equal(shared[0], a[0][0])


def test_simulate_pair_and_generic(sifsr):
    x, valid = R.make_field((97, 131), 13), R.quad_valid(97, 131)
    coarse, fine, cv, fv = sifsr.simulate_pair(dev(x), dev(valid))
    c2, cv2 = sifsr.aster_to_coarse(dev(x), dev(valid))
    f2, fv2 = sifsr.aster_to_fine(dev(x), dev(valid))
    assert bit_equal(coarse, c2) and bit_equal(fine, f2) and bit_equal(cv, cv2) and bit_equal(fv, fv2)
    assert tuple(coarse.shape) == (11, 14) and tuple(fine.shape) == (40, 53) and fv.sum() > 0
    plain = sifsr.aster_to_fine(dev(x))
    assert isinstance(plain, torch.Tensor) and bit_equal(plain[fv == 1], fine[fv == 1])
    g = sifsr.generic_downscale(dev(x)[None, None])
    assert tuple(g.shape) == (1, 1, 51, 68) and bit_equal(g, sifsr.degrade.degrade(dev(x)[None, None], 2.0, hkw=3))


# ---- 3. the C entry point: memory contract, graph capture, errors -------------------------------------------------------------------
# (B, h, w, factor, hkw, crop, with valid, with out_valid)
CONTRACT_SHAPES = [(1, 12, 12, R.COARSE, 0, False, False, False), (2, 40, 52, 2.0, 3, False, True, True), (3, 61, 83, R.FINE, 0, False, True, False),
                   (1, 40, 130, 4.0, 0, True, False, True), (2, 33, 70, 3.0, 0, True, True, True)]


def contract_inputs(i):
    B, h, w, factor, hkw, crop, with_valid, _ = CONTRACT_SHAPES[i]
    x = R.make_field((B, h, w), 600 + i)
    valid = None
    if with_valid:
        valid = np.stack([np.roll(R.quad_valid(h, w), b, axis=0) for b in range(B)])
        x[valid == 0] = np.nan
    return x, valid


def degrade_case(i):
    def make(k):
        B, h, w, factor, hkw, crop, with_valid, with_ov = CONTRACT_SHAPES[i]
        x_np, valid_np = contract_inputs(i)
        x = k.t("x", torch.from_numpy(x_np))
        valid = k.t("valid", torch.from_numpy(valid_np)) if with_valid else None
        oh, ow = R.out_side(h, factor, hkw or None, crop), R.out_side(w, factor, hkw or None, crop)
        out = k.o("out", B, oh, ow)
        ov = k.o("out_valid", B, oh, ow, dtype=torch.uint8) if with_ov else None
        need = k.L.call("sifsrs_workspace_bytes", B, h, w, factor, hkw, int(crop))
        ws = k.A.scratch(need, "workspace")                       # poisoned scratch: nothing of it may reach the outputs
        call = lambda: k.L.call("sifsrs_degrade", x, valid, out, ov, ws, need, B, h, w, factor, 0.1, hkw, int(crop), -1.0, S())
        outs = {"out": out}
        if ov is not None:
            outs["out_valid"] = ov
        return call, outs
    return make


CONTRACT = {"sifsrs_degrade": [degrade_case(i) for i in range(len(CONTRACT_SHAPES))]}


@pytest.mark.parametrize("idx", range(len(CONTRACT_SHAPES)))
def test_memory_contract(L, idx):
    """out and out_valid written in full and nowhere else -- bit-identical and NaN-free under every poison of the outputs and of the
    workspace (no workspace byte is read before it is written; the NaNs of the invalid input pixels reach no output) --, x and valid
    untouched, nothing outside the buffers and the stated workspace bytes written, the same bits on ordinary allocations, and the
    result is the restatement's."""
    first = run_contract(L, CONTRACT["sifsrs_degrade"][idx], seed=431 + idx, capacity=64 << 20)
    B, h, w, factor, hkw, crop, with_valid, with_ov = CONTRACT_SHAPES[idx]
    x, valid = contract_inputs(idx)
    got = first["out"].cpu().numpy()
    for b in range(B):
        ref, rv = R.degrade_ref(np.nan_to_num(x[b]), factor, 0.1, hkw or None, crop, None if valid is None else valid[b], fill_value=-1.0)
        assert np.abs(got[b] - ref).max() <= TOL
        if with_ov:
            assert np.array_equal(first["out_valid"][b].cpu().numpy().astype(bool), rv)


def test_graph_capture(sifsr, L):
    """one captured call, replayed twice, gives the eager bits: the entry point only enqueues"""
    B, h, w, factor = 2, 61, 83, R.FINE
    x, valid = dev(R.make_field((B, h, w), 77)), dev(np.stack([R.quad_valid(h, w)] * B))
    oh, ow = sifsr.degrade.output_shape(h, w, factor)
    need = L.call("sifsrs_workspace_bytes", B, h, w, factor, 0, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    mk = lambda: (torch.full((B, oh, ow), 7.0, device="cuda"), torch.full((B, oh, ow), 7, dtype=torch.uint8, device="cuda"))
    eager, eager_v = mk()
    out, ov = mk()
    launch = lambda o, v: L.call("sifsrs_degrade", x, valid, o, v, ws, need, B, h, w, factor, 0.1, 0, 0, float("nan"), S())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch(eager, eager_v)                                                          # also the warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(out, ov)
    for _ in range(2):
        ws.fill_(0xFF)
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert bit_equal(out, eager) and bit_equal(ov, eager_v)
    want, wv = sifsr.degrade.degrade(x, factor, valid=valid, return_valid=True)
    assert bit_equal(want, eager) and bit_equal(wv, eager_v)


def test_dropin(sifsr, gold):
    from dropin import utils as us
    for name, fn in (("coarse_97x131", us.downscale_Aster_to_coarse), ("coarse_12x40", us.downscale_Aster_to_coarse),
                     ("fine_61x83", us.downscale_Aster_to_fine), ("fine_4x4", us.downscale_Aster_to_fine)):
        got = fn(R.case_input(name))
        ref = gold[name + "_out"]
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == ref.shape
        assert np.abs(got.astype(np.float64) - ref).max() <= HOST_BAR + TOL
    assert us.downscale_Aster_to_fine(R.case_input("fine_61x83").astype(np.float64)).dtype == np.float32
    for name in ("generic_2x3x40x52", "generic_4x4"):
        got = us.generic_downscale(dev(R.case_input(name)))
        ref = gold[name + "_out"]
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape
        assert np.abs(got.cpu().numpy().astype(np.float64) - ref).max() <= HOST_BAR + TOL


def test_errors_launch_nothing(sifsr, L):
    D = sifsr.degrade
    x = dev(R.make_field((40, 52), 1))
    E = sifsr.SifsrError
    for bad in (lambda: D.degrade(x.cpu(), 2.0), lambda: D.degrade(x[:11].contiguous(), R.COARSE), lambda: D.degrade(x[:, :3].contiguous(), R.FINE),
                lambda: D.degrade(x, 1.0), lambda: D.degrade(x, 0.5), lambda: D.degrade(x, 16.5), lambda: D.degrade(x, 2.0, hkw=17),
                lambda: D.degrade(x, 2.0, hkw=0), lambda: D.degrade(x, 2.0, mtf=1.0), lambda: D.degrade(x, 2.0, mtf=0.0),
                lambda: D.degrade(x.double(), 2.0), lambda: D.degrade(x[:, ::2], 2.0), lambda: D.degrade(x[None, None, None], 2.0),
                lambda: D.degrade(x, 2.0, valid=torch.ones(40, 52, device="cuda")), lambda: D.degrade(x, 2.0, valid=torch.ones(40, 51, dtype=torch.uint8, device="cuda")),
                lambda: D.degrade(x, 2.0, valid=torch.ones(40, 52, dtype=torch.uint8)), lambda: D.degrade(x[:4, :9].contiguous(), 15.0, hkw=3)):
        with pytest.raises(E):
            bad()
    with pytest.raises(NotImplementedError):
        D.degrade(x.clone().requires_grad_(), 2.0)
    with pytest.raises(NotImplementedError):                                              # the /4 operator keeps its refusal
        sifsr.get_output_ftm(x[None, None], factor=2)
    # the C entry point: every error returns before a launch
    h, w, B = 40, 52, 2
    fn, need = L.lib().sifsrs_degrade, L.lib().sifsrs_workspace_bytes(B, h, w, 2.0, 3, 0)
    xs, out = torch.full((B, h, w), 77.0, device="cuda"), torch.full((B, 23, 29), 77.0, device="cuda")
    valid, ov = torch.full((B, h, w), 77, dtype=torch.uint8, device="cuda"), torch.full((B, 23, 29), 77, dtype=torch.uint8, device="cuda")
    ws = torch.full((need + 16,), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    args = lambda **kw: [kw.get("x", p(xs)), kw.get("valid", p(valid)), kw.get("out", p(out)), kw.get("ov", p(ov)), kw.get("ws", p(ws)),
                         kw.get("nbytes", need), kw.get("B", B), kw.get("h", h), kw.get("w", w), kw.get("factor", 2.0), kw.get("mtf", 0.1),
                         kw.get("hkw", 3), kw.get("crop", 0), -1.0, S()]
    for bad in (dict(h=3), dict(w=3), dict(h=16385), dict(factor=1.0), dict(factor=16.5), dict(hkw=17), dict(hkw=-1), dict(mtf=0.0),
                dict(mtf=1.0), dict(B=0), dict(B=65536), dict(crop=2)):
        assert fn(*args(**bad)) == 1001, bad
    for bad in (dict(x=None), dict(out=None), dict(ws=None), dict(ws=p(ws) + 8), dict(x=p(xs) + 2), dict(out=p(out) + 1)):
        assert fn(*args(**bad)) == 1002, bad
    for bad in (dict(nbytes=need - 1), dict(nbytes=0)):
        assert fn(*args(**bad)) == 1003, bad
    torch.cuda.synchronize()
    for t in (xs, out, valid, ov, ws):
        assert (t == 77).all()
    assert fn(*args(valid=None, ov=None)) == 0
    torch.cuda.synchronize()
    assert (xs == 77).all() and (ov == 77).all() and (ws[need:] == 77).all()
    assert (out[:, 4:-4, 4:-4] == 77).all() and (out[:, 0] < 77).all()          # a constant stays one; the ring is darker
