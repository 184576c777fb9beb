"""GPU: LPIPS-VGG16 on the device (include/sifsr_lpips.h) against tests/lpips_reference.py.

  * values: each of the six columns (five layer terms and the sum) of both entry points against the float64 restatement at 1e-4
    relative (the project's fp32 parity bar; CPU fp32 torch is at 1e-9 .. 4e-6 per column), at the shapes of R.VALUE_SHAPES -- a
    1 x 1 relu5_3, odd sizes with floor pooling at every level, several tiles, a feature map exactly at the direct / MFMA
    threshold (16 x 16) and one a pixel beyond it (15 x 17), and (1,128,128) / (1,256,256), where the 256- and 512-channel layers
    run on the MFMA kernel in slices of 128 output channels (at the smaller shapes they are all direct) -- and on the golden crops;
  * bit-exactness: identical images -> 0.0, x / y swap, row i of N = 3 against its N = 1 call, the pairs call against the
    three-channel call on hand-normalised repeated channels (which holds the on-device min / max to the restatement's), a
    constant pair -> NaN, one NaN pixel -> that row NaN and the others untouched;
  * the memory contract of the three writing entry points in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is
    the list tests/test_capi_gate.py gates), error codes with `out6` untouched, one linear hipGraph capture;
  * the Python interface: both key forms, the reductions, lists of mixed sizes, the nine-column table."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lpips_reference as R
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal

pytestmark = pytest.mark.gpu
F64, U8 = torch.float64, torch.uint8
TOL = 1e-4
ZERO3, ONE3 = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]


@pytest.fixture(scope="module")
def packed(L):
    vgg, lin = torch.from_numpy(R.vgg_flat()).cuda(), torch.from_numpy(R.lin_flat()).cuda()
    out = torch.empty(L.call("sifsrl_pack_floats"), device="cuda")
    L.call("sifsrl_pack", vgg, lin, out, S())
    torch.cuda.synchronize()
    return out


def c3(v):
    return (ctypes.c_float * 3)(*v)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def lpips3(L, packed, x, y, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD):
    """(N,3,H,W) numpy x2 -> (N,6) float64 device tensor through the C ABI"""
    N, _, H, W = x.shape
    need = L.call("sifsrl_workspace_bytes", N, H, W)
    ws = torch.empty(need, dtype=U8, device="cuda")
    out = torch.empty(N, 6, dtype=F64, device="cuda")
    L.call("sifsrl_lpips", dev(x), dev(y), N, H, W, c3(mean), c3(std), packed, ws, need, out, S())
    return out


def lpips1(L, packed, a, b):
    N, H, W = a.shape
    need = L.call("sifsrl_workspace_bytes", N, H, W)
    ws = torch.empty(need, dtype=U8, device="cuda")
    out = torch.empty(N, 6, dtype=F64, device="cuda")
    L.call("sifsrl_lpips_pairs", dev(a), dev(b), N, H, W, packed, ws, need, out, S())
    return out


def check_rows(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    rel = np.abs(got - want) / np.abs(want)
    for i in range(len(want)):
        print(f"{what} row {i} relative deviations:", " ".join(f"{n}={r:.2e}" for n, r in zip(("d1", "d2", "d3", "d4", "d5", "sum"), rel[i])))
    assert (want[:, :5] >= R.FLOOR).all()
    assert (rel <= TOL).all(), (what, rel)


# ---- 1. values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.VALUE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_values_against_the_restatement(L, packed, shape):
    (x, y, want3), (a, b, want1) = R.value_case(shape)
    check_rows(lpips3(L, packed, x, y), want3, f"lpips {shape}")
    check_rows(lpips1(L, packed, a, b), want1, f"pairs {shape}")


def test_golden_cases(L, packed):
    gold = np.load(R.GOLDEN)
    assert str(gold["weights_sha256"]) == R.WEIGHTS_SHA256
    for i, kind in enumerate(gold["kinds"]):
        a, b = gold[f"a{i}"][None], gold[f"b{i}"][None]
        x, y, _, _ = R.normalise_pair(a, b)
        got1, got3 = lpips1(L, packed, a, b), lpips3(L, packed, x, y)
        if kind == "same":
            assert (got1 == 0).all() and (got3 == 0).all()
            continue
        check_rows(got1, gold[f"terms_pairs{i}"][None], f"golden pairs {i}")
        check_rows(got3, gold[f"terms_imagenet{i}"][None], f"golden imagenet {i}")


# ---- 2. bit-exactness ------------------------------------------------------------------------------------------------------------
def test_bit_exactness(L, packed):
    x, y = R.images(3, 24, 40, seed=7)
    a, b = R.rasters(3, 24, 40, seed=7)
    full3, full1 = lpips3(L, packed, x, y), lpips1(L, packed, a, b)
    assert torch.isfinite(full3).all() and (full3 > 0).all() and (full1 > 0).all()
    assert (lpips3(L, packed, x, x) == 0).all() and (lpips1(L, packed, b, b.copy()) == 0).all()          # exactly 0.0, six columns
    assert bit_equal(lpips3(L, packed, y, x), full3) and bit_equal(lpips1(L, packed, b, a), full1)        # the swap
    for i in range(3):
        assert bit_equal(lpips3(L, packed, x[i:i + 1], y[i:i + 1])[0], full3[i]), i
        assert bit_equal(lpips1(L, packed, a[i:i + 1], b[i:i + 1])[0], full1[i]), i
    # the table path is the three-channel call on hand-normalised repeated channels: holds the on-device min / max to the restatement's
    tx, ty, mini, maxi = R.normalise_pair(a, b)
    assert (maxi > mini).all()
    assert bit_equal(lpips3(L, packed, tx, ty, ZERO3, ONE3), full1)
    # a constant pair: the reference divides by zero -> NaN row, the others as they were
    a2, b2 = a.copy(), b.copy()
    a2[1], b2[1] = 300.0, 300.0
    got = lpips1(L, packed, a2, b2)
    assert torch.isnan(got[1]).all() and bit_equal(got[0], full1[0]) and bit_equal(got[2], full1[2])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_one_non_finite_pixel(L, packed, bad):
    x, y = R.images(3, 24, 40, seed=7)
    a, b = R.rasters(3, 24, 40, seed=7)
    full3, full1 = lpips3(L, packed, x, y), lpips1(L, packed, a, b)
    x2, b2 = x.copy(), b.copy()
    x2[1, 2, 13, 29], b2[1, 5, 7] = bad, bad
    got3, got1 = lpips3(L, packed, x2, y), lpips1(L, packed, a, b2)
    for got, full in ((got3, full3), (got1, full1)):
        assert torch.isnan(got[1]).all()
        assert bit_equal(got[0], full[0]) and bit_equal(got[2], full[2])


# ---- 3. memory contract ----------------------------------------------------------------------------------------------------------
_PACKED_CPU = {}


def packed_cpu(L):
    if "p" not in _PACKED_CPU:
        out = torch.empty(L.call("sifsrl_pack_floats"), device="cuda")
        L.call("sifsrl_pack", torch.from_numpy(R.vgg_flat()).cuda(), torch.from_numpy(R.lin_flat()).cuda(), out, S())
        torch.cuda.synchronize()
        _PACKED_CPU["p"] = out.cpu()
    return _PACKED_CPU["p"]


def pack_case(scale):
    def make(k):
        vgg = k.A.input(torch.from_numpy(R.vgg_flat()) * scale, "vgg_params")
        lin = k.A.input(torch.from_numpy(R.lin_flat()) * scale, "lin")
        out = k.A.output(k.L.call("sifsrl_pack_floats"), torch.float32, "packed")
        return (lambda: k.L.call("sifsrl_pack", vgg, lin, out, S())), {"packed": out}
    return make


def lpips_case(shape, pairs):
    def make(k):
        N, H, W = shape
        if pairs:
            a, b = R.rasters(N, H, W, seed=k.seed % 97)
            x, y = k.A.input(torch.from_numpy(a), "a"), k.A.input(torch.from_numpy(b), "b")
        else:
            xi, yi = R.images(N, H, W, seed=k.seed % 97)
            x, y = k.A.input(torch.from_numpy(xi), "x"), k.A.input(torch.from_numpy(yi), "y")
        pk = k.A.input(packed_cpu(k.L), "packed")
        need = k.L.call("sifsrl_workspace_bytes", N, H, W)
        ws = k.A.scratch(need, "workspace")                       # poisoned: nothing of it may reach the outputs
        out = k.A.output((N, 6), F64, "out6")
        if pairs:
            call = lambda: k.L.call("sifsrl_lpips_pairs", x, y, N, H, W, pk, ws, need, out, S())
        else:
            call = lambda: k.L.call("sifsrl_lpips", x, y, N, H, W, c3(R.IMAGENET_MEAN), c3(R.IMAGENET_STD), pk, ws, need, out, S())
        return call, {"out6": out}
    return make


# (1,64,64): conv3 (256 channels, two slices of 128) on the MFMA kernel; (1,128,128): conv4 too (512 channels, four slices) -- a slice
# placed outside the raw tensor hits a guard, a slice left unwritten leaves poison in the result
CONTRACT_SHAPES = ((1, 16, 16), (2, 17, 31), (1, 32, 32), (1, 30, 34), (1, 64, 64), (1, 128, 128))
CONTRACT = {"sifsrl_pack": [pack_case(s) for s in (1.0, 0.5, -2.0)],
            "sifsrl_lpips": [lpips_case(s, False) for s in CONTRACT_SHAPES],
            "sifsrl_lpips_pairs": [lpips_case(s, True) for s in CONTRACT_SHAPES]}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output written in full and nowhere else -- NaN-free under the NaN poison, bit-identical under every poison (the
    poisoned workspace included: nothing is left over from an earlier call) --, const inputs untouched, and the same bits on
    ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=160 << 20)


def test_error_codes_leave_out6_untouched(L, packed):
    a, b = R.rasters(2, 24, 40, seed=3)
    x, y = R.images(2, 24, 40, seed=3)
    A, B, X, Y = dev(a), dev(b), dev(x), dev(y)
    need = L.call("sifsrl_workspace_bytes", 2, 24, 40)
    ws = torch.full((need,), 77, dtype=U8, device="cuda")
    out = torch.full((2, 6), 77.0, dtype=F64, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    m, s = c3(R.IMAGENET_MEAN), c3(R.IMAGENET_STD)
    f3, f1 = L.lib().sifsrl_lpips, L.lib().sifsrl_lpips_pairs
    a3 = lambda **kw: (p(kw.get("x", X)), p(kw.get("y", Y)), kw.get("N", 2), kw.get("H", 24), kw.get("W", 40), kw.get("mean", m), kw.get("std", s),
                       p(kw.get("packed", packed)), p(kw.get("ws", ws)), kw.get("nbytes", need), p(kw.get("out", out)), S())
    a1 = lambda **kw: (p(kw.get("a", A)), p(kw.get("b", B)), kw.get("N", 2), kw.get("H", 24), kw.get("W", 40), p(kw.get("packed", packed)),
                       p(kw.get("ws", ws)), kw.get("nbytes", need), p(kw.get("out", out)), S())
    for bad in (dict(H=15), dict(W=15), dict(N=0)):
        assert f3(*a3(**bad)) == 1001 and f1(*a1(**bad)) == 1001
    for bad in (dict(x=None), dict(y=None), dict(mean=None), dict(std=None), dict(packed=None), dict(ws=None), dict(out=None)):
        assert f3(*a3(**bad)) == 1002, bad
    for bad in (dict(a=None), dict(b=None), dict(packed=None), dict(ws=None), dict(out=None)):
        assert f1(*a1(**bad)) == 1002, bad
    assert f3(*a3(nbytes=need - 1)) == 1003 and f1(*a1(nbytes=need - 1)) == 1003 and f1(*a1(nbytes=0)) == 1003
    assert L.lib().sifsrl_pack(None, p(packed), p(packed), S()) == 1002
    torch.cuda.synchronize()
    assert (out == 77).all() and (ws == 77).all()
    assert f1(*a1()) == 0
    torch.cuda.synchronize()
    assert not (out == 77).any()


def test_graph_capture_of_the_table_path(L, packed):
    (_, _, _), (a, b, want) = R.value_case((2, 48, 80))
    A, B = dev(a), dev(b)
    need = L.call("sifsrl_workspace_bytes", 2, 48, 80)
    ws = torch.empty(need, dtype=U8, device="cuda")
    eager, out = torch.empty(2, 6, dtype=F64, device="cuda"), torch.zeros(2, 6, dtype=F64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        L.call("sifsrl_lpips_pairs", A, B, 2, 48, 80, packed, ws, need, eager, S())      # warm up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.call("sifsrl_lpips_pairs", A, B, 2, 48, 80, packed, ws, need, out, S())         # one linear chain of launches
    ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert bit_equal(out, eager)
    check_rows(out, want, "graph replay")


# ---- 4. the Python interface -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(sifsr):
    sd, lin = R.state_dicts("features.")
    return sifsr.lpips.LPIPS(sd, lin)


def test_python_interface(sifsr, L, packed, model):
    x, y = R.images(3, 24, 40, seed=7)
    X, Y = dev(x), dev(y)
    rows = model.layers(X, Y)
    assert rows.dtype == F64 and rows.is_cuda and tuple(rows.shape) == (3, 6)
    assert bit_equal(rows, lpips3(L, packed, x, y))
    sd2, lin2 = R.state_dicts("")                                                  # the `features` module's own keys
    other = sifsr.lpips.LPIPS(sd2, torch.cat([v.reshape(-1) for v in lin2]), reduction="none")
    assert bit_equal(other.layers(X, Y), rows) and bit_equal(other(X, Y), rows[:, 5])
    assert bit_equal(model(X, Y), rows[:, 5].mean(dim=0))
    assert bit_equal(sifsr.lpips.LPIPS(sd2, lin2, reduction="sum")(X, Y), rows[:, 5].sum(dim=0))
    # lists of mixed sizes equal the per-item calls
    x2, y2 = R.images(2, 17, 31, seed=9)
    X2, Y2 = dev(x2), dev(y2)
    small = model.layers(X2, Y2)
    mixed = model.layers([X[0], X2[1], X[2][None], X2[0]], [Y[0], Y2[1], Y[2][None], Y2[0]])
    for k, (src, i) in enumerate(((rows, 0), (small, 1), (rows, 2), (small, 0))):
        assert bit_equal(mixed[k], src[i]), k
    # chunked batches give the same rows
    keep = sifsr.lpips.WORKSPACE_CAP
    try:
        sifsr.lpips.WORKSPACE_CAP = 3 * 2 * 24 * 40 * 256 * 2                          # two pairs per call
        assert sifsr.lpips.max_pairs(24, 40) == 2 and bit_equal(model.layers(X, Y), rows)
    finally:
        sifsr.lpips.WORKSPACE_CAP = keep
    # the table
    a, b = R.rasters(3, 24, 40, seed=7)
    A, B = dev(a)[:, None], dev(b)[:, None]
    table = sifsr.metrics.aster_table(A, B, model)
    eight = sifsr.metrics.aster_metrics(A, B)
    assert sifsr.metrics.METRIC_NAMES_WITH_LPIPS == ("PSNR", "SSIM", "RMSE", "RMSE (low grad per image)", "RMSE (mean grad per image)",
                                                     "RMSE (high grad per image)", "GSSIM", "LPIPS", "RMSE_grad")
    assert tuple(table.shape) == (3, 9) and table.dtype == F64
    assert bit_equal(table[:, [0, 1, 2, 3, 4, 5, 6, 8]].contiguous(), eight)
    assert bit_equal(table[:, 7].contiguous(), lpips1(L, packed, a, b)[:, 5].contiguous())
    assert bit_equal(model.pairs(A, B), model.pairs(A[:, 0], B[:, 0]))
    tl = sifsr.metrics.aster_table([A[0, 0], A[1]], [B[0, 0], B[1]], model)
    assert bit_equal(tl, table[:2])
    with pytest.raises(sifsr.SifsrError):
        model.layers(X[:, :, :15], Y[:, :, :15])
    with pytest.raises(sifsr.SifsrError):
        model.layers(X.cpu(), Y.cpu())


def test_the_drop_in_binds(sifsr, L, packed, tmp_path, monkeypatch):
    import importlib.util
    import os
    sd, lin = R.state_dicts("features.")
    torch.save(sd, tmp_path / "vgg16.pth"); torch.save(lin, tmp_path / "lpips_weights.pt")
    monkeypatch.setenv("SIFSR_VGG16_WEIGHTS", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("SIFSR_LPIPS_WEIGHTS", str(tmp_path / "lpips_weights.pt"))
    spec = importlib.util.spec_from_file_location("dropin_lpips", os.path.join(R.ROOT, "dropin", "lpips.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lpips_loss = mod.LPIPS(distance='mse', reduction='mean', mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0])      # model_perf_aster_formatds.py:134
    a, b = R.rasters(1, 24, 40, seed=7)
    t1, t2, _, _ = R.normalise_pair(a, b)
    val = lpips_loss(torch.tensor(t1), torch.tensor(t2)).numpy()                                             # :407-410
    want = lpips1(L, packed, a, b)[0, 5]
    assert val.dtype == np.float32 and val.shape == () and val == np.float32(float(want))
