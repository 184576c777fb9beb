"""GPU: the per-pair ASTER evaluation table (model_perf_aster_formatds.py:371-437) of
sifsr.metrics.aster_metrics / gradient_strata against the golden numbers of tests/golden/make_golden_eval.py (real ASTER
crops; GSSIM and get_output_ftm pinned to the reference by import, PSNR / SSIM / strata restated -- unpinned vs
scikit-image), numpy's percentile on the returned g map, batch / graph invariance and the us.gssim drop-in."""
import os

import numpy as np
import pytest
import torch

from tests import eval_reference as E

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_eval_v1.npz")
REL = [0, 2, 3, 4, 5, 6, 7]          # columns held to 1e-5 relative


@pytest.fixture(scope="module")
def sifsr():
    import sifsr as pkg
    assert torch.cuda.is_available()
    return pkg


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def check_row(got, want, kind):
    for c in REL:
        if np.isinf(want[c]):
            assert got[c] == want[c], (c, got[c], want[c])
        else:
            assert abs(got[c] - want[c]) <= 1e-5 * abs(want[c]) + 1e-12, (E.METRIC_NAMES[c], got[c], want[c])
    tol = 1e-4 if kind == "z" else 2e-3     # float32 cancellation of uxx - ux*ux at Kelvin scale, in skimage as here
    assert abs(got[1] - want[1]) <= tol * abs(want[1]), ("SSIM", got[1], want[1])


def test_golden_columns(sifsr, gold):
    assert sifsr.metrics.METRIC_NAMES == tuple(gold["names"])
    for i, kind in enumerate(gold["kinds"]):
        a, b = gold[f"a{i}"], gold[f"b{i}"]
        got = sifsr.metrics.aster_metrics(dev(a)[None, None], dev(b)[None, None])
        assert got.shape == (1, 8) and got.dtype == torch.float64 and got.is_cuda
        row = got[0].cpu().numpy()
        check_row(row, gold[f"metrics{i}"], kind)
        g, q25, q75, counts = sifsr.metrics.gradient_strata(dev(a)[None, None])
        assert float(q25[0]) == gold[f"q{i}"][0] and float(q75[0]) == gold[f"q{i}"][1]
        assert tuple(counts[0].cpu().tolist()) == tuple(gold[f"counts{i}"])
        if kind == "same":
            assert row[0] == np.inf and row[1] == 1.0 and row[2] == row[3] == row[4] == row[5] == row[7] == 0.0


def _percentile_case(sifsr, a):
    g, q25, q75, counts = sifsr.metrics.gradient_strata(dev(a)[None, None])
    gn = g[0, 0].cpu().numpy()
    np.testing.assert_array_equal(gn, E.gradient_map(a))      # the get_output_ftm kernel's arithmetic, restated
    p25, p75 = np.percentile(gn.flatten(), 25), np.percentile(gn.flatten(), 75)
    assert np.float32(q25[0].item()).tobytes() == np.float32(p25).tobytes(), (q25.item(), p25)
    assert np.float32(q75[0].item()).tobytes() == np.float32(p75).tobytes(), (q75.item(), p75)
    want = ((gn < p25).sum(), ((gn >= p25) & (gn <= p75)).sum(), (gn >= p75).sum())
    assert tuple(counts[0].cpu().tolist()) == tuple(int(v) for v in want)


def test_quantiles_are_numpys(sifsr, gold):
    _percentile_case(sifsr, gold["a0"])                                      # real crop, ties in g
    _percentile_case(sifsr, np.full((20, 24), 301.25, np.float32))           # constant image
    rs = np.random.RandomState(5)
    _percentile_case(sifsr, (rs.standard_normal((17, 17)) * 3 + 300).astype(np.float32))   # 0.25 (N-1) = 72, integral
    _percentile_case(sifsr, (rs.standard_normal((16, 20)) * 3 + 300).astype(np.float32))   # 0.25 (N-1) = 79.75
    _percentile_case(sifsr, np.round(rs.standard_normal((64, 48)) * 4).astype(np.float32) + 300)   # heavy ties


def _pair(rs, H, W):
    a = (rs.standard_normal((H, W)).cumsum(0).cumsum(1) * 0.05 + 300).astype(np.float32)
    b = (a + 0.4 * rs.standard_normal((H, W)) + 0.2).astype(np.float32)
    return a, b


def test_shapes_and_batches(sifsr):
    rs = np.random.RandomState(7)
    for H, W in ((41, 57), (335, 374)):
        a, b = _pair(rs, H, W)
        row = sifsr.metrics.aster_metrics(dev(a)[None, None], dev(b)[None, None])[0].cpu().numpy()
        check_row(row, E.metrics(a, b)[0], "k")
    B = 64
    pairs = [_pair(rs, 256, 256) for _ in range(B)]
    A = dev(np.stack([p[0] for p in pairs]))[:, None]
    Bt = dev(np.stack([p[1] for p in pairs]))[:, None]
    batch = sifsr.metrics.aster_metrics(A, Bt)
    for i in range(B):
        one = sifsr.metrics.aster_metrics(A[i:i + 1], Bt[i:i + 1])
        assert torch.equal(batch[i], one[0]), i
    check_row(batch[3].cpu().numpy(), E.metrics(*pairs[3])[0], "k")
    # list form: mixed sizes grouped by shape, rows in list order
    a1, b1 = _pair(rs, 41, 57)
    rows = sifsr.metrics.aster_metrics([A[0, 0], dev(a1), A[1]], [Bt[0, 0], dev(b1), Bt[1]])
    assert torch.equal(rows[0], batch[0]) and torch.equal(rows[2], batch[1])
    assert torch.equal(rows[1], sifsr.metrics.aster_metrics(dev(a1)[None, None], dev(b1)[None, None])[0])


def test_determinism_and_graph(sifsr):
    rs = np.random.RandomState(11)
    pairs = [_pair(rs, 96, 80) for _ in range(4)]
    A = dev(np.stack([p[0] for p in pairs]))[:, None]
    Bt = dev(np.stack([p[1] for p in pairs]))[:, None]
    r1, r2 = sifsr.metrics.aster_metrics(A, Bt), sifsr.metrics.aster_metrics(A, Bt)
    assert torch.equal(r1, r2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sifsr.metrics.aster_metrics(A, Bt)                   # warm up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sifsr.metrics.aster_metrics(A, Bt)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, r1)


def test_dropin_gssim(sifsr, gold):
    from dropin import utils as us
    a, b = gold["a0"], gold["b0"]
    R = np.max([a, b]) - np.min([a, b])
    col = sifsr.metrics.aster_metrics(dev(a)[None, None], dev(b)[None, None])[0, 6].item()
    assert us.gssim(a, b, data_range=R) == col
    assert us.gssim(a, b, data_range=R, grad_comp_type=2) == col
    assert abs(us.gssim(a, b, data_range=R) - gold["metrics0"][6]) <= 1e-5 * abs(gold["metrics0"][6])
    with pytest.raises(TypeError):
        us.gssim(a, b)                                         # data_range=None fails in the reference too
    with pytest.raises(NotImplementedError):
        us.gssim(a, b, win_size=5, data_range=R)
    with pytest.raises(ValueError):
        us.gssim(a, b[:, :-1], data_range=R)                   # shapes differ
    with pytest.raises(sifsr.SifsrError):
        us.gssim(a[:12, :12], b[:12, :12], data_range=R)       # smaller than 16 x 16
    with pytest.raises(sifsr.SifsrError):
        us.gssim(torch.from_numpy(a), torch.from_numpy(b), data_range=R)   # CPU tensors
    with pytest.raises(sifsr.SifsrError):
        sifsr.metrics.aster_metrics(torch.from_numpy(a)[None, None], torch.from_numpy(b)[None, None])
    with pytest.raises(sifsr.SifsrError):
        sifsr.metrics.gradient_strata(torch.zeros(1, 1, 15, 40))
