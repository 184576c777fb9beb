"""GPU: scoring rasters with gaps (include/sifsr_scores.h) against the restatement tests/scores_reference.py
(held to tests/eval_reference.py and the oracle by tests/test_scores_host.py) and against the unmasked entry points.

  * per-pair table: blob masks (30 % invalid) at (41, 57) and (96, 80) within the tolerances of tests/test_eval_metrics_gpu.py,
    counts exact, the quartiles numpy's bytes on the returned eligible g; every pixel valid = aster_metrics bit for bit; NaN / 0
    in the images = the explicit mask; what an invalid pixel holds changes no bit; the edge counts (nothing valid, one 9 x 9
    block, a block in the corner); lists, determinism, one hipGraph capture,
  * the memory contract of the two writing entry points in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is the
    table tests/test_capi_gate.py checks against the header),
  * train-time pair: B = 2 at (40, 24), (64, 64), (100, 36), both scales, three masks, within the f1 tolerances of
    tests/test_pipeline_gpu.py::test_psnr_ssim; every byte valid = psnr_ssim bit for bit; nothing valid = NaN,
  * the epoch keyword."""
import numpy as np
import pytest
import torch

from tests import eval_reference as E
from tests import scores_reference as R
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal
from tests.test_eval_metrics_gpu import check_row

pytestmark = pytest.mark.gpu
U8, I32, F64 = torch.uint8, torch.int32, torch.float64
WORKSPACE_ERR = 1003
G_OUT = 0xFFFFFFFF


def dev(x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.astype(np.float32) if x.dtype.kind == "f" else x).cuda()


def rows_of(sifsr, a, b, m=None, **kw):
    """(B,H,W) numpy images and mask -> (rows (B,8) float64, counts (B,5)) as numpy"""
    out, cnt = sifsr.metrics.masked_aster_metrics(dev(a)[:, None], dev(b)[:, None], None if m is None else dev(m), return_counts=True, **kw)
    assert out.dtype == F64 and cnt.dtype == I32 and out.is_cuda and tuple(out.shape) == (len(a), 8) and tuple(cnt.shape) == (len(a), 5)
    return out.cpu().numpy(), cnt.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_masked_row(got, want, kind, what=""):
    """check_row of tests/test_eval_metrics_gpu.py (1e-5 on columns 0, 2-7; SSIM 2e-3 at Kelvin scale, 1e-4 z-scored), each
    figure printed first"""
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{what} relative deviations:", " ".join(f"{n.split()[0]}={abs(g - w) / abs(w):.2e}" for n, g, w in zip(E.METRIC_NAMES, got, want)))
    check_row(got, want, kind)


# ---- 1. blobs against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.BLOB_SHAPES)
def test_blobs_against_the_restatement(sifsr, hw):
    """Measured on an MI355X (relative deviation from the restatement, largest over the six images): PSNR 0, RMSE and strata
    7.9e-8, GSSIM 7.1e-15, RMSE_grad 1.2e-16; SSIM at Kelvin scale 1.91e-3 at (41, 57) seed 3 (599 windows of a smooth 300 K
    field: the float32 cancellation in uxx - ux^2 that the 2e-3 bar of tests/test_eval_metrics_gpu.py exists for) and 2.2e-4 at
    (96, 80)."""
    a, b, m = R.blob_case(hw)
    got, cnt = rows_of(sifsr, a, b, m)
    g, q25, q75, cnt2 = sifsr.metrics.masked_gradient_strata(dev(a)[:, None], dev(b)[:, None], dev(m))
    assert np.array_equal(cnt2.cpu().numpy(), cnt)
    gu = g[:, 0].cpu().numpy().view(np.uint32)
    for i in range(len(a)):
        want, wx = R.metrics(a[i], b[i], m[i])
        assert tuple(cnt[i]) == wx["counts"], (i, cnt[i], wx["counts"])
        assert min(wx["counts"]) >= 300
        check_masked_row(got[i], want, "k", f"{hw} image {i}")
        # the set S is marked in g, g on S is the restatement's, and the quartiles are numpy's on those values, byte for byte
        assert np.array_equal(gu[i] != G_OUT, wx["S"])
        gs = gu[i][wx["S"]].view(np.float32)
        assert np.array_equal(gs, wx["g"][wx["S"]])
        p25, p75 = np.percentile(gs, 25), np.percentile(gs, 75)
        assert np.float32(q25[i].item()).tobytes() == np.float32(p25).tobytes(), (q25[i].item(), p25)
        assert np.float32(q75[i].item()).tobytes() == np.float32(p75).tobytes(), (q75[i].item(), p75)
    # a given data range replaces R in PSNR, SSIM and GSSIM
    got_r, cnt_r = rows_of(sifsr, a[:1], b[:1], m[:1], data_range=40.0)
    check_masked_row(got_r[0], R.metrics(a[0], b[0], m[0], data_range=40.0)[0], "k", f"{hw} data_range 40")
    assert np.array_equal(cnt_r[0], cnt[0]) and np.array_equal(bits(got_r[0, [2, 3, 4, 5, 7]]), bits(got[0, [2, 3, 4, 5, 7]]))


# ---- 2. every pixel valid: the unmasked table, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (2, 41, 57), (1, 335, 374), (64, 256, 256)])
def test_all_valid_is_aster_metrics_bit_for_bit(sifsr, B, H, W):
    rs = np.random.RandomState(H + W)
    if B == 64:                                                       # one pair, rolled: the batch is there for the grid, not the data
        a0, b0 = R.pair(rs, H, W)
        a, b = np.stack([np.roll(a0, 3 * i, 1) for i in range(B)]), np.stack([np.roll(b0, 3 * i, 1) for i in range(B)])
    else:
        pairs = [R.pair(rs, H, W) for _ in range(B)]
        a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    A, Bt = dev(a)[:, None], dev(b)[:, None]
    want = sifsr.metrics.aster_metrics(A, Bt)
    counts = [H * W, (H - 2) * (W - 2), (H - 6) * (W - 6), (H - 8) * (W - 8), H * W]
    for valid in (None, torch.ones((B, H, W), dtype=U8, device="cuda"), torch.full((B, 1, H, W), 255, dtype=U8, device="cuda"),
                  torch.ones((B, H, W), dtype=torch.bool, device="cuda")):
        got, cnt = sifsr.metrics.masked_aster_metrics(A, Bt, valid, return_counts=True)
        assert bit_equal(got, want)
        assert cnt.cpu().tolist() == [counts] * B
    assert bit_equal(sifsr.metrics.masked_aster_metrics(A, Bt, data_range=35.5), sifsr.metrics.aster_metrics(A, Bt, data_range=35.5))


# ---- 3. no-data values in the images are the mask; invalid pixels are inert ------------------------------------------------------
@pytest.mark.parametrize("hw", R.BLOB_SHAPES)
def test_nodata_is_the_mask_and_invalid_pixels_are_inert(sifsr, hw):
    a, b, m = R.blob_case(hw)
    want, cnt = rows_of(sifsr, a, b, m)
    hole = m == 0
    for junk in (np.nan, np.inf, 0.0, 1e30):
        pa, pb = a.copy(), b.copy()
        pa[hole] = junk
        pb[hole] = -junk
        for qa, qb in ((pa, pb), (pa, b), (a, pb)):
            got, c = rows_of(sifsr, qa, qb, m)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(c, cnt), junk
        if junk != 1e30:                                  # NaN, inf and 0 K are no-data on their own
            for qa, qb in ((pa, b), (a, pb)):
                got, c = rows_of(sifsr, qa, qb, None)
                assert np.array_equal(bits(got), bits(want)) and np.array_equal(c, cnt), junk
    # half of the holes in the mask, the other half as NaN in the reference and 0 in the prediction
    half = hole & (np.arange(hw[1])[None, None, :] % 2 == 0)
    pa, pb = a.copy(), b.copy()
    pa[half & (np.arange(hw[0])[None, :, None] % 2 == 0)] = np.nan
    pb[half & (np.arange(hw[0])[None, :, None] % 2 == 1)] = 0.0
    got, c = rows_of(sifsr, pa, pb, (~(hole & ~half)).astype(np.uint8))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(c, cnt)


# ---- 4. edge counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(16, 16), (24, 40)])
def test_edge_counts(sifsr, hw):
    a, b, m = R.edge_case(hw)
    got, cnt = rows_of(sifsr, a, b, m)
    want = [R.metrics(a[i], b[i], m[i]) for i in range(4)]
    assert cnt.tolist() == [list(w[1]["counts"]) for w in want]
    assert cnt[0].tolist() == [0] * 5 and np.isnan(got[0]).all()                           # nothing valid: a row of NaN
    assert cnt[1].tolist() == [81, 49, 9, 1, 1] and cnt[2].tolist() == [81, 49, 9, 1, 25]
    for i in (1, 2, 3):
        check_masked_row(got[i], want[i][0], "z", f"{hw} image {i} counts {cnt[i].tolist()}")
    g, q25, q75, _ = sifsr.metrics.masked_gradient_strata(dev(a)[:, None], dev(b)[:, None], dev(m))
    gu = g[:, 0].cpu().numpy().view(np.uint32)
    one = gu[1][gu[1] != G_OUT].view(np.float32)
    assert one.shape == (1,) and q25[1].item() == q75[1].item() == one[0] == want[1][1]["g"][want[1][1]["S"]][0]
    assert got[1][3] == 0 and got[1][4] == got[1][5] > 0                                    # one value: below nothing, in both others
    assert np.array_equal(gu[2] != G_OUT, want[2][1]["S"]) and (gu[0] == G_OUT).all()
    # a row of a batch is its own B = 1 call, whatever its neighbours hold
    for i in range(4):
        one_row, one_cnt = rows_of(sifsr, a[i:i + 1], b[i:i + 1], m[i:i + 1])
        assert np.array_equal(bits(one_row[0]), bits(got[i])) and np.array_equal(one_cnt[0], cnt[i])


def test_a_perfect_prediction(sifsr):
    a, _, m = R.blob_case((41, 57))
    got, cnt = rows_of(sifsr, a, a, m)
    assert (got[:, 0] == np.inf).all() and (got[:, 1] == 1.0).all() and (got[:, [2, 3, 4, 5, 7]] == 0).all()      # mse = 0: +inf stays


# ---- 5. lists, determinism, graph ------------------------------------------------------------------------------------------------
def test_lists_determinism_and_graph(sifsr):
    a, b, m = R.blob_case((96, 80))
    a1, b1, m1 = R.blob_case((41, 57))
    A, Bt, M = dev(a)[:, None], dev(b)[:, None], dev(m)
    r1, c1 = sifsr.metrics.masked_aster_metrics(A, Bt, M, return_counts=True)
    r2, c2 = sifsr.metrics.masked_aster_metrics(A, Bt, M, return_counts=True)
    assert bit_equal(r1, r2) and torch.equal(c1, c2)
    small, csmall = sifsr.metrics.masked_aster_metrics(dev(a1)[:, None], dev(b1)[:, None], dev(m1), return_counts=True)
    rows, cnt = sifsr.metrics.masked_aster_metrics([A[0, 0], dev(a1[1]), A[1], dev(a1[0])[None]], [Bt[0, 0], dev(b1[1]), Bt[1], dev(b1[0])[None]],
                                                   [M[0], dev(m1[1]), M[1][None], dev(m1[0]).bool()], return_counts=True)
    for k, (src, csrc, i) in enumerate(((r1, c1, 0), (small, csmall, 1), (r1, c1, 1), (small, csmall, 0))):
        assert bit_equal(rows[k], src[i]) and torch.equal(cnt[k], csrc[i]), k
    nomask = sifsr.metrics.masked_aster_metrics([A[0, 0], dev(a1[1])], [Bt[0, 0], dev(b1[1])])
    assert bit_equal(nomask, sifsr.metrics.aster_metrics([A[0, 0], dev(a1[1])], [Bt[0, 0], dev(b1[1])]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sifsr.metrics.masked_aster_metrics(A, Bt, M)          # warm up outside the capture
        sifsr.metrics.masked_psnr_ssim(A, Bt, M)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, cnt = sifsr.metrics.masked_aster_metrics(A, Bt, M, return_counts=True)
        ps = torch.stack(sifsr.metrics.masked_psnr_ssim(A, Bt, M))
    graph.replay()
    torch.cuda.synchronize()
    assert bit_equal(out, r1) and torch.equal(cnt, c1)
    assert bit_equal(ps, torch.stack(sifsr.metrics.masked_psnr_ssim(A, Bt, M)))


def test_errors(sifsr):
    Err = sifsr.SifsrError
    z = torch.zeros((2, 1, 24, 24), device="cuda")
    ok = torch.ones((2, 24, 24), dtype=U8, device="cuda")
    for valid in (ok.float(), ok[:, :20], ok.cpu(), ok[:1]):
        with pytest.raises(Err):
            sifsr.metrics.masked_aster_metrics(z, z, valid)
    with pytest.raises(Err):
        sifsr.metrics.masked_aster_metrics(z[:, :, :12], z[:, :, :12])
    with pytest.raises(Err):
        sifsr.metrics.masked_aster_metrics([z[0]], [z[0]], [ok[0], ok[1]])
    for valid in (ok.float(), ok[:, :12, :12], ok.cpu(), ok[:1], ok[0]):
        with pytest.raises(Err):
            sifsr.metrics.masked_psnr_ssim(z, z, valid)


# ---- 6. memory contract ----------------------------------------------------------------------------------------------------------
def _contract_mask(H, W, B, seed):
    """masks under which every count of every image is positive (an output of the contract run must not be NaN)"""
    if H == 16:
        m = np.ones((B, H, W), np.uint8)
        m[0, :2, :2] = 0
        return m
    return np.stack([R.blob_mask(H, W, seed + i) for i in range(B)])


def eval_case(hw, masked=True, B=2):
    def make(k):
        import sifsr
        H, W = hw
        ref, pred = k.i("ref", B, 1, H, W, scale=3.0, shift=300.0), k.i("pred", B, 1, H, W, scale=3.0, shift=300.0)
        mask = k.t("mask", torch.from_numpy(_contract_mask(H, W, B, int(k.rs.randint(1, 4))) * 9)) if masked else None
        need = k.L.call("sifsrv_eval_metrics_scratch_bytes", B, H, W)
        scratch = k.A.scratch(need, "scratch")                    # poisoned scratch: nothing of it may reach the outputs
        out8, counts5 = k.o("out8", B, 8, dtype=F64), k.o("counts5", B, 5, dtype=I32)
        taps = sifsr.sif_ops._taps_c(0.1, 4, None)
        call = lambda: k.L.call("sifsrv_eval_metrics", ref, pred, mask, B, H, W, taps, -1.0, scratch, need, out8, counts5, S())
        return call, {"out8": out8, "counts5": counts5}
    return make


def psnr_case(hw, scale, B=2):
    def make(k):
        H, W = hw
        pred, targ = k.i("pred", B, 1, H, W), k.i("targ", B, 1, H, W)
        m = _contract_mask(H // scale, W // scale, B, int(k.rs.randint(1, 4))) if H // scale != 4 else np.ones((B, 4, 4), np.uint8)
        m[0, 0, 0] = 0
        valid = k.t("valid", torch.from_numpy(m * 3))
        need = k.L.call("sifsrv_psnr_ssim_scratch_bytes", B, H, W)
        scratch = k.A.scratch(need, "scratch")
        out2, counts2 = k.o("out2", 2), k.o("counts2", 2, dtype=I32)
        call = lambda: k.L.call("sifsrv_psnr_ssim", pred, targ, valid, scale, B, H, W, scratch, need, out2, counts2, S())
        return call, {"out2": out2, "counts2": counts2}
    return make


CONTRACT = {"sifsrv_eval_metrics": [eval_case(hw) for hw in ((16, 16), (41, 57), (96, 80))] + [eval_case((41, 57), masked=False)],
            "sifsrv_psnr_ssim": [psnr_case((16, 16), 4), psnr_case((16, 16), 1), psnr_case((41, 57), 1), psnr_case((96, 80), 4)]}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output written in full and nowhere else -- NaN-free under the NaN poison, bit-identical under every poison (the
    poisoned scratch included) --, const inputs untouched, and the same bits on ordinary allocations."""
    first = run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=64 << 20)
    if name == "sifsrv_eval_metrics":
        assert (first["counts5"] > 0).all()


def test_scratch_too_small(sifsr, L):
    a, b, m = R.blob_case((41, 57))
    A, Bt, M = dev(a), dev(b), dev(m)
    p = lambda t: t.data_ptr()
    taps = sifsr.sif_ops._taps_c(0.1, 4, None)
    need = L.call("sifsrv_eval_metrics_scratch_bytes", 3, 41, 57)
    ws = torch.full((need,), 77, dtype=U8, device="cuda")
    out8, counts5 = torch.full((3, 8), 77.0, dtype=F64, device="cuda"), torch.full((3, 5), 77, dtype=I32, device="cuda")
    fn = L.lib().sifsrv_eval_metrics
    args = lambda nbytes: (p(A), p(Bt), p(M), 3, 41, 57, taps, -1.0, p(ws), nbytes, p(out8), p(counts5), S())
    assert fn(*args(need - 1)) == WORKSPACE_ERR and fn(*args(0)) == WORKSPACE_ERR
    torch.cuda.synchronize()
    assert (ws == 77).all() and (out8 == 77).all() and (counts5 == 77).all()
    assert fn(*args(need)) == 0
    torch.cuda.synchronize()
    assert not (out8 == 77).any() and not (counts5 == 77).any()
    need = L.call("sifsrv_psnr_ssim_scratch_bytes", 3, 41, 57)
    ws = torch.full((need,), 77, dtype=U8, device="cuda")
    out2, counts2 = torch.full((2,), 77.0, device="cuda"), torch.full((2,), 77, dtype=I32, device="cuda")
    fn = L.lib().sifsrv_psnr_ssim
    args = lambda nbytes: (p(Bt), p(A), p(M), 1, 3, 41, 57, p(ws), nbytes, p(out2), p(counts2), S())
    assert fn(*args(need - 1)) == WORKSPACE_ERR and fn(*args(0)) == WORKSPACE_ERR
    torch.cuda.synchronize()
    assert (ws == 77).all() and (out2 == 77).all() and (counts2 == 77).all()
    assert fn(*args(need)) == 0
    torch.cuda.synchronize()
    assert not (out2 == 77).any() and counts2.tolist() == [3, 3]


# ---- 7. the train-time pair ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_reference():
    """the restatement of every train-time case, computed once"""
    out = {}
    for hw in R.TRAIN_SHAPES:
        for kelvin in (False, True):
            p, t = R.train_inputs(hw, kelvin)
            for scale in (1, 4):
                for kind in R.TRAIN_MASKS:
                    v = R.train_mask(hw, scale, kind)
                    out[hw, kelvin, scale, kind] = (p, t, v, R.psnr_ssim(p, t, v, scale))
    return out


@pytest.mark.parametrize("kelvin", [False, True], ids=["z", "kelvin"])
@pytest.mark.parametrize("scale", [4, 1])
@pytest.mark.parametrize("hw", R.TRAIN_SHAPES)
def test_masked_psnr_ssim(sifsr, train_reference, hw, scale, kelvin):
    for kind in R.TRAIN_MASKS:
        p, t, v, (ps_ref, ss_ref, n_ref) = train_reference[hw, kelvin, scale, kind]
        P, T, V = dev(p), dev(t), dev(v)
        ps, ss, cnt = sifsr.metrics.masked_psnr_ssim(P, T, V[:, None], return_counts=True)
        print(f"{hw} x{scale} {'K' if kelvin else 'z'} {kind}: psnr {float(ps):.7g} vs {ps_ref:.7g} (rel {abs(float(ps) - ps_ref) / abs(ps_ref):.2e}), "
              f"ssim {float(ss):.7g} vs {ss_ref:.7g} (rel {abs(float(ss) - ss_ref) / abs(ss_ref):.2e}), images {cnt.tolist()}")
        assert tuple(cnt.tolist()) == n_ref
        assert abs(float(ps) - ps_ref) < 1e-4 * abs(ps_ref)
        if kind == "single":
            assert n_ref == (1, 0) and np.isnan(float(ss))          # a 4 x 4 block holds no 7 x 7 window: PSNR contributes, SSIM not
        else:
            assert abs(float(ss) - ss_ref) < (2e-3 if kelvin else 1e-4) * abs(ss_ref)
        # what the invalid pixels hold changes no bit; a bool mask and the (B,h,w) layout are the same mask
        hole = ~R.upsampled(v, scale)
        for junk in (np.nan, 1e30):
            qp, qt = p.copy(), t.copy()
            qp[:, 0][hole] = junk
            qt[:, 0][hole] = -junk
            again = sifsr.metrics.masked_psnr_ssim(dev(qp), dev(qt), V != 0)
            assert bit_equal(again[0], ps) and bit_equal(again[1], ss)


@pytest.mark.parametrize("B,H,W", [(2, 40, 24), (2, 64, 64), (2, 100, 36), (300, 8, 8)])
def test_all_valid_is_psnr_ssim_bit_for_bit(sifsr, B, H, W):
    for kelvin in (False, True):
        p, t = R.train_inputs((H, W), kelvin, B)
        P, T = dev(p), dev(t)
        want = sifsr.metrics.psnr_ssim(P, T)
        for scale, fill in ((4, 1), (1, 255)):
            valid = torch.full((B, 1, H // scale, W // scale), fill, dtype=U8, device="cuda")
            ps, ss, cnt = sifsr.metrics.masked_psnr_ssim(P, T, valid, return_counts=True)
            assert bit_equal(ps, want[0]) and bit_equal(ss, want[1]) and cnt.tolist() == [B, B]
    none = sifsr.metrics.masked_psnr_ssim(P, T, torch.zeros_like(valid), return_counts=True)
    assert torch.isnan(none[0]) and torch.isnan(none[1]) and none[2].tolist() == [0, 0]


# ---- 8. the epoch keyword --------------------------------------------------------------------------------------------------------
def test_masked_metrics_of_an_epoch(sifsr):
    from tests.test_masked_gpu import mined_with_holes, small_model
    mined, _, _ = mined_with_holes(sifsr, n=10, w=16, seed=5)
    stats = mined.statistics(None, valid_only=True)
    batch = next(iter(mined.masked_loader(None, 2, stats, shuffle=False)))
    lst, lst_up, ndvi, valid, n = batch
    assert tuple(lst_up.shape) == (2, 1, 64, 64) and 0 < int(n) < 2 * 256
    m = small_model(sifsr)
    default = sifsr.train.eval_epoch(m, [batch], stats, 0.5, -0.25)
    masked = sifsr.train.eval_epoch(m, [batch], stats, 0.5, -0.25, masked_metrics=True)
    with torch.inference_mode():
        sr = m.eval()(torch.cat((lst_up, ndvi), dim=1))
        ps, ss = sifsr.metrics.masked_psnr_ssim(sr, lst_up, valid)
    print(f"default psnr / ssim {default[3]:.6f} / {default[4]:.6f}, over the valid pixels {masked[3]:.6f} / {masked[4]:.6f}")
    assert masked[:3] == default[:3]
    assert masked[3] == float(ps) and masked[4] == float(ss) and np.isfinite(masked).all()
    assert masked[3] != default[3] and masked[4] != default[4]
    ones = (lst, lst_up, ndvi, torch.ones_like(valid), torch.tensor(2 * 256, device="cuda"))
    a = sifsr.train.eval_epoch(m, [ones], stats, 0.5, -0.25)
    b = sifsr.train.eval_epoch(m, [ones], stats, 0.5, -0.25, masked_metrics=True)
    assert a == b
    # a batch of three is scored as before, and a batch without a valid pixel leaves the means of the others
    three = sifsr.train.eval_epoch(m, [batch[:3]], stats, 0.5, -0.25, masked_metrics=True)
    assert three[3:] == sifsr.train.eval_epoch(m, [batch[:3]], stats, 0.5, -0.25)[3:]
    empty = (lst, lst_up, ndvi, torch.zeros_like(valid), torch.tensor(0, device="cuda"))
    both = sifsr.train.eval_epoch(m, [batch, empty], stats, 0.5, -0.25, masked_metrics=True)
    assert both[3:] == masked[3:]
    # the training epoch takes the keyword too
    opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
    out = sifsr.train.train_epoch(m, [batch], opt, stats, 0.5, -0.25, "sr2", masked_metrics=True)
    assert len(out) == 5 and np.isfinite(out).all()
