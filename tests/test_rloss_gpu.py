"""GPU: the fused, masked SIF loss at any ratio (include/sifsr_rloss.h, sifsr/rloss.py) against the float64
restatement tests/rloss_reference.py (built from the operators of tests/sensor_reference.py; tests/test_rloss_host.py), against
the composed path sensor.sif_loss, and through the training step and adapt_granule.

Bars: the project's parity bar, 1e-4 relative for the three losses and 1e-4 max|dsr_ref| per element of dsr (f9, f17); bits where
the header promises bits.  There is no x4 cross-check against masked_sif_loss_with_grad: tests/test_rloss_host.py found that the two
statements of the x4 operator differ (the /4 kernels and the oracle use the reference's fp32 PSF taps), DESIGN.md §9 f19.

Shapes (tests/rloss_reference.SHAPES), B = 2: an integer factor, cells of 2 and 3 pixels, a non-terminating ratio, hw = 2, the x4
operator, two shapes with several LR tiles per image and ragged last tiles in both axes, and factor 8, where the LR tile is 8 x 8
cells so that the staged region fits the LDS.

Measured on an MI355X over every case of this file (printed by each test): see DESIGN.md §9 f19."""
import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import adapt_reference as A
from tests import rloss_reference as Q
from tests.conftest import rel_err
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal

pytestmark = pytest.mark.gpu
PARITY = 1e-4
MEAN, STD = Q.MEAN, Q.STD
ALPHA, GAMMA = 0.5, -0.25
K2 = {"sr2": 2, "sr1": 1}


def fused(sifsr, shape, kind, alpha, gamma, mask, lst=None):
    """-> (losses3, dsr) of the case on the device"""
    sr, lst0, ndvi, valid, _, _, _ = Q.loss_reference(shape, kind, alpha, gamma, mask)
    lst = lst0 if lst is None else lst
    v = valid.cuda()
    counts = sifsr.rloss.valid_counts(v, shape[:2])
    return sifsr.rloss.sif_loss_with_grad(kind, sr.cuda(), lst.cuda(), ndvi.cuda(), shape[2], MEAN, STD, alpha, gamma, valid=v, counts=counts)


def assert_parity(tag, losses, dsr, ref_losses, ref_g):
    """-> (worst relative loss error, worst dsr error as a fraction of max|dsr_ref|)"""
    worst = 0.0
    for name, a, b in zip(("ds", "pl", "loss"), losses.tolist(), ref_losses):
        e = abs(a - b) / abs(b) if b != 0 else abs(a)
        worst = max(worst, e)
        assert e <= PARITY, (tag, name, a, b)
    top = float(ref_g.abs().max())
    err = float((dsr.double().cpu() - ref_g).abs().max())
    assert err <= PARITY * top, (tag, err, top)
    return worst, (err / top if top > 0 else 0.0)


# ---- 1. parity with the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Q.SHAPES, ids=str)
def test_parity_with_the_restatement(sifsr, shape):
    """every (kind, alpha, gamma) x every mask: losses3 and dsr inside the parity bar; the empty mask gives exact zeros, a wholly
    invalid image has dsr exactly 0"""
    wl = wg = 0.0
    for kind, alpha, gamma in Q.KINDS:
        for mask in Q.MASKS:
            _, _, _, valid, counts, ref_losses, ref_g = Q.loss_reference(shape, kind, alpha, gamma, mask)
            losses, dsr = fused(sifsr, shape, kind, alpha, gamma, mask)
            assert dsr.shape == ref_g.shape and losses.shape == (3,) and dsr.dtype == losses.dtype == torch.float32
            if mask == "none":
                assert counts == (0, 0) and not losses.any() and not dsr.any() and ref_losses == (0.0, 0.0, 0.0)
                continue
            a, b = assert_parity((shape, kind, alpha, mask), losses, dsr, ref_losses, ref_g)
            wl, wg = max(wl, a), max(wg, b)
            if mask in ("image0", "single"):
                assert not dsr[0].any() and dsr[1].any()
    print(f"{shape}: worst relative loss error {wl:.2e}, worst |dsr - ref| / max|ref| {wg:.2e}")


@pytest.mark.parametrize("shape", [Q.SHAPES[0], Q.SHAPES[1], Q.SHAPES[5], Q.SHAPES[7]], ids=str)
def test_against_the_composed_path(sifsr, shape):
    """all valid: sensor.sif_loss and its autograd gradient on the same device tensors"""
    sr, lst, ndvi = (t.cuda() for t in Q.loss_inputs(shape))
    for kind, alpha, gamma in Q.KINDS[:3]:
        s = sr.clone().requires_grad_(True)
        want = sifsr.sensor.sif_loss(kind, s, lst, ndvi, shape[2], MEAN, STD, alpha, gamma)
        want[2].backward()
        losses, dsr = sifsr.rloss.sif_loss_with_grad(kind, sr, lst, ndvi, shape[2], MEAN, STD, alpha, gamma)
        worst = max(abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(losses, (t.detach() for t in want)))
        e = rel_err(dsr, s.grad)
        print(f"{shape} {kind}: against sensor.sif_loss: losses {worst:.2e}, d loss / d sr {e:.2e}")
        assert worst <= PARITY and e <= PARITY
        # ... and through the autograd form
        s2 = sr.clone().requires_grad_(True)
        ds, pl, loss = sifsr.rloss.sif_loss(kind, s2, lst, ndvi, shape[2], MEAN, STD, alpha, gamma)
        assert not ds.requires_grad and not pl.requires_grad and loss.requires_grad and ds.dim() == pl.dim() == loss.dim() == 0
        (3.0 * loss).backward()
        assert bit_equal(torch.stack((ds, pl, loss.detach())), losses) and torch.equal(s2.grad, dsr * 3.0)


@pytest.mark.parametrize("shape", [Q.SHAPES[1], Q.SHAPES[6]], ids=str)
def test_unmasked_is_the_all_ones_mask_bit_for_bit(sifsr, shape):
    """both paths form their scales on the device by the same expressions"""
    sr, lst, ndvi = (t.cuda() for t in Q.loss_inputs(shape))
    for kind, alpha, gamma in Q.KINDS[:2]:
        a = sifsr.rloss.sif_loss_with_grad(kind, sr, lst, ndvi, shape[2], MEAN, STD, alpha, gamma)
        b = fused(sifsr, shape, kind, alpha, gamma, "all")
        assert bit_equal(a[0], b[0]) and bit_equal(a[1], b[1])
        # sif_loss forms the counts itself
        c = sifsr.rloss.sif_loss(kind, sr, lst, ndvi, shape[2], MEAN, STD, alpha, gamma, valid=Q.loss_mask(shape, "all").cuda())
        assert bit_equal(torch.stack(c), a[0])


# ---- 2. masks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [Q.SHAPES[1], Q.SHAPES[5]], ids=str)
def test_nan_at_invalid_targets_changes_no_bit(sifsr, shape):
    for kind, alpha, gamma in Q.KINDS[:2]:
        for mask in ("blobs30", "image0", "single"):
            _, lst, _, valid, _, _, _ = Q.loss_reference(shape, kind, alpha, gamma, mask)
            poisoned = lst.clone()
            poisoned[valid == 0] = float("nan")
            assert torch.isnan(poisoned).any()
            a, b = fused(sifsr, shape, kind, alpha, gamma, mask), fused(sifsr, shape, kind, alpha, gamma, mask, lst=poisoned)
            assert bit_equal(a[0], b[0]) and bit_equal(a[1], b[1]) and not torch.isnan(b[1]).any()


@pytest.mark.parametrize("shape", [Q.SHAPES[0], Q.SHAPES[1]], ids=str)
def test_the_rim_of_a_gap_is_still_constrained(sifsr, shape):
    """alpha = 1: an HR pixel under an INVALID cell that borders a valid one has a non-zero gradient, the restatement's"""
    for kind in ("sr2", "sr1"):
        _, _, _, valid, _, _, ref_g = Q.loss_reference(shape, kind, 1.0, GAMMA if kind == "sr2" else -0.5, "blobs30")
        _, dsr = fused(sifsr, shape, kind, 1.0, GAMMA if kind == "sr2" else -0.5, "blobs30")
        v = valid.numpy() != 0
        near = np.zeros_like(v)
        near[..., 1:, :] |= v[..., :-1, :]; near[..., :-1, :] |= v[..., 1:, :]; near[..., :, 1:] |= v[..., :, :-1]; near[..., :, :-1] |= v[..., :, 1:]
        rim = torch.from_numpy(Q.hr_mask(~v & near, shape[0], shape[1]))
        got, ref = dsr.cpu()[rim], ref_g[rim]
        assert rim.any() and (got != 0).any() and (ref != 0).any()
        assert float((got.double() - ref).abs().max()) <= PARITY * float(ref_g.abs().max())


def test_repeatability_and_independence(sifsr):
    shape = Q.SHAPES[5]
    for kind, alpha, gamma in Q.KINDS[:2]:
        a, b = fused(sifsr, shape, kind, alpha, gamma, "blobs30"), fused(sifsr, shape, kind, alpha, gamma, "blobs30")
        assert bit_equal(a[0], b[0]) and bit_equal(a[1], b[1])
        # dsr = NULL: the same losses3 bits
        sr, lst, ndvi, valid, _, _, _ = Q.loss_reference(shape, kind, alpha, gamma, "blobs30")
        sr, lst, ndvi, v = sr.cuda(), lst.cuda(), ndvi.cuda(), valid.cuda()
        counts = sifsr.rloss.valid_counts(v, shape[:2])
        k = K2[kind]
        need = L_call_size(sifsr, k, Q.B, shape)
        ws, out = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.full((3,), -7.0, device="cuda")
        sifsr._lib.call("sifsrq_sif_loss", k, sr, lst, v, counts, ndvi, Q.B, shape[0], shape[1], shape[2], MEAN, STD, alpha, gamma, ws, need,
                        out, None, S())
        assert bit_equal(out, a[0])
        # image 1 of a B = 2 call with image 0 wholly invalid = its own B = 1 call with the same counts
        v0 = Q.loss_mask(shape, "image0").cuda()
        c0 = sifsr.rloss.valid_counts(v0, shape[:2])
        two = sifsr.rloss.sif_loss_with_grad(kind, sr, lst, ndvi, shape[2], MEAN, STD, alpha, gamma, valid=v0, counts=c0)
        one = sifsr.rloss.sif_loss_with_grad(kind, sr[1:], lst[1:], ndvi[1:], shape[2], MEAN, STD, alpha, gamma, valid=v0[1:], counts=c0)
        assert bit_equal(two[1][1:], one[1]) and not two[1][0].any()


def L_call_size(sifsr, k, B, shape):
    return sifsr._lib.call("sifsrq_sif_loss_workspace_bytes", k, B, shape[0], shape[1], shape[2])


@pytest.mark.parametrize("shape", Q.SHAPES, ids=str)
def test_valid_counts(sifsr, shape):
    H, W, f = shape
    h, w = Q.lr_shape(H, W, f)
    last = np.zeros((3, 1, h, w), np.uint8)
    last[2, 0, h - 1, w - 1] = 200
    rs = np.random.RandomState(H + W)
    for v in (Q.loss_mask(shape, m).numpy() for m in Q.MASKS):
        got = sifsr.rloss.valid_counts(torch.from_numpy(v).cuda(), (H, W))
        assert got.dtype == torch.int64 and got.shape == (2,) and tuple(got.tolist()) == Q.counts_ref(v, H, W)
    for v in (last, (rs.uniform(size=(5, h, w)) > 0.5).astype(np.uint8), np.ones((1, h, w), bool)):
        assert tuple(sifsr.rloss.valid_counts(torch.from_numpy(v).cuda(), (H, W)).tolist()) == Q.counts_ref(v, H, W)
    # the single valid cell of the last row and column holds the pixels from ceil((n - 1) N / n) on
    assert Q.counts_ref(last, H, W) == (1, (H - -(-((h - 1) * H) // h)) * (W - -(-((w - 1) * W) // w)))


def test_graph_replay(sifsr):
    """captured once on static buffers, replayed with three masks and inputs copied in: the eager results, bit for bit"""
    shapes = [Q.SHAPES[1]]
    shape = shapes[0]
    H, W, f = shape
    h, w = Q.lr_shape(H, W, f)
    sr, lst, ndvi = (torch.zeros((Q.B, 1) + s, device="cuda") for s in ((H, W), (h, w), (H, W)))
    v = torch.ones((Q.B, 1, h, w), dtype=torch.uint8, device="cuda")

    def run():
        counts = sifsr.rloss.valid_counts(v, (H, W))
        return sifsr.rloss.sif_loss_with_grad("sr2", sr, lst, ndvi, f, MEAN, STD, ALPHA, GAMMA, valid=v, counts=counts)

    def load(seed, mask):
        rs = np.random.RandomState(seed)
        for t in (sr, lst, ndvi):
            t.copy_(torch.from_numpy(rs.standard_normal(tuple(t.shape)).astype(np.float32)))
        v.copy_(Q.loss_mask(shape, mask))

    load(1, "all")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses_g, dsr_g = run()
    seen = []
    for seed, mask in ((2, "blobs30"), (3, "single"), (4, "all")):
        load(seed, mask)
        graph.replay()
        torch.cuda.synchronize()
        got = (losses_g.clone(), dsr_g.clone())
        want = run()
        torch.cuda.synchronize()
        assert bit_equal(got[0], want[0]) and bit_equal(got[1], want[1]) and float(want[1].abs().max()) > 0
        seen.append(got[0])
    assert not bit_equal(seen[0], seen[1]) and not bit_equal(seen[1], seen[2])


# ---- 3. the training step and adapt_granule -----------------------------------------------------------------------------------------
def step_inputs(B=4, H=24, W=24, factor=3.0, seed=72):
    x, _, _ = A.network_inputs(seed, B, H, W)
    h, w = Q.lr_shape(H, W, factor)
    rs = np.random.RandomState(seed + 1)
    lst = torch.from_numpy(rs.standard_normal((B, 1, h, w)).astype(np.float32))
    valid = torch.from_numpy(np.stack([Q.blobs(h, w, rs) for _ in range(B)])[:, None])
    return x, lst, valid


def test_train_step_masked_against_the_restatement(sifsr):
    """HR (24, 24), x3, B = 4, a 30 % mask: the losses at the returned sr"""
    from tests.test_model_gpu import make_model
    x, lst, valid = step_inputs()
    for kind, alpha, gamma in Q.KINDS[:2]:
        m = make_model(sifsr, O.synthetic_state(71))
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
        p0 = m.flat_parameters().detach().clone()
        out = sifsr.rloss.train_step(m, opt, lst.cuda(), x[:, 0:1].cuda().contiguous(), x[:, 1:2].cuda().contiguous(), A.STATS, alpha, gamma, 3.0,
                                     kind=kind, valid=valid.cuda(), return_sr=True)
        assert len(out) == 4 and m.training and not out[2].requires_grad and not torch.equal(m.flat_parameters(), p0)
        ref = Q.loss_ref(kind, out[3].cpu(), lst, valid, x[:, 1:2], 3.0, MEAN, STD, alpha, gamma)
        for name, a, b in zip(("ds", "pl", "loss"), out[:3], ref):
            print(f"[{kind}] masked step {name}: {float(a):.8f} | float64 {float(b):.8f}")
            assert abs(float(a) - float(b)) <= PARITY * abs(float(b)), (kind, name)


def test_train_step_all_valid_is_sensor_train_step(sifsr):
    """all valid: the three losses and every parameter after one step against sensor.train_step from the same start"""
    from tests.test_model_gpu import make_model
    x, lst, _ = step_inputs()
    sd = O.synthetic_state(71)
    args = lambda: (lst.cuda(), x[:, 0:1].cuda().contiguous(), x[:, 1:2].cuda().contiguous(), A.STATS, ALPHA, GAMMA, 3.0)
    for kind in ("sr2", "sr1"):
        ma, mb = make_model(sifsr, sd), make_model(sifsr, sd)
        oa, ob = sifsr.FlatAdam(ma.parameters(), lr=1e-3), sifsr.FlatAdam(mb.parameters(), lr=1e-3)
        p0 = ma.flat_parameters().detach().clone()
        got = sifsr.rloss.train_step(ma, oa, *args(), kind=kind, valid=torch.ones((4, 1, 8, 8), dtype=torch.uint8, device="cuda"), return_sr=True)
        want = sifsr.sensor.train_step(mb, ob, *args(), kind=kind, return_sr=True)
        assert bit_equal(got[3], want[3])                                    # the same forward: the same ReLU masks
        worst = max(abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(got[:3], want[:3]))
        eg = rel_err(ma.flat_grad(), mb.flat_grad())
        ep = rel_err(ma.flat_parameters(), mb.flat_parameters())
        print(f"[{kind}] fused step against sensor.train_step: losses {worst:.2e}, gradients {eg:.2e}, parameters after the step {ep:.2e}")
        assert worst <= PARITY and eg <= PARITY and ep <= PARITY and not torch.equal(ma.flat_parameters(), p0)


def test_train_step_with_frozen_batchnorm(sifsr):
    from tests.test_model_gpu import make_model
    x, lst, valid = step_inputs()
    m = make_model(sifsr, O.synthetic_state(71))
    m.bn_frozen = True
    opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
    p0 = m.flat_parameters().detach().clone()
    buffers = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    out = sifsr.rloss.train_step(m, opt, lst.cuda(), x[:, 0:1].cuda().contiguous(), x[:, 1:2].cuda().contiguous(), A.STATS, ALPHA, GAMMA, 3.0,
                                 valid=valid.cuda())
    assert len(out) == 3 and all(torch.isfinite(v) for v in out) and not torch.equal(m.flat_parameters(), p0) and buffers
    for k, v in m.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k


GRANULE = (40, 56)
LR_RATE, STEPS, BATCH = 1e-3, 3, 4


def ratio_granule(window, hr, seed=5):
    """-> (lst (40,56) fp32 [K] with a seeded cloud, a sprinkle of gaps and the block of tile (0, 0) wholly invalid, ndvi at hr / window)"""
    rs = np.random.RandomState(seed)
    h, w = GRANULE
    lst = rs.uniform(290.0, 325.0, (h, w)).astype(np.float32)
    lst[rs.uniform(size=(h, w)) < 0.04] = 0.0
    lst[0:16, 0:16] = 0.0
    lst[20:29, 30:41] = np.nan
    H, W = h * hr // window, w * hr // window
    return lst, np.clip(0.4 + 0.3 * rs.standard_normal((H, W)), -1.2, 1.2).astype(np.float32)


@pytest.mark.parametrize("window,hr", [(8, 24), (16, 40)])
def test_adapt_granule(sifsr, window, hr):
    from tests.test_model_gpu import make_model
    lst, ndvi = ratio_granule(window, hr)
    lst_d, ndvi_d = torch.from_numpy(lst).cuda(), torch.from_numpy(ndvi).cuda()
    filled, valid = sifsr.gaps.fill_gaps(lst_d)
    _, active, n_active = sifsr.gaps.select_tiles(valid, window, 2, True)
    n = int(n_active)
    tiles = sifsr.ratio.geometry(GRANULE, window, hr, 2, True).tiles
    assert 0 < n < tiles[0] * tiles[1]                                        # tile (0, 0) has no valid pixel
    sd = O.synthetic_state(37)
    m = make_model(sifsr, sd).eval()
    p0 = m.flat_parameters().detach().clone()
    buffers = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    res = sifsr.rloss.adapt_granule(m, lst_d, ndvi_d, A.STATS, window, hr, steps=STEPS, lr=LR_RATE, alpha=ALPHA, gamma=GAMMA, kind="sr2",
                                    batch=BATCH, overlap=2, cover_edges=True)
    assert isinstance(res, sifsr.adapt.Adaptation) and res.n_active == n and tuple(res.losses.shape) == (STEPS, 3)
    assert torch.isfinite(res.losses).all() and not m.training and m.bn_frozen is False
    assert not torch.equal(m.flat_parameters(), p0)
    for k, v in m.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k
    # step 0 against the restatement on tile_targets' outputs, at the prediction of the starting network with frozen statistics
    b = min(BATCH, n)
    x = sifsr.ratio.prepare_active_tiles(filled, ndvi_d, A.STATS, active, n_active, n, window, hr, 2, True)[:b]
    tl, tv, _ = sifsr.adapt.tile_targets(filled, valid, active, n_active, 0, b, A.STATS, window, 2, True)
    assert 0 < int((tv == 0).sum())                                           # the first batch holds cloudy cells
    with torch.no_grad():
        sr0 = make_model(sifsr, sd).eval()(x)
    ref = Q.loss_ref("sr2", sr0.cpu(), tl.cpu(), tv.cpu(), x[:, 1:2].cpu(), hr / window, MEAN, STD, ALPHA, GAMMA)
    for name, a, c in zip(("ds", "pl", "loss"), res.losses[0].tolist(), ref):
        print(f"[{window} -> {hr}] step 0 {name}: {a:.8f} | float64 {float(c):.8f}")
        assert abs(a - float(c)) <= PARITY * abs(float(c)), name
    res.restore()
    assert torch.equal(m.flat_parameters(), p0)


def test_adapt_granule_without_a_valid_pixel_and_refusals(sifsr):
    from tests.test_model_gpu import make_model
    m = make_model(sifsr, O.synthetic_state(37)).eval()
    p0 = m.flat_parameters().detach().clone()
    calls = []
    hook = m.register_forward_hook(lambda *a: calls.append(1))
    try:
        res = sifsr.rloss.adapt_granule(m, torch.zeros(GRANULE, device="cuda"), torch.zeros((120, 168), device="cuda"), A.STATS, 8, 24,
                                        steps=STEPS, batch=BATCH, overlap=2, cover_edges=True)
        assert res.n_active == 0 and res.losses.shape[0] == 0 and not calls and torch.equal(m.flat_parameters(), p0)
        res.restore()
        E = sifsr.SifsrError
        lst, ndvi = torch.full((32, 48), 300.0, device="cuda"), torch.zeros((40, 60), device="cuda")
        with pytest.raises(E, match=r"\(17, 17\)"):
            sifsr.rloss.adapt_granule(m, lst, ndvi, A.STATS, 16, 20)
        for bad in (lambda: sifsr.rloss.adapt_granule(m, lst, torch.zeros((96, 143), device="cuda"), A.STATS, 8, 24),
                    lambda: sifsr.rloss.adapt_granule(m, lst, torch.zeros((96, 144), device="cuda"), A.STATS, 8, 24, overlap=5),
                    lambda: sifsr.rloss.adapt_granule(m, lst, torch.zeros((96, 144), device="cuda"), A.STATS, 8, 24, batch=0),
                    lambda: sifsr.rloss.adapt_granule(m, lst.cpu(), torch.zeros((96, 144)), A.STATS, 8, 24)):
            with pytest.raises(E):
                bad()
        assert not calls and torch.equal(m.flat_parameters(), p0)
    finally:
        hook.remove()


# ---- 4. the C entry points: memory contract, errors ---------------------------------------------------------------------------------
# (shape, kind, mask or None for the unmasked call, with dsr)
LOSS_CONTRACT = [((24, 24, 3.0), "sr2", None, True), ((40, 56, 2.5), "sr1", "blobs30", True), ((96, 120, 3.0), "sr2", "blobs30", True),
                 ((80, 200, 2.5), "sr1", None, False), ((80, 104, Q.MAX_FACTOR), "sr2", "single", True), ((48, 32, 2.0), "sr2", "blobs30", False),
                 ((32, 48, 8.0 / 3.0), "sr1", "image0", True)]
COUNTS_CONTRACT = [((24, 24, 3.0), "blobs30"), ((80, 200, 2.5), "single"), ((40, 56, 2.5), "none"), ((96, 120, 3.0), "all")]


def loss_case(i):
    def make(k):
        shape, kind, mask, with_dsr = LOSS_CONTRACT[i]
        H, W, f = shape
        sr_, lst_, ndvi_ = Q.loss_inputs(shape)
        sr, ndvi = k.t("sr", sr_), k.t("ndvi", ndvi_)
        valid = counts = None
        if mask is not None:
            v = Q.loss_mask(shape, mask)
            lst_ = lst_.clone()
            lst_[v == 0] = float("nan")                           # never read
            valid = k.t("valid", v)
            counts = k.t("counts2", torch.tensor(Q.counts_ref(v.numpy(), H, W), dtype=torch.int64))
        lst = k.t("lst", lst_)
        losses = k.o("losses3", 3)
        dsr = k.o("dsr", Q.B, 1, H, W) if with_dsr else None
        need = k.L.call("sifsrq_sif_loss_workspace_bytes", K2[kind], Q.B, H, W, f)
        ws = k.A.scratch(need, "workspace")                       # poisoned scratch: nothing of it may reach the outputs
        outs = {"losses3": losses}
        if with_dsr:
            outs["dsr"] = dsr
        return (lambda: k.L.call("sifsrq_sif_loss", K2[kind], sr, lst, valid, counts, ndvi, Q.B, H, W, f, MEAN, STD, ALPHA, GAMMA, ws, need,
                                 losses, dsr, S())), outs
    return make


def counts_case(i):
    def make(k):
        shape, mask = COUNTS_CONTRACT[i]
        v = Q.loss_mask(shape, mask)
        valid = k.t("valid", v)
        counts = k.o("counts2", 2, dtype=torch.int64)
        return (lambda: k.L.call("sifsrq_valid_counts", valid, Q.B, v.shape[2], v.shape[3], shape[0], shape[1], counts, S())), {"counts2": counts}
    return make


CONTRACT = {"sifsrq_sif_loss": [loss_case(i) for i in range(len(LOSS_CONTRACT))],
            "sifsrq_valid_counts": [counts_case(i) for i in range(len(COUNTS_CONTRACT))]}


@pytest.mark.parametrize("idx", range(len(LOSS_CONTRACT)))
def test_memory_contract_sif_loss(L, idx):
    """losses3 and dsr written in full and nowhere else -- bit-identical and NaN-free under every poison of the outputs and of the
    workspace (no workspace byte is read before it is written; the NaNs of lst under the invalid cells reach nothing) --, the five
    const inputs untouched, nothing outside the buffers and the stated workspace bytes written, the same bits on ordinary
    allocations, and the result is the restatement's"""
    first = run_contract(L, CONTRACT["sifsrq_sif_loss"][idx], seed=731 + idx, capacity=64 << 20)
    shape, kind, mask, with_dsr = LOSS_CONTRACT[idx]
    _, _, _, _, _, ref_losses, ref_g = Q.loss_reference(shape, kind, ALPHA, GAMMA, mask or "all")
    for a, b in zip(first["losses3"].tolist(), ref_losses):
        assert abs(a - b) <= PARITY * abs(b)
    if with_dsr:
        assert float((first["dsr"].double().cpu() - ref_g).abs().max()) <= PARITY * float(ref_g.abs().max())


@pytest.mark.parametrize("idx", range(len(COUNTS_CONTRACT)))
def test_memory_contract_valid_counts(L, idx):
    first = run_contract(L, CONTRACT["sifsrq_valid_counts"][idx], seed=831 + idx, capacity=16 << 20)
    shape, mask = COUNTS_CONTRACT[idx]
    assert tuple(first["counts2"].tolist()) == Q.counts_ref(Q.loss_mask(shape, mask).numpy(), shape[0], shape[1])


def test_errors_launch_nothing(sifsr, L):
    N, E = sifsr.rloss, sifsr.SifsrError
    shape = (40, 56, 2.5)
    sr, lst, ndvi = (t.cuda() for t in Q.loss_inputs(shape))
    v = Q.loss_mask(shape, "blobs30").cuda()
    c = N.valid_counts(v, (40, 56))
    call = lambda **kw: N.sif_loss_with_grad("sr2", kw.get("sr", sr), kw.get("lst", lst), kw.get("ndvi", ndvi), kw.get("factor", 2.5), MEAN, STD,
                                             0.5, 1.0, valid=kw.get("valid", v), counts=kw.get("counts", c))
    for bad in (dict(sr=sr.cpu()), dict(lst=lst[:, :, :15].contiguous()), dict(counts=None), dict(valid=None), dict(factor=8.5), dict(factor=1.0),
                dict(sr=sr.double()), dict(valid=v.float()), dict(valid=v[:, :, :15]), dict(counts=c.int()), dict(counts=c.cpu()),
                dict(counts=torch.zeros(3, dtype=torch.int64, device="cuda")), dict(valid=v.cpu())):
        with pytest.raises(E):
            call(**bad)
    # the C entry points: every error returns before a launch
    lib = L.lib()
    H, W, f, B = 40, 56, 2.5, 2
    need = lib.sifsrq_sif_loss_workspace_bytes(2, B, H, W, f)
    hr, lr = torch.full((B, H, W), 77.0, device="cuda"), torch.full((B, 16, 22), 77.0, device="cuda")
    vv, cc = torch.full((B, 16, 22), 77, dtype=torch.uint8, device="cuda"), torch.full((4,), 77, dtype=torch.int64, device="cuda")
    out, dsr = torch.full((4,), 77.0, device="cuda"), torch.full((B, H, W), 77.0, device="cuda")
    ws = torch.full((need + 16,), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    args = lambda **kw: [kw.get("kind", 2), kw.get("sr", p(hr)), kw.get("lst", p(lr)), kw.get("valid", p(vv)), kw.get("counts", p(cc)),
                         kw.get("ndvi", p(hr)), kw.get("B", B), kw.get("H", H), kw.get("W", W), kw.get("factor", f), MEAN, STD, 0.5, 1.0,
                         kw.get("ws", p(ws)), kw.get("nbytes", need), kw.get("out", p(out)), kw.get("dsr", p(dsr)), S()]
    fn = lib.sifsrq_sif_loss
    for bad in (dict(H=3), dict(W=3), dict(H=16385), dict(factor=1.0), dict(factor=8.5), dict(factor=float("nan")), dict(B=0), dict(B=65536)):
        assert fn(*args(**bad)) == 1001, bad
    for bad in (dict(sr=None), dict(lst=None), dict(ndvi=None), dict(ws=None), dict(out=None), dict(valid=None), dict(counts=None), dict(kind=0),
                dict(ws=p(ws) + 8), dict(sr=p(hr) + 2), dict(lst=p(lr) + 1), dict(out=p(out) + 2), dict(dsr=p(dsr) + 1), dict(counts=p(cc) + 4)):
        assert fn(*args(**bad)) == 1002, bad
    for bad in (dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=need - 1, dsr=None), dict(nbytes=need - 1, valid=None, counts=None)):
        assert fn(*args(**bad)) == 1003, bad
    cfn = lib.sifsrq_valid_counts
    cargs = lambda **kw: [kw.get("valid", p(vv)), kw.get("B", B), kw.get("h", 16), kw.get("w", 22), H, W, kw.get("counts", p(cc)), S()]
    for bad, rc in ((dict(B=0), 1001), (dict(h=41), 1001), (dict(w=0), 1001), (dict(valid=None), 1002), (dict(counts=None), 1002),
                    (dict(counts=p(cc) + 4), 1002)):
        assert cfn(*cargs(**bad)) == rc, bad
    torch.cuda.synchronize()
    for t in (hr, lr, vv, cc, out, dsr, ws):
        assert (t == 77).all()
    # ... and a good call writes what it says and no more
    assert cfn(*cargs()) == 0 and fn(*args()) == 0
    torch.cuda.synchronize()
    assert cc.tolist() == [B * 16 * 22, B * H * W, 77, 77] and (hr == 77).all() and (lr == 77).all() and (vv == 77).all()
    assert (ws[need:] == 77).all() and (out[:3] != 77).all() and float(out[3]) == 77 and torch.isfinite(dsr).all() and (dsr != 77).all()
