"""GPU: training on partly valid patches (include/sifsr_masked.h) against the restatement
tests/masked_reference.py (held to the oracle by tests/test_masked_host.py) and against the unmasked entry points.

  * the memory contract of the two writing entry points in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is the
    table tests/test_capi_gate.py checks against the header); the loss workspace is poisoned scratch,
  * fill: N = 4 patches (all valid, none valid, one valid pixel, a hole with scattered zeros, a NaN and an inf) at w = 8, 20, 64,
    bit-equal to the restatement and to sifsrg_fill per patch, moments exact (M2 to 1e-12), a row of a batch = its N = 1 call,
  * loss: B = 2 at (40, 24), (64, 64), (100, 36) -- partial 32 x 32 tiles, a last row of tiles with partial LR blocks --, both
    kinds, three masks, within TOL = 1e-4 of the float64 restatement (the bar and the `rel_err` of tests/test_ops_gpu.py); an
    all-valid mask IS sifsr.sif_loss_with_grad, bit for bit; NaN in `lst` at invalid pixels changes no bit; n_valid = 0: zeros,
  * statistics over valid pixels, as a condition; the masked loader, the masked step, the masked graphed step."""

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import masked_reference as R
from tests.conftest import rel_err
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal

pytestmark = pytest.mark.gpu
TOL = 1e-4                                   # tests/test_ops_gpu.py: the bar of the unmasked fused loss
U8, I64, F64 = torch.uint8, torch.int64, torch.float64
WORKSPACE_ERR = 1003
MEAN, STD = R.MEAN, R.STD
KIND_ID = {"sr2": 2, "sr1": 1}


def dev(a):
    return (a.clone() if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).cuda()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def taps(sifsr):
    return sifsr.sif_ops._taps_c(0.1, 4, None), sifsr.sif_ops._taps_c(0.25, 4, None)


def count(valid):
    return torch.tensor(int((valid != 0).sum()), dtype=I64, device="cuda")


# ---- 1. memory contract --------------------------------------------------------------------------------------------------------
def fill_case(w):
    def make(k):
        lst = k.t("lst", torch.from_numpy(R.make_patches(w, seed=int(k.rs.randint(100)))))
        filled, valid, mom = k.o("filled", 4, w, w), k.o("valid", 4, w, w, dtype=U8), k.o("moments", 4, 5, dtype=F64)
        call = lambda: k.L.call("sifsrm_patches_fill", lst, filled, valid, mom, 4, w, S())
        # (+-inf are values of an empty patch's row, NaN is not)
        return call, {"filled": filled, "valid": valid, "moments": mom}
    return make


def loss_case(hw, kind, with_grad=True):
    def make(k):
        import sifsr
        H, W = hw
        sr, lst, ndvi = k.i("sr", R.B, 1, H, W, scale=1.3), k.i("lst", R.B, 1, H // 4, W // 4), k.i("ndvi", R.B, 1, H, W)
        v = (k.rs.uniform(size=(R.B, 1, H // 4, W // 4)) > 0.3).astype(np.uint8)
        valid, n = k.t("valid", torch.from_numpy(v)), k.t("n_valid", torch.tensor([int(v.sum())], dtype=I64))
        need = k.L.call("sifsrm_sif_loss_workspace_bytes", KIND_ID[kind], R.B, H, W)
        ws = k.A.scratch(need, "workspace")                       # poisoned scratch: nothing of it may reach the outputs
        losses, dsr = k.o("losses3", 3), (k.o("dsr", R.B, 1, H, W) if with_grad else None)
        t1, t2 = taps(sifsr)
        call = lambda: k.L.call("sifsrm_sif_loss", KIND_ID[kind], sr, lst, valid, n, ndvi, R.B, H, W, MEAN, STD, 0.5, -0.25, t1, t2, ws,
                                need, losses, dsr, S())
        return call, ({"losses3": losses, "dsr": dsr} if with_grad else {"losses3": losses})
    return make


CONTRACT = {"sifsrm_patches_fill": [fill_case(w) for w in (4, 8, 20, 64)],
            "sifsrm_sif_loss": [loss_case(hw, kind) for hw in R.SHAPES for kind in ("sr2", "sr1")] + [loss_case((40, 24), "sr2", False)]}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output written in full and nowhere else -- NaN-free under the NaN poison, bit-identical under every poison (the
    poisoned loss workspace included) --, const inputs untouched, and the same bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=64 << 20)


def test_workspace_too_small(sifsr, L):
    sr, lst, ndvi = (dev(t) for t in R.loss_inputs((40, 24)))
    valid = torch.ones((2, 1, 10, 6), dtype=U8, device="cuda")
    need = L.call("sifsrm_sif_loss_workspace_bytes", 2, 2, 40, 24)
    ws = torch.full((need,), 77, dtype=U8, device="cuda")
    losses, dsr = torch.full((3,), 77.0, device="cuda"), torch.full((2, 1, 40, 24), 77.0, device="cuda")
    t1, t2 = taps(sifsr)
    p = lambda t: t.data_ptr()
    args = lambda nbytes: (2, p(sr), p(lst), p(valid), p(count(valid)), p(ndvi), 2, 40, 24, MEAN, STD, 0.5, -0.25, t1, t2, p(ws), nbytes,
                           p(losses), p(dsr), S())
    fn = L.lib().sifsrm_sif_loss
    assert fn(*args(need - 1)) == WORKSPACE_ERR and fn(*args(0)) == WORKSPACE_ERR
    torch.cuda.synchronize()
    assert (ws == 77).all() and (losses == 77).all() and (dsr == 77).all()
    n = count(valid)
    assert fn(2, p(sr), p(lst), p(valid), p(n), p(ndvi), 2, 40, 24, MEAN, STD, 0.5, -0.25, t1, t2, p(ws), need, p(losses), p(dsr), S()) == 0
    torch.cuda.synchronize()
    assert not (losses == 77).any() and not (dsr == 77).any()


# ---- 2. fill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 20, 64])
def test_fill_patches(sifsr, w):
    p = R.make_patches(w)
    want_f, want_v, want_m = R.fill_patches_ref(p)
    filled, valid, mom = sifsr.products.fill_patches(dev(p))
    assert filled.dtype == torch.float32 and valid.dtype == U8 and mom.dtype == F64
    assert tuple(filled.shape) == tuple(valid.shape) == (4, w, w) and tuple(mom.shape) == (4, 5)
    assert np.array_equal(valid.cpu().numpy(), want_v) and np.array_equal(bits(filled), bits(want_f))
    got = mom.cpu().numpy()
    for c, what in ((0, "count"), (1, "mean"), (3, "min"), (4, "max")):
        assert np.array_equal(got[:, c], want_m[:, c]), what
    m2 = np.abs(got[:, 2] - want_m[:, 2]) / np.maximum(np.abs(want_m[:, 2]), 1e-300)
    print(f"w {w}: M2 relative error per patch {m2}")
    assert (got[[1, 2], 2] == 0).all() and (m2 <= 1e-12).all()
    for n in range(4):
        # ... and the whole-raster fill of the gap-aware prediction, per patch, on the device
        f1, v1 = sifsr.gaps.fill_gaps(dev(p[n]))
        assert bit_equal(f1, filled[n]) and bit_equal(v1, valid[n])
        # row n of the batch is its own N = 1 call; the (N,1,w,w) layout is the same call
        fs, vs, ms = sifsr.products.fill_patches(dev(p[n:n + 1])[:, None])
        assert tuple(fs.shape) == (1, 1, w, w)
        assert bit_equal(fs[0, 0], filled[n]) and bit_equal(vs[0, 0], valid[n]) and np.array_equal(bits(ms[0]), bits(mom[n]))


def test_fill_errors(sifsr):
    E = sifsr.SifsrError
    for shape in ((2, 1, 6, 6), (2, 1, 68, 68), (2, 2, 8, 8), (2, 8, 12), (8, 8)):
        with pytest.raises(E):
            sifsr.products.fill_patches(torch.zeros(shape, device="cuda"))
    with pytest.raises(E):
        sifsr.products.fill_patches(torch.zeros((2, 8, 8), device="cuda", dtype=F64))


# ---- 3. loss -------------------------------------------------------------------------------------------------------------------
def run_loss(sifsr, kind, sr, lst, valid, n, ndvi, alpha, gamma):
    out = sifsr.masked_sif_loss_with_grad(kind, dev(sr), dev(lst), dev(valid), n, dev(ndvi), MEAN, STD, alpha, gamma)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("kind,alpha,gamma", R.KINDS)
def test_masked_loss_vs_restatement(sifsr, kind, alpha, gamma, hw, mask):
    sr, lst, ndvi, valid, n, want, g_ref = R.loss_reference(hw, kind, alpha, gamma, mask)
    planted = lst.clone()
    planted[valid == 0] = float("nan")
    ds, pl, loss, dsr = run_loss(sifsr, kind, sr, lst, valid, count(valid), ndvi, alpha, gamma)
    for got, ref, what in zip((ds, pl, loss), want, ("ds", "pl", "loss")):
        print(f"{kind} {hw} {mask} {what}: {float(got):.9g} vs {ref:.9g}, rel {abs(float(got) - ref) / abs(ref):.2e}")
    err = rel_err(dsr, g_ref)
    print(f"{kind} {hw} {mask} dsr: rel_err {err:.2e}")
    for got, ref in zip((ds, pl, loss), want):
        assert abs(float(got) - ref) < TOL * abs(ref)
    assert err < TOL
    if mask != "random30":
        assert (dsr[0] == 0).all() and (dsr[1] != 0).any()               # a whole invalid image: EXACTLY zero there
    # NaN in lst at the invalid pixels changes no bit of any output
    again = run_loss(sifsr, kind, sr, planted, valid, count(valid), ndvi, alpha, gamma)
    for a, b in zip((ds, pl, loss, dsr), again):
        assert bit_equal(a, b)
    # the autograd form is the same call
    srd = dev(sr).requires_grad_(True)
    out = sifsr.masked_sif_loss(kind, srd, dev(planted), dev(valid), count(valid), dev(ndvi), MEAN, STD, alpha, gamma)
    (g,) = torch.autograd.grad(out[2], srd)
    assert bit_equal(g, dsr) and all(bit_equal(a.detach(), b) for a, b in zip(out, (ds, pl, loss)))


@pytest.mark.parametrize("hw", R.SHAPES + [(256, 256)])
@pytest.mark.parametrize("kind,alpha,gamma", R.KINDS)
def test_all_valid_is_the_unmasked_loss_bit_for_bit(sifsr, kind, alpha, gamma, hw):
    if hw == (256, 256):
        lst, lst_up, ndvi = O.synthetic_batch(4, 2)                   # the training shape: 8 x 8 full tiles per image
        sr = (lst_up + 0.8 * ndvi.flip(-1)).contiguous()
    else:
        sr, lst, ndvi = R.loss_inputs(hw)
    want = sifsr.sif_loss_with_grad(kind, dev(sr), dev(lst), dev(ndvi), MEAN, STD, alpha, gamma)
    for fill in (1, 255):
        valid = torch.full(lst.shape, fill, dtype=U8)
        got = run_loss(sifsr, kind, sr, lst, valid, count(valid), ndvi, alpha, gamma)
        for a, b, what in zip(got, want, ("ds", "pl", "loss", "dsr")):
            assert bit_equal(a, b), what
    # ... and without a gradient (the evaluation path): the losses of the unmasked evaluation path
    with torch.no_grad():
        a = sifsr.masked_sif_loss(kind, dev(sr), dev(lst), dev(valid), count(valid), dev(ndvi), MEAN, STD, alpha, gamma)
        b = sifsr.sif_loss(kind, dev(sr), dev(lst), dev(ndvi), MEAN, STD, alpha, gamma)
    assert all(bit_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["sr2", "sr1"])
def test_no_valid_pixel_gives_zeros(sifsr, kind):
    sr, lst, ndvi = R.loss_inputs((100, 36))
    lst = torch.full_like(lst, float("nan"))
    valid = torch.zeros(lst.shape, dtype=U8)
    ds, pl, loss, dsr = run_loss(sifsr, kind, sr, lst, valid, count(valid), ndvi, 0.5, -0.25)
    assert float(ds) == float(pl) == float(loss) == 0.0 and (dsr == 0).all()
    with torch.no_grad():
        out = sifsr.masked_sif_loss(kind, dev(sr), dev(lst), dev(valid).bool(), 0, dev(ndvi), MEAN, STD, 0.5, -0.25)
    assert all(float(o) == 0.0 for o in out)


def test_loss_errors(sifsr):
    sr, lst, ndvi = (dev(t) for t in R.loss_inputs((40, 24)))
    valid = torch.ones(lst.shape, dtype=U8, device="cuda")
    n = count(valid)
    E = sifsr.SifsrError
    bad = [dict(valid=valid.float()), dict(valid=valid[:, :, :5]), dict(valid=valid.cpu()), dict(n_valid=n.to(torch.int32)),
           dict(n_valid=n.cpu()), dict(n_valid=torch.stack([n, n])), dict(lst=lst[:, :, :5].contiguous()), dict(sr=sr.cpu())]
    for kw in bad:
        a = dict(sr=sr, lst=lst, valid=valid, n_valid=n, ndvi=ndvi)
        a.update(kw)
        with pytest.raises(E):
            sifsr.masked_sif_loss_with_grad("sr2", a["sr"], a["lst"], a["valid"], a["n_valid"], a["ndvi"], MEAN, STD, 0.5, -0.25)
    # (B,H/4,W/4) and bool are the same mask
    a = sifsr.masked_sif_loss_with_grad("sr2", sr, lst, valid, n, ndvi, MEAN, STD, 0.5, -0.25)
    b = sifsr.masked_sif_loss_with_grad("sr2", sr, lst, valid[:, 0].bool(), n, ndvi, MEAN, STD, 0.5, -0.25)
    assert all(bit_equal(x, y) for x, y in zip(a, b))


# ---- 4. statistics, as a condition ---------------------------------------------------------------------------------------------
def mined_with_holes(sifsr, n=6, w=16, seed=0):
    """n patches of w x w LST pixels in [290, 310] K with exactly 10 % zeros and NDVI in [-1, 1], as a MinedPatches on the device"""
    lst = R.holes_10_percent(n, w, seed)
    ndvi = np.clip(np.random.RandomState(seed + 1).standard_normal((n, 1, 4 * w, 4 * w)) * 0.3 + 0.4, -1, 1).astype(np.float32)
    index = np.stack([np.zeros(n), np.arange(n), np.zeros(n), np.zeros(n)], 1).astype(np.int64)
    return sifsr.products.MinedPatches(dev(lst), dev(ndvi), index, R.gather_moments(lst, ndvi), w), lst, ndvi


def test_statistics_over_valid_pixels(sifsr):
    mined, lst, _ = mined_with_holes(sifsr, n=10, w=20)
    plain = mined.statistics(None)
    assert plain["mini"] == 0 and plain["mean_lst"] < 290            # the harm: at most 0.9 * 310 = 279 by construction
    st = mined.statistics(None, valid_only=True)
    v = lst[lst != 0].astype(np.float64)
    print(f"mean_lst {plain['mean_lst']:.3f} -> {st['mean_lst']:.3f}, std_lst {plain['std_lst']:.3f} -> {st['std_lst']:.3f}")
    assert st["mini"] >= 290 and st["mini"] == v.min() and st["maxi"] == v.max()
    assert abs(st["mean_lst"] - v.mean()) <= 1e-12 * v.mean()
    assert abs(st["std_lst"] - v.std()) <= 1e-9 * v.std()
    assert (st["mean_ndvi"], st["std_ndvi"]) == (plain["mean_ndvi"], plain["std_ndvi"])
    assert mined.fill() is mined and mined.valid_moments.shape == (10, 5) and mined.valid_moments[:, 0].sum() == v.size
    f = mined.filled
    assert mined.fill().filled is f                                   # computed once
    mined.assign_split()
    tr = mined.statistics("Train", valid_only=True)
    vt = lst[mined.rows("Train")]
    assert abs(tr["mean_lst"] - vt[vt != 0].astype(np.float64).mean()) <= 1e-12 * tr["mean_lst"]


# ---- 5. loader and step --------------------------------------------------------------------------------------------------------
def small_model(sifsr, seed=3):
    m = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1)
    m.load_state_dict(O.synthetic_state(seed), strict=True)
    return m.cuda()


@pytest.fixture(scope="module")
def batch(sifsr):
    """one masked loader batch: HR 64 x 64, B = 2"""
    mined, lst, ndvi = mined_with_holes(sifsr, n=10, w=16, seed=5)
    stats = mined.statistics(None, valid_only=True)
    loader = mined.masked_loader(None, 2, stats, shuffle=False)
    batches = list(loader)
    return mined, lst, ndvi, stats, batches


def test_masked_loader_is_prepare_tiles_on_the_filled_patches(sifsr, batch):
    mined, lst, ndvi, stats, batches = batch
    assert len(batches) == 5 and all(len(b) == 5 for b in batches)
    want_f, want_v, want_m = R.fill_patches_ref(lst[:, 0])
    for i, (l, up, nd, valid, n) in enumerate(batches[:2]):
        rows = slice(2 * i, 2 * i + 2)
        ln = (dev(want_f[rows])[:, None] - float(stats["mean_lst"])) / float(stats["std_lst"])
        nn = (dev(ndvi[rows]) - float(stats["mean_ndvi"])) / float(stats["std_ndvi"])
        x = sifsr.pipeline.prepare_tiles(ln, nn)
        assert bit_equal(l, ln) and bit_equal(up, x[:, 0:1].contiguous()) and bit_equal(nd, nn)
        assert valid.dtype == U8 and np.array_equal(valid.cpu().numpy()[:, 0], want_v[rows])
        assert n.dtype == I64 and n.dim() == 0 and n.is_cuda and int(n) == int(want_m[rows, 0].sum()) < 2 * 256
        assert not torch.isnan(up).any() and float(l.abs().max()) < 10          # no -55 sigma pixel reaches the network
    # the unmasked loader is what it was: three items, the raw patch
    l3 = next(iter(mined.loader(None, 2, stats, shuffle=False)))
    assert len(l3) == 3 and float(l3[0].min()) < -40
    # the dataset form: five items, a (b,) count vector after the default collate
    from torch.utils.data import DataLoader
    ds = sifsr.MinedDataset(mined, None, stats, masked=True)
    a, b, c, v, cnt = next(iter(DataLoader(ds, batch_size=2)))
    assert a.shape == (2, 1, 16, 16) and b.shape == c.shape == (2, 1, 64, 64) and v.shape == (2, 1, 16, 16) and v.dtype == U8
    assert cnt.dtype == I64 and cnt.tolist() == want_m[:2, 0].astype(np.int64).tolist()
    assert np.allclose(a.numpy(), batches[0][0].cpu().numpy(), rtol=1e-6, atol=1e-6) and np.array_equal(v.numpy(), batches[0][3].cpu().numpy())
    assert sifsr.MinedDataset(mined, None, masked=True).stats == mined.statistics("Train", valid_only=True)
    assert len(sifsr.MinedDataset(mined, None)[0]) == 3


def test_masked_train_step(sifsr, batch):
    _, _, _, stats, batches = batch
    lst, lst_up, ndvi, valid, n = batches[0]
    m = small_model(sifsr)
    opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
    before = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()
    ds, pl, loss, sr = sifsr.train.train_step(m, opt, lst, lst_up, ndvi, stats, 0.5, -0.25, "sr2", return_sr=True, valid=valid, n_valid=n)
    torch.cuda.synchronize()
    want = R.masked_loss_ref("sr2", sr.cpu(), lst.cpu(), valid.cpu(), ndvi.cpu(), stats["mean_lst"], stats["std_lst"], 0.5, -0.25)
    for got, ref, what in zip((ds, pl, loss), want, ("ds", "pl", "loss")):
        print(f"masked step {what}: {float(got):.9g} vs {float(ref):.9g}")
        assert abs(float(got) - float(ref)) < TOL * abs(float(ref))
    after = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    # evaluation: the masked loss of the eval-mode prediction, finite
    ev = sifsr.train.eval_step(m, lst, lst_up, ndvi, stats, 0.5, -0.25, "sr2", valid=valid, n_valid=n)
    assert all(torch.isfinite(e) for e in ev)
    # an epoch of one batch with a (b,) count vector, as the default collate of the masked dataset gives it: the same loss
    out = sifsr.train.eval_epoch(m, [(lst.cpu(), lst_up.cpu(), ndvi.cpu(), valid.cpu(), torch.tensor([200, int(n) - 200]))], stats, 0.5, -0.25)
    assert np.isfinite(out).all() and abs(out[2] - float(ev[2])) <= 1e-6 * abs(out[2])
    # a training epoch over masked batches: five finite numbers
    out = sifsr.train.train_epoch(m, batches[:2], opt, stats, 0.5, -0.25, "sr2")
    assert len(out) == 5 and np.isfinite(out).all()


def test_all_valid_step_is_the_unmasked_step(sifsr, batch):
    _, _, _, stats, batches = batch
    lst, lst_up, ndvi, valid, _ = batches[1]
    ones = torch.ones_like(valid)
    res = []
    for masked in (False, True):
        m = small_model(sifsr)
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
        kw = dict(valid=ones, n_valid=count(ones)) if masked else {}
        out = sifsr.train.train_step(m, opt, lst, lst_up, ndvi, stats, 0.5, -0.25, "sr2", **kw)
        torch.cuda.synchronize()
        res.append((out, torch.cat([p.detach().reshape(-1) for p in m.parameters()])))
    for a, b in zip(res[0][0], res[1][0]):
        assert bit_equal(a.detach(), b.detach())
    assert bit_equal(res[0][1], res[1][1])


def test_masked_graphed_train_step_matches_eager(sifsr):
    """train.GraphedTrainStep(masked=True) as tests/test_model_gpu.test_graphed_train_step_matches_eager checks the unmasked one: 3
    eager warm-up calls, capture on the 4th, replays after -- each batch with ANOTHER mask and count through the same graph."""
    stats = {"mean_lst": MEAN, "std_lst": STD}
    Bn, lr, hr = 2, 1e-3, 64
    batches = []
    for i in range(7):
        lst, lst_up, ndvi = (t.cuda() for t in O.synthetic_batch(60 + i, Bn, hr))
        valid = (torch.rand((Bn, 1, hr // 4, hr // 4), generator=torch.Generator().manual_seed(i)) > 0.1 * i).to(U8).cuda()
        batches.append((lst, lst_up, ndvi, valid, count(valid)))
    assert len({int(b[4]) for b in batches}) == 7

    def run(graphed):
        torch.manual_seed(5)
        m = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda()
        opt = sifsr.FlatAdam(m.parameters(), lr=lr, capturable=graphed)
        stepper = sifsr.train.GraphedTrainStep(m, opt, Bn, stats, 0.5, -0.25, "sr2", hr=hr, masked=True) if graphed else None
        losses = []
        for lst, lst_up, ndvi, valid, n in batches:
            out = stepper(lst, lst_up, ndvi, valid, n) if graphed else \
                sifsr.train.train_step(m, opt, lst, lst_up, ndvi, stats, 0.5, -0.25, "sr2", valid=valid, n_valid=n)
            losses.append(float(out[2].detach()))
        torch.cuda.synchronize()
        if graphed:
            assert stepper.graph is not None and opt.state_dict()["flat"]["step"] == len(batches)
            with pytest.raises(ValueError):
                stepper(lst, lst_up, ndvi)
        return losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()

    l_e, p_e = run(False)
    l_g, p_g = run(True)
    print(f"eager {l_e}\ngraph {l_g}")
    assert np.allclose(l_g, l_e, rtol=1e-5)
    assert (p_g - p_e).abs().max().item() <= 1e-6          # device pow() vs host pow() in the bias correction: <= 1 ulp of lr
