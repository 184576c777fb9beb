"""GPU: the captured step and the captured granule predictors at any ratio against the eager calls they replay.

Every comparison is for EQUAL BITS: the eval forward is per image, the kernels are deterministic, and a captured chain enqueues the
launches of the eager one (plus, in the gap-aware predictor, the forwards of the slots nobody reads).  There is no tolerance in this
file and no float64 oracle: the eager calls are held to theirs in tests/test_ratio_gpu.py, test_rloss_gpu.py, test_gaps_gpu.py and
test_adapt_gpu.py.

  * ratio.GranulePredictor without gaps = ratio.predict_granule, with conserve=k too, over replays with other rasters;
  * GranulePredictor(gaps=True), at three ratios and at x4 = predict_granule_gaps, fill_value pixels included, over ONE object and
    a sequence of masks chosen for stale slots: fewer active tiles after more, more after fewer, no valid pixel at all, then a
    full raster with mask=None; n_active stays on the device;
  * rloss.GraphedTrainStep = the rloss.train_step loop from clones of one model and one FlatAdam(capturable=True): three losses per
    step and the flat parameter vector after every step, through the eager warm-up, the capture call and the replays -- unmasked and
    masked, sr2 and sr1, frozen and batch statistics, a mask that changes between replays, an image without a valid cell, counts
    given ((2,) and (b,2)) and formed inside, alternating through one graph;
  * adapt_granule(graphed=True) = the eager loop with an optimizer of the same construction, at x4 and at a ratio; restore();
  * train_epoch(graphed=step) = the eager epoch's five means, with short batches in the loader;
  * a replaying call of every new object reads nothing back (torch.cuda.set_sync_debug_mode("error")); the eager
    predict_granule_gaps is the positive control and must trip.

Shapes: the smallest with every moving part -- pairs (8, 24), (16, 40), (12, 24) and the x4 pair (8, 32); batches of 2 - 4; granules
of 12 - 15 tiles with overlap > 0 and cover_edges (tile origins are no multiples of the window) and a batch that does not divide the
tile count (padded slots exist)."""
import copy

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import adapt_reference as A
from tests.contract import sifsr  # noqa: F401  (the fixture)
from tests.memcheck import bit_equal
from tests.test_model_gpu import make_model

pytestmark = pytest.mark.gpu
STATS = A.STATS
ALPHA, GAMMA, LR = 0.5, -0.25, 1e-3
U8 = torch.uint8
# (window, hr, (h, w) of the LST granule, overlap, batch): ratio.geometry accepts each; T = 15, 12, 15, 15 tiles
LAYOUTS = {"x3": (8, 24, (20, 28), 2, 4), "x2.5": (16, 40, (36, 50), 2, 5), "x2": (12, 24, (30, 40), 3, 4), "x4": (8, 32, (20, 28), 2, 4)}


@pytest.fixture(scope="module")
def model(sifsr):
    return make_model(sifsr, O.synthetic_state(3)).eval()


def granule(seed, window, hr, shape):
    """-> (lst (h,w) [K] without a gap, ndvi (h hr / window, w hr / window)) on the device"""
    rs = np.random.RandomState(seed)
    h, w = shape
    lst = rs.uniform(290.0, 325.0, (h, w)).astype(np.float32)
    ndvi = np.clip(0.4 + 0.3 * rs.standard_normal((h * hr // window, w * hr // window)), -1.2, 1.2).astype(np.float32)
    return torch.from_numpy(lst).cuda(), torch.from_numpy(ndvi).cuda()


def mask_sequence(shape, window):
    """-> [(name, lst edit, mask or None)]: the replays of one predictor.  "mid": the block of tile (0, 0) and a sprinkle; "few": only
    a corner block is kept; "more": one cloud; "none": nothing valid; "full": no gap, no mask."""
    h, w = shape
    rs = np.random.RandomState(h * w)
    ones = np.ones((h, w), np.uint8)
    mid = ones.copy(); mid[:window, :window] = 0; mid[rs.uniform(size=(h, w)) < 0.05] = 0
    few = np.zeros((h, w), np.uint8); few[h - window // 2:, w - window:] = 1
    more = ones.copy(); more[h // 2 - 2:h // 2 + 3, 3:9] = 0
    return [("mid", "sprinkle", mid), ("few", None, few), ("more", "sprinkle", more), ("none", None, np.zeros((h, w), np.uint8)),
            ("full", None, None), ("few again", None, few)]


def sprinkle(lst):
    """gaps in the raster itself: 0 K, NaN and inf pixels"""
    lst = lst.clone()
    lst[1, 2] = 0.0; lst[5, 7] = float("nan"); lst[-2, -3] = float("inf"); lst[3:5, 10:13] = 0.0
    return lst


# ---- 1. the predictors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,conserve", [("x3", 0), ("x3", 2), ("x2.5", 1), ("x2", 0)])
def test_ratio_predictor_without_gaps_is_predict_granule(sifsr, model, name, conserve):
    window, hr, shape, overlap, batch = LAYOUTS[name]
    kw = dict(window=window, hr=hr, batch=batch, overlap=overlap, cover_edges=True)
    gp = sifsr.ratio.GranulePredictor(model, shape, STATS, conserve=conserve, **kw)
    n = gp.tiles[0] * gp.tiles[1]
    assert n % gp.batch != 0 and gp.x.shape[0] > n and gp.graph is not None                            # padded slots exist
    outs = []
    for seed in (1, 2, 1):
        lst, ndvi = granule(seed, window, hr, shape)
        got = gp(lst, ndvi)
        want = sifsr.ratio.predict_granule(model, lst, ndvi, STATS, conserve=conserve, **kw)
        assert got.data_ptr() != gp.out.data_ptr() and bit_equal(got, want) and torch.isfinite(got).all()
        outs.append(got)
    assert bit_equal(outs[0], outs[2]) and not bit_equal(outs[0], outs[1])
    if conserve:
        assert not bit_equal(outs[0], sifsr.ratio.predict_granule(model, *granule(1, window, hr, shape), STATS, **kw))
    with pytest.raises(ValueError):
        gp(lst[:-1], ndvi)
    with pytest.raises(ValueError):
        gp(lst, ndvi, mask=torch.ones(shape, dtype=U8, device="cuda"))                                # a mask goes with gaps=True


@pytest.mark.parametrize("name,conserve,fill_value", [("x3", 0, float("nan")), ("x2.5", 1, -9999.0), ("x2", 0, float("nan")),
                                                      ("x4", 1, float("nan")), ("x4", 0, 0.0)])
def test_gap_aware_predictor_over_changing_masks(sifsr, model, name, conserve, fill_value):
    """one object, six replays; the stale slots of an earlier replay reach nothing"""
    window, hr, shape, overlap, batch = LAYOUTS[name]
    kw = dict(window=window, batch=batch, overlap=overlap, cover_edges=True)
    if name == "x4":
        gp = sifsr.predict.GranulePredictor(model, shape, STATS, conserve=conserve, gaps=True, fill_value=fill_value, **kw)
        eager = lambda *a, **k: sifsr.predict.predict_granule_gaps(*a, **kw, **k)
    else:
        gp = sifsr.ratio.GranulePredictor(model, shape, STATS, hr=hr, conserve=conserve, gaps=True, fill_value=fill_value, **kw)
        eager = lambda *a, **k: sifsr.ratio.predict_granule_gaps(*a, hr=hr, **kw, **k)
    n = gp.tiles[0] * gp.tiles[1]
    assert n % gp.batch != 0 and gp.x.shape[0] > n and not gp.x.any()                                  # zero-initialised, padded
    lst0, ndvi = granule(7, window, hr, shape)
    counts = {}
    for step, (what, edit, mask) in enumerate(mask_sequence(shape, window)):
        lst = sprinkle(lst0) if edit else lst0
        m = None if mask is None else torch.from_numpy(mask).cuda()
        got, info = gp(lst, ndvi, mask=m, return_info=True)
        want, winfo = eager(model, lst, ndvi, STATS, mask=m, fill_value=fill_value, return_info=True, conserve=conserve)
        assert isinstance(info["n_active"], torch.Tensor) and info["n_active"].is_cuda and info["n_active"].dtype == torch.int32
        counts[what] = int(info["n_active"])
        assert counts[what] == winfo["n_active"] and info["n_tiles"] == winfo["n_tiles"] == n
        assert info["valid"].dtype == torch.bool and torch.equal(info["valid"], winfo["valid"])
        assert bit_equal(got, want), (what, step)
        up = sifsr.rproducts.expand_valid(info["valid"][None, None], got.shape)[0, 0].bool()
        assert torch.isfinite(got[up]).all() and (got[up] != fill_value).all()
        assert (torch.isnan(got[~up]) if fill_value != fill_value else got[~up] == fill_value).all()     # (the bits are in `want`)
    print(f"{name}: active tiles {counts} of {n}")
    assert 0 == counts["none"] < counts["few"] == counts["few again"] < counts["mid"] < counts["more"] <= counts["full"] == n
    # a bool mask, and a gappy raster with mask=None (the static mask then holds all ones)
    lst = sprinkle(lst0)
    assert bit_equal(gp(lst, ndvi), eager(model, lst, ndvi, STATS, fill_value=fill_value, conserve=conserve))
    mb = torch.from_numpy(mask_sequence(shape, window)[0][2] != 0).cuda()
    assert bit_equal(gp(lst, ndvi, mask=mb), eager(model, lst, ndvi, STATS, mask=mb, fill_value=fill_value, conserve=conserve))
    for bad in (lambda: gp(lst[:-1], ndvi), lambda: gp(lst, ndvi[:, :-1])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(sifsr.SifsrError):
        gp(lst, ndvi, mask=torch.ones(shape, device="cuda"))                                          # a float mask


# ---- 2. the training step --------------------------------------------------------------------------------------------------------
def step_batches(window, hr, B, masked, n_steps=8, seed=80):
    """-> [(lst, lst_up, ndvi, valid or None)] on the device; with masks: another one per step, all ones at step 1, and at step 5
    (a replay) image 0 without a valid cell"""
    out = []
    for i in range(n_steps):
        x, _, _ = A.network_inputs(seed + i, B, hr, hr)
        rs = np.random.RandomState(seed + 100 + i)
        lst = torch.from_numpy(rs.standard_normal((B, 1, window, window)).astype(np.float32))
        valid = None
        if masked:
            v = (rs.uniform(size=(B, 1, window, window)) > 0.08 * i).astype(np.uint8)
            if i == 1:
                v[:] = 1
            if i == 5:
                v[0] = 0
            assert v[1].any()
            valid = torch.from_numpy(v).cuda()
        out.append((lst.cuda(), x[:, 0:1].contiguous().cuda(), x[:, 1:2].contiguous().cuda(), valid))
    return out


def counts_for(sifsr, valid, hr, form):
    """the counts argument of step i in its three forms: None, the (2,) tensor, the (b,2) rows of a loader"""
    if form == "formed":
        return None
    rows = torch.stack([sifsr.rloss.valid_counts(valid[b:b + 1], (hr, hr)) for b in range(valid.shape[0])])
    return rows if form == "rows" else rows.sum(0)


STEP_CASES = [("x3", 3, False, "sr2", False, None), ("x3", 2, False, "sr1", True, None), ("x2.5", 2, True, "sr1", False, ("formed",)),
              ("x2", 4, True, "sr2", True, ("given", "rows")), ("x4", 2, True, "sr2", False, ("given", "formed", "rows")),
              ("x3", 3, True, "sr2", True, ("formed", "given"))]


@pytest.mark.parametrize("name,B,masked,kind,frozen,forms", STEP_CASES, ids=lambda v: str(v))
def test_graphed_train_step_is_the_eager_loop(sifsr, name, B, masked, kind, frozen, forms):
    window, hr = LAYOUTS[name][:2]
    batches = step_batches(window, hr, B, masked)
    sd = O.synthetic_state(71)

    def run(graphed):
        m = make_model(sifsr, copy.deepcopy(sd)).train()
        m.bn_frozen = frozen
        opt = sifsr.FlatAdam(m.parameters(), lr=LR, capturable=True)
        step = sifsr.rloss.GraphedTrainStep(m, opt, B, STATS, ALPHA, GAMMA, window, hr, kind=kind, masked=masked, return_sr=True) if graphed else None
        losses, params, srs = [], [], []
        for i, (lst, up, ndvi, valid) in enumerate(batches):
            c = counts_for(sifsr, valid, hr, forms[i % len(forms)]) if masked else None
            if graphed:
                out = step(lst, up, ndvi, valid, c) if masked else step(lst, up, ndvi)
            else:
                out = sifsr.rloss.train_step(m, opt, lst, up, ndvi, STATS, ALPHA, GAMMA, hr / window, kind=kind, valid=valid,
                                             counts=None if c is None else (c.sum(0) if c.dim() == 2 else c), return_sr=True)
            assert len(out) == 4 and not any(t.requires_grad for t in out)
            losses.append(torch.stack(out[:3]).clone()); srs.append(out[3].clone()); params.append(m.flat_parameters().detach().clone())
        torch.cuda.synchronize()
        if graphed:
            assert step.graph is not None and step.bn_frozen is frozen and opt.state_dict()["flat"]["step"] == len(batches)
            m.bn_frozen = not frozen                                                                   # the mode of every replay is the captured one
            with pytest.raises(ValueError, match="bn_frozen"):
                step(*batches[0][:3], *((batches[0][3],) if masked else ()))
            m.bn_frozen = frozen
            with pytest.raises(ValueError):
                step(*batches[0][:3], *(() if masked else (torch.ones((B, 1, window, window), dtype=U8, device="cuda"),)))
            assert torch.equal(m.flat_parameters(), params[-1])                                        # a refused call changed nothing
        return torch.stack(losses), torch.stack(params), srs, m

    le, pe, se, me = run(False)
    lg, pg, sg, mg = run(True)
    print(f"{name} {kind} masked={masked} frozen={frozen}: loss per step, eager {le[:, 2].tolist()}\n{'':>40}replay {lg[:, 2].tolist()}")
    assert torch.isfinite(le).all() and not torch.equal(pe[0], pe[-1]) and len({float(v) for v in le[:, 2]}) == len(batches)
    for i in range(len(batches)):
        assert bit_equal(lg[i], le[i]), ("losses", i)
        assert bit_equal(sg[i], se[i]), ("sr", i)
        assert torch.equal(pg[i], pe[i]), ("parameters", i)
    for (k, a), b in zip(mg.state_dict().items(), me.state_dict().values()):                           # BatchNorm buffers too
        assert torch.equal(a, b), k
    if frozen:
        assert all(torch.equal(v.cpu(), sd[k]) for k, v in mg.state_dict().items() if "running" in k)


# ---- 3. adaptation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,hr,batch", [(8, 32, 16), (8, 24, 16), (16, 40, 5)])
def test_adapt_granule_graphed_is_the_eager_loop(sifsr, window, hr, batch):
    from tests.test_rloss_gpu import GRANULE, ratio_granule
    lst, ndvi = (torch.from_numpy(a).cuda() for a in ratio_granule(window, hr))
    steps = 7
    sd = O.synthetic_state(37)

    def adapt(m, **kw):
        kw = dict(dict(steps=steps, lr=LR, alpha=ALPHA, gamma=GAMMA, kind="sr2", batch=batch, overlap=2, cover_edges=True), **kw)
        if hr == 4 * window:
            return sifsr.adapt.adapt_granule(m, lst, ndvi, STATS, window=window, **kw)
        return sifsr.rloss.adapt_granule(m, lst, ndvi, STATS, window, hr, **kw)

    def run(graphed):
        m = make_model(sifsr, copy.deepcopy(sd)).eval()
        p0 = m.flat_parameters().detach().clone()
        # the eager loop takes an optimizer of the construction the graphed loop makes for itself
        res = adapt(m, graphed=True) if graphed else adapt(m, optimizer=sifsr.FlatAdam(m.parameters(), lr=LR, capturable=True))
        assert not m.training and m.bn_frozen is False and res.optimizer.capturable
        return m, p0, res

    me, p0, re_ = run(False)
    mg, _, rg = run(True)
    n = rg.n_active
    assert n == re_.n_active and batch < n < steps * batch and tuple(rg.losses.shape) == (steps, 3)      # seven steps wrap the active list
    print(f"({window},{hr}) on {GRANULE}: {n} active tiles; loss per step {rg.losses[:, 2].tolist()}")
    assert bit_equal(rg.losses, re_.losses) and torch.isfinite(rg.losses).all()
    assert torch.equal(mg.flat_parameters(), me.flat_parameters()) and not torch.equal(mg.flat_parameters(), p0)
    assert torch.equal(rg.optimizer._m, re_.optimizer._m) and torch.equal(rg.optimizer._v, re_.optimizer._v)
    assert rg.optimizer.state_dict()["flat"]["step"] == steps
    for (k, a), b in zip(mg.state_dict().items(), me.state_dict().values()):
        assert torch.equal(a, b), k
    rg.restore()
    assert torch.equal(mg.flat_parameters(), p0)
    # fewer than four steps: nothing is captured, and that is fine
    m3 = make_model(sifsr, copy.deepcopy(sd)).eval()
    assert bit_equal(adapt(m3, steps=3, graphed=True).losses, re_.losses[:3])
    with pytest.raises(ValueError, match="capturable"):
        adapt(m3, optimizer=sifsr.FlatAdam(m3.parameters(), lr=LR), graphed=True)


# ---- 4. the epoch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_train_epoch_graphed_is_the_eager_epoch(sifsr, masked):
    """seven batches: four full ones (the fourth captures), a short one, a full one (a replay), a short last one; masked batches
    carry (b,2) count rows, as the loaders of patches mined at a ratio give them"""
    window, hr, B = 8, 24, 3
    loader = []
    for i, (lst, up, ndvi, valid) in enumerate(step_batches(window, hr, B, masked, n_steps=7, seed=300)):
        b = 2 if i in (4, 6) else B
        item = [lst[:b].cpu(), up[:b].cpu(), ndvi[:b].cpu()]
        if masked:
            item += [valid[:b].cpu(), counts_for(sifsr, valid[:b], hr, "rows").cpu()]
        loader.append(tuple(item))
    sd = O.synthetic_state(72)

    def run(graphed):
        m = make_model(sifsr, copy.deepcopy(sd)).train()
        opt = sifsr.FlatAdam(m.parameters(), lr=LR, capturable=True)
        kw = {}
        if graphed:
            kw["graphed"] = sifsr.rloss.GraphedTrainStep(m, opt, B, STATS, ALPHA, GAMMA, window, hr, masked=masked, return_sr=True)
        means = sifsr.rloss.train_epoch(m, loader, opt, STATS, ALPHA, GAMMA, hr / window, "sr2", "cuda", masked_metrics=masked, **kw)
        if graphed:
            assert kw["graphed"].graph is not None
        return means, m.flat_parameters().detach().clone()

    (want, pe), (got, pg) = run(False), run(True)
    print(f"epoch means (ds, pl, loss, psnr, ssim), masked={masked}: eager {want}\n{'':>50}graphed {got}")
    assert len(got) == 5 and np.isfinite(got).all() and got == want and torch.equal(pg, pe)


# ---- 5. no host synchronisation --------------------------------------------------------------------------------------------------
def test_a_replaying_call_reads_nothing_back(sifsr, model):
    window, hr, shape, overlap, batch = LAYOUTS["x3"]
    kw = dict(window=window, batch=batch, overlap=overlap, cover_edges=True)
    lst, ndvi = granule(9, window, hr, shape)
    lst = sprinkle(lst)
    mask = torch.from_numpy(mask_sequence(shape, window)[0][2]).cuda()
    plain = sifsr.ratio.GranulePredictor(model, shape, STATS, hr=hr, conserve=1, **kw)
    gappy = sifsr.ratio.GranulePredictor(model, shape, STATS, hr=hr, conserve=1, gaps=True, **kw)
    lst4, ndvi4 = granule(9, 8, 32, shape)
    gappy4 = sifsr.predict.GranulePredictor(model, shape, STATS, gaps=True, **kw)
    # a masked step past its capture, counts given and formed
    B = 2
    batches = step_batches(window, hr, B, True, n_steps=5, seed=400)
    m = make_model(sifsr, O.synthetic_state(71)).train()
    opt = sifsr.FlatAdam(m.parameters(), lr=LR, capturable=True)
    step = sifsr.rloss.GraphedTrainStep(m, opt, B, STATS, ALPHA, GAMMA, window, hr, masked=True, return_sr=True)
    for b in batches[:4]:
        step(*b)
    given = counts_for(sifsr, batches[4][3], hr, "rows")
    for g in (plain, gappy, gappy4):
        assert g.graph is not None
    assert step.graph is not None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = [plain(lst, ndvi), gappy(lst, ndvi), gappy(lst, ndvi, mask=mask, return_info=True), gappy4(lst4, ndvi4, mask=mask),
               step(*batches[4]), step(*batches[4], given)]
        with pytest.raises(RuntimeError):                                                           # the positive control: the eager call reads
            sifsr.ratio.predict_granule_gaps(model, lst, ndvi, STATS, hr=hr, **kw)                    # the active count
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bit_equal(out[1], sifsr.ratio.predict_granule_gaps(model, lst, ndvi, STATS, hr=hr, conserve=1, **kw))
    assert int(out[2][1]["n_active"]) > 0 and all(torch.isfinite(t).all() for t in out[4][:3])
