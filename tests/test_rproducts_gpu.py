"""GPU: patch mining at a ratio, its loaders and the epoch loop on them (include/sifsr_rproducts.h, sifsr/rproducts.py, the `hr` of
sifsr/products.py, rloss.train_epoch / eval_epoch / fit).

  * against the NumPy restatement tests/rproducts_reference.py (held at x4 to tests/products_reference.py, and through it to the
    reference's recorded results, by tests/test_rproducts_host.py): counts, index, n_accepted, both patch arrays, the min / max
    columns of the moments and `decode` -- equal, NaN and +-inf positions included -- for every case, coverage and QC mode; the
    statistics with the bound of `check_statistics` (tests/test_products_host.py, argued there),
  * at (8, 32) every output of the `sifsrn_` calls against the `sifsrp_` calls on the same rasters, moments included: bit-equal,
  * the three access paths (16, 8 and 2 bytes) on the same rasters: bit-equal, moments included,
  * a patch of a granule = the patch of its own cut-out raster, two granules in turn = two single runs, nothing accepted: the
    outputs untouched,
  * `patch_counts` row n = `rloss.valid_counts` of patch n alone = the restatement; `expand_valid` = the restatement;
    `masked_psnr_ssim` through an all-ones expanded mask = `psnr_ssim` bit for bit,
  * the loaders: lst_up = `ratio.upsample`, the summed counts = `rloss.valid_counts` of the batch, a x4-mined set keeps today's bits,
  * end to end at (8, 24): fill, statistics, masked loader, one training and one validation epoch, `fit`, `predict_granule`,
  * the memory contract of the five writing entry points (CONTRACT below is the table tests/test_capi_gate.py checks against the
    header), and the refusals.

Every comparison of kernel output is for equality; nothing here has a tolerance taken from what the kernels give."""
import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import rproducts_reference as R
from tests.contract import L, S, dev, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import Partial, bit_equal
from tests.test_products_host import STAT_KEYS, check_statistics

pytestmark = pytest.mark.gpu
I32, I64, F64, U8 = torch.int32, torch.int64, torch.float64, torch.uint8
MODE_NAMES = ("MOD21A1D", "MOD11A1")
CONFIGS = [(ci, m, vi) for ci in range(len(R.CASES)) for m in (0, 1) for vi in range(len(R.COVERAGES))]
ALPHA, GAMMA = 0.5, -0.25


@pytest.fixture(scope="module")
def RP(sifsr):
    from sifsr import rproducts
    return rproducts


def case_of(ci):
    return R.make_case(*R.CASES[ci])


def rasters(case):
    return dev(case["lst_raw"]), dev(case["nir"]), dev(case["red"]), dev(case["qc"])


def clean_case(seed, h, w, ws, hr):
    """seeded rasters without a single bad pixel or zero denominator"""
    rs = np.random.RandomState(seed)
    fine = R.fine_shape(h, w, ws, hr)
    return {"ws": ws, "hr": hr, "lst_raw": rs.randint(13000, 16500, (h, w)).astype(np.uint16), "qc": np.zeros((h, w), np.uint8),
            "nir": rs.randint(1, 6000, fine).astype(np.int16), "red": rs.randint(1, 3000, fine).astype(np.int16)}


def same_bits_or_nan(got, want):
    """float32 arrays equal bit for bit, a NaN matching any NaN (the sign of the NaN of 0 / 0 is the platform's)"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def run_miner(RP, case, coverage=0.0, mode=0, arrays=None):
    lst_raw, nir, red, qc = arrays or rasters(case)
    miner = RP.PatchMiner(case["ws"], case["hr"], coverage, MODE_NAMES[mode])
    g = miner.add(lst_raw, nir, red, qc if mode else None)
    return g, miner.finish()


def mined_equal(a, b):
    return (bit_equal(a.lst, b.lst) and bit_equal(a.ndvi, b.ndvi) and np.array_equal(a.moments.view(np.uint64), b.moments.view(np.uint64))
            and np.array_equal(a.index, b.index))


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,mode,vi", CONFIGS)
def test_mining_vs_restatement(RP, ci, mode, vi):
    case = case_of(ci)
    ws, hr, cov = case["ws"], case["hr"], R.COVERAGES[vi]
    g, mined = run_miner(RP, case, cov, mode)
    counts, index, r_lst, r_ndvi, r_mom = R.mine(case, cov, mode)
    n = int(g["n_accepted"].item())
    assert n == len(index) == len(mined) >= 1 and mined.hr == hr and mined.window == ws
    assert np.array_equal(g["counts"].cpu().numpy(), counts) and g["counts"].dtype == I32
    assert np.array_equal(g["index"][:n].cpu().numpy(), index)
    assert np.array_equal(mined.index[:, 1:], index) and (mined.index[:, 0] == 0).all()
    lst, ndvi = mined.lst.cpu().numpy(), mined.ndvi.cpu().numpy()
    assert lst.shape == (n, 1, ws, ws) and ndvi.shape == (n, 1, hr, hr)
    assert np.array_equal(lst.view(np.uint32), r_lst.view(np.uint32))
    assert same_bits_or_nan(ndvi, r_ndvi) and np.abs(ndvi).max() <= 1.0
    m = mined.moments
    assert m.shape == (n, 8) and (m[:, 0] == ws * ws).all() and (m[:, 7] == 0).all()
    assert np.array_equal(m[:, 3], r_mom[:, 3]) and np.array_equal(m[:, 4], r_mom[:, 4])        # min, max
    want = R.statistics(r_lst, r_ndvi)
    check_statistics(mined.statistics(None), [want[k] for k in STAT_KEYS])
    if index[0, 0] == case["planted"]["clean"]:
        assert (ndvi[0] == 1).sum() >= 1 and (ndvi[0] == -1).sum() >= 1                          # the clipped pixels, the last one included
    if vi == 1 and mode == 0 and "bad_max" in case["planted"]:
        i = index[:, 0].tolist().index(case["planted"]["bad_max"])
        assert m[i, 3] == 0.0 and (lst[i] == 0).sum() == case["max_bad"]


@pytest.mark.parametrize("ci", range(len(R.CASES)))
@pytest.mark.parametrize("clip", [False, True])
def test_decode_bit_equal(RP, ci, clip):
    case = case_of(ci)
    lst_raw, nir, red, _ = rasters(case)
    lst_k, ndvi = RP.decode(lst_raw, nir, red, clip=clip)
    r_lst, r_ndvi = R.decode(case["lst_raw"], case["nir"], case["red"], clip=clip)
    assert tuple(lst_k.shape) == case["lst_raw"].shape and tuple(ndvi.shape) == case["nir"].shape
    assert np.array_equal(lst_k.cpu().numpy().view(np.uint32), r_lst.view(np.uint32))
    got = ndvi.cpu().numpy()
    assert same_bits_or_nan(got, r_ndvi)
    assert np.array_equal(np.isposinf(got), np.isposinf(r_ndvi)) and np.array_equal(np.isneginf(got), np.isneginf(r_ndvi))
    if len(case["full"]) >= 5:
        assert np.isnan(got).sum() >= 3 and (np.isinf(got).sum() >= 1) == (not clip)


# ---- 2. the two families at x4, the three access paths ------------------------------------------------------------------------------
def raw_buffers(case, fill, extra=0):
    h, w = case["lst_raw"].shape
    ws, hr = case["ws"], case["hr"]
    nwin, cap = len(R.windows(h, w, ws)), len([1 for q in R.windows(h, w, ws) if q[3]]) + extra
    mk = lambda shape, dt: torch.full(shape, fill, dtype=dt, device="cuda")
    return {"counts": mk((nwin, 2), I32), "index": mk((cap, 3), I32), "n": mk((1,), I32), "lst": mk((cap, 1, ws, ws), torch.float32),
            "ndvi": mk((cap, 1, hr, hr), torch.float32), "moments": mk((cap, 8), F64)}


def run_raw(L, case, b, family, arrays=None, mode=0, max_bad=0):
    lst_raw, nir, red, qc = arrays or rasters(case)
    h, w = case["lst_raw"].shape
    ws, cap = case["ws"], b["index"].shape[0]
    pair = (ws, case["hr"]) if family == "sifsrn_" else (ws,)
    L.call(family + "census", lst_raw, qc, nir, red, b["counts"], h, w, *pair, mode, S())
    L.call("sifsrp_select", b["counts"], b["index"], b["n"], h, w, ws, max_bad, cap, S())
    L.call(family + "gather", lst_raw, nir, red, b["index"], b["n"], b["lst"], b["ndvi"], b["moments"], h, w, *pair, cap, S())
    torch.cuda.synchronize()


def test_at_x4_the_two_families_give_the_same_bits(L, RP):
    """40 x 32 at (8, 32): the fine pitch is 128 int16, both families take their 16-byte path; the merge order is shared code"""
    from sifsr import products
    case = case_of(4)
    assert (case["ws"], case["hr"]) == (8, 32)
    for mode, max_bad in ((0, 0), (1, 0), (0, 3)):
        a, b = raw_buffers(case, 77), raw_buffers(case, 77)
        run_raw(L, case, a, "sifsrn_", mode=mode, max_bad=max_bad)
        run_raw(L, case, b, "sifsrp_", mode=mode, max_bad=max_bad)
        assert int(a["n"]) == int(b["n"]) >= 3
        for name in a:
            assert bit_equal(a[name], b[name]), name
    lst_raw, nir, red, _ = rasters(case)
    for clip in (False, True):
        got, want = RP.decode(lst_raw, nir, red, clip), products.decode(lst_raw, nir, red, clip)
        assert bit_equal(got[0], want[0]) and bit_equal(got[1], want[1])


def shifted(a, elements):
    """a device copy of the int16 raster `a` that starts `elements` int16 into a 16-byte aligned buffer"""
    buf = torch.zeros(a.size + 16, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[elements:elements + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() == buf.data_ptr() + 2 * elements and view.is_contiguous()
    return view


def test_the_three_access_paths_give_the_same_bits(L, RP):
    """36 x 24 at (12, 40): the fine pitch is 80 int16, so the aligned rasters take the 16-byte path; from a base 8 bytes on the
    same rasters take the 8-byte path, from a base one int16 on the 2-byte path.  Counts, patches, moments and decode: bit-equal."""
    case = case_of(2)
    assert case["nir"].shape[1] == 80
    lst_raw, nir, red, qc = rasters(case)
    assert nir.data_ptr() % 16 == 0 and red.data_ptr() % 16 == 0
    runs = []
    for off in (0, 4, 1):
        arrays = (lst_raw, nir if off == 0 else shifted(case["nir"], off), red if off == 0 else shifted(case["red"], off), qc)
        assert arrays[1].data_ptr() % 16 == (2 * off) % 16
        g, mined = run_miner(RP, case, 0.05, 0, arrays)
        runs.append((g["counts"].clone(), mined, RP.decode(*arrays[:3], clip=True)))
    assert len(runs[0][1]) >= 2
    for counts, mined, dec in runs[1:]:
        assert bit_equal(counts, runs[0][0]) and mined_equal(mined, runs[0][1])
        assert bit_equal(dec[0], runs[0][2][0]) and bit_equal(dec[1], runs[0][2][1])
    # a base that is only 8-byte aligned for ONE of the two rasters takes the narrower path for both
    g, mined = run_miner(RP, case, 0.05, 0, (lst_raw, nir, shifted(case["red"], 1), qc))
    assert mined_equal(mined, runs[0][1])
    # the LST raster from an odd base as well (decode picks its width from that base)
    lk = RP.decode(shifted(case["lst_raw"].view(np.int16), 1).view(torch.uint16), nir, red, clip=True)[0]
    assert bit_equal(lk, runs[0][2][0])


def test_a_patch_is_its_own_single_call(RP):
    """row i of a granule's result = the result of the window's own cut-out rasters (8 x 8 under 24 x 24: pitch 24, the 16-byte
    path, where the granule's pitch of 84 takes the 8-byte path): no patch depends on another, or on the path"""
    case = case_of(0)
    ws, hr = case["ws"], case["hr"]
    _, mined = run_miner(RP, case)
    assert len(mined) >= 3
    for i in (0, len(mined) // 2, len(mined) - 1):
        _, r, c = (int(v) for v in mined.index[i, 1:])
        fr, fc = R.fine_origin(r, c, ws, hr)
        cut = {"ws": ws, "hr": hr, "lst_raw": case["lst_raw"][r:r + ws, c:c + ws], "qc": case["qc"][r:r + ws, c:c + ws],
               "nir": case["nir"][fr:fr + hr, fc:fc + hr], "red": case["red"][fr:fr + hr, fc:fc + hr]}
        _, single = run_miner(RP, cut)
        assert len(single) == 1
        assert bit_equal(single.lst[0], mined.lst[i]) and bit_equal(single.ndvi[0], mined.ndvi[i])
        assert np.array_equal(single.moments[0].view(np.uint64), mined.moments[i].view(np.uint64))
    assert not bit_equal(mined.lst[0], mined.lst[len(mined) - 1])


def test_two_granules_are_two_single_runs(RP, sifsr):
    a, b = case_of(0), R.make_case(27, *R.CASES[0][1:])
    miner = RP.PatchMiner(8, 24, 0.05)
    miner.add(*rasters(a)[:3], granule_id=2021001)
    miner.add(*rasters(b)[:3])
    both = miner.finish()
    one, two = run_miner(RP, a, 0.05)[1], run_miner(RP, b, 0.05)[1]
    assert len(both) == len(one) + len(two) and len(one) >= 3 and len(two) >= 3 and both.hr == 24
    assert bit_equal(both.lst, torch.cat([one.lst, two.lst])) and bit_equal(both.ndvi, torch.cat([one.ndvi, two.ndvi]))
    assert np.array_equal(both.moments, np.concatenate([one.moments, two.moments]))
    assert np.array_equal(both.index[:, 1:], np.concatenate([one.index, two.index])[:, 1:])
    assert both.index[:, 0].tolist() == [2021001] * len(one) + [1] * len(two)
    with pytest.raises(sifsr.SifsrError):
        miner.finish()                                                         # the miner is empty again


def test_nothing_accepted_leaves_the_outputs_untouched(L):
    case = dict(clean_case(6, 40, 28, 8, 24))
    case["lst_raw"] = np.zeros_like(case["lst_raw"])
    b = raw_buffers(case, 77)
    run_raw(L, case, b, "sifsrn_")
    want = [[64, 0] if full else [-1, -1] for _, _, _, full in R.windows(40, 28, 8)]
    assert int(b["n"]) == 0 and b["counts"].cpu().tolist() == want
    for name in ("index", "lst", "ndvi", "moments"):
        assert (b[name] == 77).all(), name


# ---- 3. the masks -----------------------------------------------------------------------------------------------------------------
def seeded_valid(ws, n=6, seed=0):
    rs = np.random.RandomState(100 + ws + seed)
    valid = (rs.uniform(size=(n, 1, ws, ws)) < 0.6).astype(np.uint8) * rs.randint(1, 256, (n, 1, ws, ws)).astype(np.uint8)
    valid[1], valid[2] = 0, 1
    return valid


def mask_of(shape):
    """a seeded (B, h, w) mask of any non-zero bytes, about half of it valid"""
    rs = np.random.RandomState(sum(shape))
    return (rs.uniform(size=shape) < 0.5).astype(np.uint8) * rs.randint(1, 256, shape).astype(np.uint8)


@pytest.mark.parametrize("ws,hr", [(8, 24), (16, 40), (12, 40), (64, 192)])
def test_patch_counts(sifsr, RP, ws, hr):
    valid = seeded_valid(ws)
    v = torch.from_numpy(valid).cuda()
    got = RP.patch_counts(v, hr)
    assert got.dtype == I64 and tuple(got.shape) == (6, 2) and got.is_cuda
    want = R.patch_counts(valid[:, 0], hr)
    assert np.array_equal(got.cpu().numpy(), want) and want[1].tolist() == [0, 0] and want[2].tolist() == [ws * ws, hr * hr]
    for n in range(6):
        assert torch.equal(got[n], sifsr.rloss.valid_counts(v[n:n + 1], (hr, hr))), n
    assert torch.equal(got.sum(0), sifsr.rloss.valid_counts(v, (hr, hr)))
    assert torch.equal(RP.patch_counts(v[:, 0].contiguous() != 0, hr), got)                  # (N,w,w), bool


@pytest.mark.parametrize("shape,size", [((3, 8, 8), (24, 24)), ((3, 16, 16), (40, 40)), ((3, 12, 12), (40, 40)), ((2, 34, 18), (85, 45)),
                                        ((2, 64, 64), (192, 192))])
def test_expand_valid(RP, shape, size):
    valid = mask_of(shape)
    assert 0 < (valid != 0).sum() < valid.size
    got = RP.expand_valid(torch.from_numpy(valid).cuda(), size)
    assert got.dtype == U8 and tuple(got.shape) == (shape[0],) + size
    assert np.array_equal(got.cpu().numpy(), R.expand_valid(valid, size))
    got4 = RP.expand_valid(torch.from_numpy(valid[:, None]).cuda() != 0, size)                # (B,1,h,w), bool
    assert tuple(got4.shape) == (shape[0], 1) + size and torch.equal(got4[:, 0], got)
    if size[1] % 4 == 0:                                                                      # an output that is not on 4 bytes: byte stores
        out = torch.full((shape[0] * size[0] * size[1] + 4,), 9, dtype=U8, device="cuda")
        RP._lib.call("sifsrn_expand_valid", torch.from_numpy(valid).cuda(), out[1:], shape[0], shape[1], shape[2], size[0], size[1], S())
        assert torch.equal(out[1:-3].view(got.shape), got) and out[0] == 9 and (out[-3:] == 9).all()


def test_masked_metrics_through_an_all_ones_mask_are_psnr_ssim(sifsr, RP):
    rs = np.random.RandomState(8)
    sr = torch.from_numpy(rs.standard_normal((3, 1, 24, 24)).astype(np.float32)).cuda()
    tgt = sr + torch.from_numpy(0.1 * rs.standard_normal((3, 1, 24, 24)).astype(np.float32)).cuda()
    hr_mask = RP.expand_valid(torch.ones((3, 1, 8, 8), dtype=U8, device="cuda"), (24, 24))
    assert (hr_mask == 1).all()
    got, want = sifsr.metrics.masked_psnr_ssim(sr, tgt, hr_mask), sifsr.metrics.psnr_ssim(sr, tgt)
    assert bit_equal(got[0], want[0]) and bit_equal(got[1], want[1]) and float(want[0]) > 0


# ---- 4. the loaders -----------------------------------------------------------------------------------------------------------------
def test_a_loader_batch_at_a_ratio(sifsr, RP):
    _, mined = run_miner(RP, case_of(0))
    n = len(mined)
    assert n >= 5
    stats = mined.statistics(None)
    loader = mined.loader(None, 4, stats, shuffle=True, seed=3)
    order = loader.order(0)
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [4] * (n // 4) + ([n % 4] if n % 4 else []) and all(len(b) == 3 for b in batches)
    mean_n, std_n = np.float32(stats["mean_ndvi"]), np.float32(stats["std_ndvi"])
    for j, (lst_n, lst_up, ndvi_n) in enumerate(batches):
        sel = torch.from_numpy(order[4 * j:4 * j + 4]).cuda()
        assert lst_n.shape == (len(sel), 1, 8, 8) and lst_up.shape == ndvi_n.shape == (len(sel), 1, 24, 24)
        assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (lst_n, lst_up, ndvi_n))
        assert bit_equal(lst_n, (mined.lst[sel] - float(stats["mean_lst"])) / float(stats["std_lst"]))
        assert bit_equal(lst_up, sifsr.ratio.upsample(lst_n, (24, 24)))
        assert bit_equal(ndvi_n, (mined.ndvi[sel] - float(stats["mean_ndvi"])) / float(stats["std_ndvi"]))
        # the z-score itself against NumPy: one float32 subtraction and one division, within one unit in the last place each
        ref = (mined.ndvi[sel].cpu().numpy() - mean_n) / std_n
        assert np.abs(ndvi_n.cpu().numpy() - ref).max() <= 2 * np.spacing(np.float32(np.abs(ref).max()))


def test_a_x4_mined_set_keeps_todays_loader_bits(sifsr, RP):
    """(8, 32) mined by products.PatchMiner: hr is 4 * window, the loader is pipeline.prepare_tiles and the count one number"""
    from sifsr import pipeline, products
    case = case_of(4)
    miner = products.PatchMiner(8, 0.05)
    miner.add(*rasters(case)[:3])
    mined = miner.finish()
    assert mined.hr == 32 and len(mined) >= 4
    by_ratio = run_miner(RP, case, 0.05)[1]
    assert mined_equal(mined, by_ratio) and by_ratio.hr == 32
    for m in (mined, by_ratio):
        stats = m.statistics(None, valid_only=True)
        lst_n, lst_up, ndvi_n, valid, n_valid = next(iter(m.masked_loader(None, 4, stats, shuffle=False)))
        want_l = (m.filled[:4] - float(stats["mean_lst"])) / float(stats["std_lst"])
        want_n = (m.ndvi[:4] - float(stats["mean_ndvi"])) / float(stats["std_ndvi"])
        x = pipeline.prepare_tiles(want_l, want_n)
        assert bit_equal(lst_n, want_l) and bit_equal(lst_up, x[:, 0:1].contiguous()) and bit_equal(ndvi_n, want_n)
        assert n_valid.dim() == 0 and n_valid.dtype == I64 and int(n_valid) == int(valid.sum()) and m._patch_counts is None
    assert mined.statistics(None) == by_ratio.statistics(None)


# ---- 5. end to end at (8, 24) -------------------------------------------------------------------------------------------------------
def test_end_to_end_at_x3(sifsr, RP):
    from tests.test_model_gpu import make_model
    rloss = sifsr.rloss
    case = case_of(0)
    _, mined = run_miner(RP, case, 0.05)
    n = len(mined)
    assert n >= 8 and mined.fill() is mined and int((mined.valid == 0).sum()) == case["max_bad"]
    stats = mined.statistics(None, valid_only=True)
    assert stats["mini"] > 250 and mined.statistics(None)["mini"] == 0.0
    want_counts = R.patch_counts(mined.valid[:, 0].cpu().numpy(), 24)
    assert np.array_equal(mined.patch_counts().cpu().numpy(), want_counts) and want_counts[:, 1].min() == 9 * (64 - case["max_bad"])

    loader = mined.masked_loader(None, 5, stats, shuffle=False)
    batches = list(loader)
    assert len(batches) == len(loader) == -(-n // 5) and all(len(b) == 5 for b in batches)
    for j, (lst_n, lst_up, ndvi_n, valid, counts) in enumerate(batches):
        assert counts.dtype == I64 and tuple(counts.shape) == (2,) and counts.is_cuda
        assert torch.equal(counts, rloss.valid_counts(valid, (24, 24)))
        assert bit_equal(lst_up, sifsr.ratio.upsample(lst_n, (24, 24))) and valid.dtype == U8
        assert bit_equal(lst_n, (mined.filled[5 * j:5 * j + 5] - float(stats["mean_lst"])) / float(stats["std_lst"]))

    # one batch holds every patch: the epoch means ARE the batch's losses
    sd = O.synthetic_state(71)
    whole = lambda: mined.masked_loader(None, n, stats, shuffle=False)
    for masked_metrics in (False, True):
        m, ref = make_model(sifsr, sd), make_model(sifsr, sd)
        opt, ref_opt = sifsr.FlatAdam(m.parameters(), lr=1e-3), sifsr.FlatAdam(ref.parameters(), lr=1e-3)
        out = rloss.train_epoch(m, whole(), opt, stats, ALPHA, GAMMA, 3.0, masked_metrics=masked_metrics)
        lst_n, lst_up, ndvi_n, valid, counts = next(iter(whole()))
        direct = rloss.train_step(ref, ref_opt, lst_n, lst_up, ndvi_n, stats, ALPHA, GAMMA, 3.0, valid=valid, counts=counts, return_sr=True)
        assert len(out) == 5 and all(np.isfinite(v) for v in out)
        assert list(out[:3]) == [float(v) for v in direct[:3]]
        if masked_metrics:
            ps, ss = sifsr.metrics.masked_psnr_ssim(direct[3], lst_up, RP.expand_valid(valid, (24, 24)))
        else:
            ps, ss = sifsr.metrics.psnr_ssim(direct[3], lst_up)
        assert list(out[3:]) == [float(ps), float(ss)]
        ev = rloss.eval_epoch(m, whole(), stats, ALPHA, GAMMA, 3.0, masked_metrics=masked_metrics)
        step = rloss.eval_step(m, lst_n, lst_up, ndvi_n, stats, ALPHA, GAMMA, 3.0, valid=valid, counts=counts)
        assert len(ev) == 5 and all(np.isfinite(v) for v in ev) and list(ev[:3]) == [float(v) for v in step] and not m.training
    # several batches, no mask, (b, 2) count rows
    out = rloss.train_epoch(m, mined.loader(None, 4, stats, seed=1), opt, stats, ALPHA, GAMMA, 3.0, kind="sr1")
    assert all(np.isfinite(v) for v in out)
    rows = [(b[0], b[1], b[2], b[3], mined.patch_counts()[5 * j:5 * j + 5]) for j, b in enumerate(batches)]
    assert rows[0][4].shape == (5, 2)
    a = rloss.eval_epoch(m, rows, stats, ALPHA, GAMMA, 3.0)
    b = rloss.eval_epoch(m, batches, stats, ALPHA, GAMMA, 3.0)
    assert a == b

    mined.assign_split()
    assert len(mined.rows("Train")) >= 1 and len(mined.rows("Val")) >= 1
    m = make_model(sifsr, sd)
    opt = sifsr.FlatAdam(m.parameters(), lr=1e-3)
    ck = sifsr.train.ModelCheckpoint(2, patience=5)
    model, metrics = rloss.fit(m, mined.masked_loader("Train", 4, stats, seed=2), mined.masked_loader("Val", 4, stats, shuffle=False), 2, opt,
                               stats, ALPHA, GAMMA, 3.0, checkpoint=ck, masked_metrics=True)
    keys = {f"{s}_{k}" for s in ("train", "val") for k in ("dsloss", "perceploss", "loss", "psnr", "ssim")}
    assert model is m and keys <= set(metrics) <= keys | {"best_epoch"} and all(len(metrics[k]) == 2 for k in keys)
    assert all(np.isfinite(metrics[k]).all() for k in ("train_loss", "val_loss", "train_dsloss", "val_perceploss"))
    assert ck.best_epoch in (1, 2) and metrics.get("best_epoch", ck.best_epoch) in (1, 2)

    lst_raw, nir, red, _ = rasters(case)
    lst_k, ndvi = RP.decode(lst_raw, nir, red)
    sr = sifsr.ratio.predict_granule(m, lst_k, torch.nan_to_num(ndvi, 0.0, 1.0, -1.0), stats, window=8, hr=24, batch=8)
    assert tuple(sr.shape) == (120, 84) and torch.isfinite(sr).all() and float(sr.abs().max()) > 0


# ---- 6. memory contract ---------------------------------------------------------------------------------------------------------------
def _inputs(k, case, with_qc=True):
    lst_raw, nir, red = (k.t(n, torch.from_numpy(np.array(case[n]))) for n in ("lst_raw", "nir", "red"))
    qc = k.t("qc", torch.from_numpy(np.array(case["qc"]))) if with_qc else None
    return lst_raw, nir, red, qc


def _partial(t, n):
    """rows < n of `t` written, the rest must keep what they held"""
    mask = (torch.arange(t.shape[0]) < n).reshape((-1,) + (1,) * (t.dim() - 1))
    init = t.clone()
    return lambda: Partial(t, mask, init)


def decode_case(case, clip):
    def make(k):
        lst_raw, nir, red, _ = _inputs(k, case, False)
        (h, w), (fh, fw) = case["lst_raw"].shape, case["nir"].shape
        lst_k, ndvi = k.o("lst_k", h, w), k.o("ndvi", fh, fw)
        return (lambda: k.L.call("sifsrn_decode", lst_raw, nir, red, lst_k, ndvi, h, w, fh, fw, clip, S())), {"lst_k": lst_k, "ndvi": ndvi}
    return make


def census_case(case, mode):
    def make(k):
        lst_raw, nir, red, qc = _inputs(k, case, mode == 1)
        h, w = case["lst_raw"].shape
        counts = k.o("counts", len(R.windows(h, w, case["ws"])), 2, dtype=I32)
        return (lambda: k.L.call("sifsrn_census", lst_raw, qc, nir, red, counts, h, w, case["ws"], case["hr"], mode, S())), {"counts": counts}
    return make


def gather_case(case, coverage, extra=0):
    def make(k):
        lst_raw, nir, red, _ = _inputs(k, case, False)
        h, w = case["lst_raw"].shape
        ws, hr = case["ws"], case["hr"]
        counts = R.census(case["lst_raw"], case["qc"], case["nir"], case["red"], ws, hr, 0)
        sel = R.select(counts, h, w, ws, coverage)
        n, cap = len(sel), len([1 for q in R.windows(h, w, ws) if q[3]]) + extra
        idx = np.full((cap, 3), -12345, dtype=np.int32)                        # rows >= n: never to be used
        idx[:n] = sel
        index, n_acc = k.t("index", torch.from_numpy(idx)), k.t("n_accepted", torch.tensor([n], dtype=I32))
        lst, ndvi, mom = k.o("lst", cap, 1, ws, ws), k.o("ndvi", cap, 1, hr, hr), k.o("moments", cap, 8, dtype=F64)
        parts = {"lst": _partial(lst, n), "ndvi": _partial(ndvi, n), "moments": _partial(mom, n)}
        call = lambda: k.L.call("sifsrn_gather", lst_raw, nir, red, index, n_acc, lst, ndvi, mom, h, w, ws, hr, cap, S())
        return call, parts
    return make


def counts_case(ws, hr):
    def make(k):
        valid = k.t("valid", torch.from_numpy(seeded_valid(ws)))
        counts = k.o("counts", 6, 2, dtype=I64)
        return (lambda: k.L.call("sifsrn_patch_counts", valid, counts, 6, ws, hr, S())), {"counts": counts}
    return make


def expand_case(shape, size):
    def make(k):
        valid = k.t("valid", torch.from_numpy(mask_of(shape)))
        out = k.o("out", shape[0], *size, dtype=U8)
        return (lambda: k.L.call("sifsrn_expand_valid", valid, out, *shape, *size, S())), {"out": out}
    return make


def _contract():
    # (NaN-free results are part of the contract check: decode and gather run on rasters without a zero denominator among what they
    # write; the planted cases are accepted windows only.)  One case per access path: pitches 84, 45, 80, 76, 128 and 192 int16.
    clean = [clean_case(40 + i, *R.CASES[i][1:]) for i in range(len(R.CASES))]
    planted = [case_of(i) for i in range(len(R.CASES))]
    return {
        "sifsrn_decode": [decode_case(clean[0], 0), decode_case(clean[1], 1), decode_case(clean[2], 0), decode_case(clean[5], 1)],
        "sifsrn_census": [census_case(planted[0], 0), census_case(planted[0], 1), census_case(planted[1], 0), census_case(planted[2], 1),
                          census_case(planted[3], 0), census_case(planted[5], 0)],
        "sifsrn_gather": [gather_case(planted[0], 0.0), gather_case(planted[0], 0.05, extra=1), gather_case(planted[1], 0.0),
                          gather_case(planted[2], 0.05), gather_case(planted[3], 0.0), gather_case(clean[5], 0.0)],
        "sifsrn_patch_counts": [counts_case(8, 24), counts_case(16, 40), counts_case(12, 40), counts_case(64, 192)],
        "sifsrn_expand_valid": [expand_case((6, 8, 8), (24, 24)), expand_case((6, 16, 16), (40, 40)), expand_case((2, 34, 18), (85, 45)),
                                expand_case((6, 12, 12), (40, 40))],
    }


CONTRACT = _contract()
CONTRACT_CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CONTRACT_CASES, ids=[f"{n[7:]}-{i}" for n, i in CONTRACT_CASES])
def test_memory_contract(L, name, idx):
    """every output written where the header says and nowhere else -- NaN-free under the NaN poison, bit-identical under every
    poison, rows past n_accepted still holding their poison --, inputs untouched, nothing outside the buffers written, and the same
    bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=32 << 20)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(sifsr, RP, L):
    case = case_of(1)                                                          # 34 x 18 at (16, 40): q = 2, fine 85 x 45
    lst_raw, nir, red, qc = rasters(case)
    E = sifsr.SifsrError
    with pytest.raises(E, match="exactly"):
        RP.PatchMiner(16, 40).add(lst_raw, nir[:80].contiguous(), red[:80].contiguous())          # a fine raster of the wrong size
    with pytest.raises(E, match="same ratio"):
        RP.decode(lst_raw, nir[:, :40].contiguous(), red[:, :40].contiguous())                    # unequal axis ratios
    with pytest.raises(E, match="multiples of q"):
        RP.PatchMiner(16, 40).add(lst_raw[:33].contiguous(), nir, red)                            # h no multiple of q
    with pytest.raises(E, match="sensor model"):
        RP.PatchMiner(20, 24)
    with pytest.raises(E):
        RP.PatchMiner(16, 40).add(lst_raw[:14].contiguous(), nir[:35].contiguous(), red[:35].contiguous())   # smaller than a window
    with pytest.raises(ValueError):
        RP.PatchMiner(16, 40, qc_mode="MOD11A1").add(lst_raw, nir, red)                           # no QC raster
    with pytest.raises(E):
        RP.decode(lst_raw.cpu(), nir, red)                                                        # no CPU path
    with pytest.raises(E):
        RP.decode(nir, nir, red)                                                                  # int16 where uint16 is due
    with pytest.raises(E):
        RP.expand_valid(torch.ones((1, 8, 8), dtype=U8, device="cuda"), (7, 24))
    with pytest.raises(E):
        RP.patch_counts(torch.ones((1, 8, 8), dtype=torch.float32, device="cuda"), 24)
    # the x4 family keeps its refusal of any other ratio
    with pytest.raises(ValueError):
        sifsr.products.decode(lst_raw, nir, red)
    with pytest.raises(ValueError):
        sifsr.products.PatchMiner(16).add(lst_raw, nir, red)
    # the C entry points: nothing is launched
    b = raw_buffers(case, 55)
    h, p = L.lib(), (lambda t: t.data_ptr())
    assert h.sifsrn_census(p(lst_raw), None, p(nir), p(red), p(b["counts"]), 33, 18, 16, 40, 0, S()) == 1001
    assert h.sifsrn_census(p(lst_raw), None, p(nir), p(red), p(b["counts"]), 34, 18, 20, 24, 0, S()) == 1001
    assert h.sifsrn_census(p(lst_raw), None, p(nir), p(red), p(b["counts"]), 34, 18, 16, 40, 1, S()) == 1002
    args = (p(b["index"]), p(b["n"]), p(b["lst"]), p(b["ndvi"]), p(b["moments"]))
    assert h.sifsrn_gather(p(lst_raw), p(nir), p(red), *args, 34, 18, 16, 40, 1, S()) == 1001     # cap < the full windows
    assert h.sifsrn_gather(p(lst_raw), p(nir), p(red), args[0], args[1], args[2], args[3] + 4, args[4], 34, 18, 16, 40, 2, S()) == 1002
    torch.cuda.synchronize()
    assert all((t == 55).all() for t in b.values())
    _, mined = run_miner(RP, case)
    with pytest.raises(E, match="x4"):
        sifsr.MinedDataset(mined, None)
