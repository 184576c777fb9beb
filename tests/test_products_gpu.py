"""GPU: patch mining from raw MODIS rasters (include/sifsr_products.h, sifsr/products.py).

  * against the reference's own results (tests/golden/golden_products_v1.npz): both counts per window, the accepted
    [k, row0, col0] lists and n_accepted for every case, coverage and QC mode -- equal; the LST patches by sha256; the statistics
    (maxi / mini exactly, means and standard deviations to 1e-12 relative, the bound argued in tests/test_products_host.py),
  * against the NumPy restatement tests/products_reference.py (pinned to the same golden by tests/test_products_host.py): NDVI
    patches and `decode` bit-equal, NaN and +-inf positions included; the odd-width raster that takes the 8-byte access path,
  * edge cases: nothing accepted (outputs untouched), everything accepted, two granules in turn = two single runs, a patch of a
    granule = the patch of its own cut-out raster, bit for bit,
  * the memory contract of every entry point in the guarded, poisoned arena of tests/memcheck.py (CONTRACT below is the table
    tests/test_capi_gate.py checks against the header): rows past n_accepted keep their initial content,
  * the argument errors, and the way into the training loop: `loader`, one `train_epoch`, `predict_granule` on `decode`.

Every comparison of kernel output is for equality; nothing here has a tolerance taken from what the kernels give."""
import numpy as np
import pytest
import torch

from tests import products_reference as R
from tests.contract import L, S, dev, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import Partial, bit_equal
from tests.test_products_host import CONFIGS, check_statistics, golden  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
I32, F64 = torch.int32, torch.float64
SHAPE_ERR, ARG_ERR = 1001, 1002
MODE_NAMES = ("MOD21A1D", "MOD11A1")
WS = 64


@pytest.fixture(scope="module")
def P(sifsr):
    from sifsr import products
    return products


def rasters(case):
    return dev(case["lst_raw"]), dev(case["nir"]), dev(case["red"]), dev(case["qc"])


def clean_case(seed, h, w):
    """seeded rasters without a single bad pixel or zero denominator"""
    rs = np.random.RandomState(seed)
    return {"lst_raw": rs.randint(13000, 16500, (h, w)).astype(np.uint16), "qc": np.zeros((h, w), np.uint8),
            "nir": rs.randint(1, 6000, (4 * h, 4 * w)).astype(np.int16), "red": rs.randint(1, 3000, (4 * h, 4 * w)).astype(np.int16)}


def same_bits_or_nan(got, want):
    """float32 arrays equal bit for bit, a NaN matching any NaN (the sign of the NaN of 0 / 0 is the platform's)"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def run_miner(P, case, coverage=0.0, mode=0, window=WS):
    lst_raw, nir, red, qc = rasters(case)
    miner = P.PatchMiner(window, coverage, MODE_NAMES[mode])
    g = miner.add(lst_raw, nir, red, qc if mode else None)
    return g, miner.finish()


# ---- 1. against the reference's results and the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("ci,mode,vi", CONFIGS)
def test_mining_vs_golden(P, golden, ci, mode, vi):  # noqa: F811
    seed, h, w = R.CASES[ci]
    case = R.make_case(seed, h, w)
    g, mined = run_miner(P, case, R.COVERAGES[vi], mode)
    key = f"c{ci}_m{mode}_v{vi}"
    want = golden[key + "_index"]
    n = int(g["n_accepted"].item())
    assert n == len(want) == len(mined)
    assert np.array_equal(g["counts"].cpu().numpy(), golden[f"c{ci}_m{mode}_counts"])
    assert np.array_equal(g["index"][:n].cpu().numpy(), want)
    assert np.array_equal(mined.index[:, 1:], want) and (mined.index[:, 0] == 0).all()
    _, _, r_lst, r_ndvi, r_mom = R.mine(case, WS, R.COVERAGES[vi], mode)
    lst, ndvi = mined.lst.cpu().numpy(), mined.ndvi.cpu().numpy()
    assert lst.shape == (n, 1, 64, 64) and ndvi.shape == (n, 1, 256, 256)
    ks = golden[f"c{ci}_sha_k"].tolist()
    for i, k in enumerate(want[:, 0].tolist()):
        assert R.sha(lst[i, 0]) == golden[f"c{ci}_sha_lst"][ks.index(k)]              # bit-equal to np.float32(0.02) * raw
        assert R.sha(ndvi[i, 0]) == golden[f"c{ci}_sha_ndvi"][ks.index(k)]
    assert same_bits_or_nan(ndvi, r_ndvi) and np.abs(ndvi).max() <= 1.0
    m = mined.moments
    assert m.shape == (n, 8) and (m[:, 0] == 4096).all() and (m[:, 7] == 0).all()
    assert np.array_equal(m[:, 3], r_mom[:, 3]) and np.array_equal(m[:, 4], r_mom[:, 4])        # min, max
    assert mined.assign_split().tolist() == golden[key + "_labels"].tolist()
    if (mined.split == "Train").any():
        check_statistics(mined.statistics("Train"), golden[key + "_stats"])
    if ci == 0 and vi == 1:
        assert mined.moments[1, 3] == 0.0 and (ndvi[0] == 1).sum() >= 1 and (ndvi[0] == -1).sum() >= 1


@pytest.mark.parametrize("ci", range(len(R.CASES)))
@pytest.mark.parametrize("clip", [False, True])
def test_decode_bit_equal(P, ci, clip):
    seed, h, w = R.CASES[ci]
    case = R.make_case(seed, h, w)
    lst_raw, nir, red, _ = rasters(case)
    lst_k, ndvi = P.decode(lst_raw, nir, red, clip=clip)
    r_lst, r_ndvi = R.decode(case["lst_raw"], case["nir"], case["red"], clip=clip)
    assert tuple(lst_k.shape) == (h, w) and tuple(ndvi.shape) == (4 * h, 4 * w)
    assert np.array_equal(lst_k.cpu().numpy().view(np.uint32), r_lst.view(np.uint32))
    got = ndvi.cpu().numpy()
    assert same_bits_or_nan(got, r_ndvi)
    if len(case["full"]) >= 6:
        assert np.isnan(got).sum() >= 3 and (np.isinf(got).sum() >= 1) == (not clip)
        assert np.array_equal(np.isposinf(got), np.isposinf(r_ndvi))


def test_decode_tail_and_numpy_input(P):
    """7 x 5 = 35 LST pixels: four 16-byte groups and a tail of 3; NumPy arrays are copied to the device"""
    case = clean_case(3, 7, 5)
    lst_k, ndvi = P.decode(case["lst_raw"], case["nir"], case["red"])
    r_lst, r_ndvi = R.decode(case["lst_raw"], case["nir"], case["red"])
    assert np.array_equal(lst_k.cpu().numpy().view(np.uint32), r_lst.view(np.uint32))
    assert np.array_equal(ndvi.cpu().numpy().view(np.uint32), r_ndvi.view(np.uint32))


def test_odd_width_takes_the_8_byte_path(P):
    """w = 67: rows of the fine rasters start on 8 bytes only; 68 x 67 has one full window, (0, 0)"""
    case = clean_case(4, 68, 67)
    lst = case["lst_raw"].copy()
    lst[5, 7] = 0
    case["lst_raw"] = lst
    g, mined = run_miner(P, case, 0.01)
    counts, index, r_lst, r_ndvi, r_mom = R.mine(case, WS, 0.01, 0)
    assert np.array_equal(g["counts"].cpu().numpy(), counts) and counts.tolist() == [[1, 0], [-1, -1], [-1, -1], [-1, -1]]
    assert np.array_equal(mined.index[:, 1:], index) and len(mined) == 1
    assert np.array_equal(mined.lst.cpu().numpy(), r_lst) and np.array_equal(mined.ndvi.cpu().numpy(), r_ndvi)
    st, want = mined.statistics(None), R.statistics(r_lst, r_ndvi)
    check_statistics(st, [want[k] for k in st])


# ---- 2. edge cases ------------------------------------------------------------------------------------------------------------
def raw_buffers(nwin, cap, fill):
    mk = lambda shape, dt: torch.full(shape, fill, dtype=dt, device="cuda")
    return {"counts": mk((nwin, 2), I32), "index": mk((cap, 3), I32), "n": mk((1,), I32), "lst": mk((cap, 1, WS, WS), torch.float32),
            "ndvi": mk((cap, 1, 4 * WS, 4 * WS), torch.float32), "moments": mk((cap, 8), F64)}


def run_raw(L, case, b, mode=0, max_bad=0):
    lst_raw, nir, red, qc = rasters(case)
    h, w = case["lst_raw"].shape
    cap = b["index"].shape[0]
    L.call("sifsrp_census", lst_raw, qc, nir, red, b["counts"], h, w, WS, mode, S())
    L.call("sifsrp_select", b["counts"], b["index"], b["n"], h, w, WS, max_bad, cap, S())
    L.call("sifsrp_gather", lst_raw, nir, red, b["index"], b["n"], b["lst"], b["ndvi"], b["moments"], h, w, WS, cap, S())
    torch.cuda.synchronize()


def test_nothing_accepted_leaves_the_outputs_untouched(L):
    case = clean_case(6, 128, 128)
    case["lst_raw"] = np.zeros_like(case["lst_raw"])
    b = raw_buffers(4, 4, 77)
    run_raw(L, case, b)
    assert int(b["n"]) == 0 and b["counts"].cpu().tolist() == [[4096, 0]] * 4
    for name in ("index", "lst", "ndvi", "moments"):
        assert (b[name] == 77).all(), name


def test_everything_accepted(L, P):
    case = clean_case(7, 128, 128)
    b = raw_buffers(4, 4, 77)
    run_raw(L, case, b)
    assert int(b["n"]) == 4 and b["counts"].cpu().tolist() == [[0, 0]] * 4
    assert b["index"].cpu().tolist() == [[1, 0, 0], [2, 64, 0], [3, 0, 64], [4, 64, 64]]       # column blocks outer, row blocks inner
    _, _, r_lst, r_ndvi, _ = R.mine(case)
    assert np.array_equal(b["lst"].cpu().numpy(), r_lst) and np.array_equal(b["ndvi"].cpu().numpy(), r_ndvi)
    g, mined = run_miner(P, case)
    assert bit_equal(mined.lst, b["lst"]) and bit_equal(mined.ndvi, b["ndvi"])
    assert np.array_equal(mined.moments, b["moments"].cpu().numpy())


def test_two_granules_are_two_single_runs(P):
    a, b = R.make_case(*R.CASES[0]), R.make_case(*R.CASES[1])
    miner = P.PatchMiner(WS, 0.01)
    miner.add(*rasters(a)[:3], granule_id=2021001)
    miner.add(*rasters(b)[:3])
    both = miner.finish()
    one, two = run_miner(P, a, 0.01)[1], run_miner(P, b, 0.01)[1]
    assert len(both) == len(one) + len(two) == 3 + 8
    assert bit_equal(both.lst, torch.cat([one.lst, two.lst])) and bit_equal(both.ndvi, torch.cat([one.ndvi, two.ndvi]))
    assert np.array_equal(both.moments, np.concatenate([one.moments, two.moments]))
    assert np.array_equal(both.index[:, 1:], np.concatenate([one.index, two.index])[:, 1:])
    assert both.index[:, 0].tolist() == [2021001] * 3 + [1] * 8
    with pytest.raises(P._lib.SifsrError):
        miner.finish()                                                         # the miner is empty again


def test_a_patch_is_its_own_single_call(P):
    """row i of a granule's result = the result of the 64 x 64 raster cut out at its window: no patch depends on another"""
    case = R.make_case(*R.CASES[1])
    _, mined = run_miner(P, case)
    assert len(mined) == 7
    for i in (0, 3, 6):
        _, r, c = mined.index[i, 1:]
        cut = {"lst_raw": case["lst_raw"][r:r + WS, c:c + WS], "qc": case["qc"][r:r + WS, c:c + WS],
               "nir": case["nir"][4 * r:4 * (r + WS), 4 * c:4 * (c + WS)], "red": case["red"][4 * r:4 * (r + WS), 4 * c:4 * (c + WS)]}
        _, single = run_miner(P, cut)
        assert len(single) == 1
        assert bit_equal(single.lst[0], mined.lst[i]) and bit_equal(single.ndvi[0], mined.ndvi[i])
        assert np.array_equal(single.moments[0], mined.moments[i])
    assert not bit_equal(mined.lst[0], mined.lst[6])


# ---- 3. memory contract -------------------------------------------------------------------------------------------------------
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
        h, w = case["lst_raw"].shape
        lst_k, ndvi = k.o("lst_k", h, w), k.o("ndvi", 4 * h, 4 * w)
        return (lambda: k.L.call("sifsrp_decode", lst_raw, nir, red, lst_k, ndvi, h, w, clip, S())), {"lst_k": lst_k, "ndvi": ndvi}
    return make


def census_case(case, mode):
    def make(k):
        lst_raw, nir, red, qc = _inputs(k, case, mode == 1)
        h, w = case["lst_raw"].shape
        counts = k.o("counts", len(R.windows(h, w)), 2, dtype=I32)
        return (lambda: k.L.call("sifsrp_census", lst_raw, qc, nir, red, counts, h, w, WS, mode, S())), {"counts": counts}
    return make


def select_case(case, coverage, extra=0):
    def make(k):
        h, w = case["lst_raw"].shape
        counts = R.census(case["lst_raw"], case["qc"], case["nir"], case["red"], WS, 0)
        n = len(R.select(counts, h, w, WS, coverage))
        cap = len([1 for q in R.windows(h, w) if q[3]]) + extra
        c = k.t("counts", torch.from_numpy(counts))
        index, n_acc = k.o("index", cap, 3, dtype=I32), k.o("n_accepted", 1, dtype=I32)
        part = _partial(index, n)
        call = lambda: k.L.call("sifsrp_select", c, index, n_acc, h, w, WS, R.max_bad(coverage), cap, S())
        return call, {"index": part, "n_accepted": n_acc}
    return make


def gather_case(case, coverage, extra=0):
    def make(k):
        lst_raw, nir, red, _ = _inputs(k, case, False)
        h, w = case["lst_raw"].shape
        counts = R.census(case["lst_raw"], case["qc"], case["nir"], case["red"], WS, 0)
        sel = R.select(counts, h, w, WS, coverage)
        n, cap = len(sel), len([1 for q in R.windows(h, w) if q[3]]) + extra
        idx = np.full((cap, 3), -12345, dtype=np.int32)                        # rows >= n: never to be used
        idx[:n] = sel
        index, n_acc = k.t("index", torch.from_numpy(idx)), k.t("n_accepted", torch.tensor([n], dtype=I32))
        lst, ndvi, mom = k.o("lst", cap, 1, WS, WS), k.o("ndvi", cap, 1, 4 * WS, 4 * WS), k.o("moments", cap, 8, dtype=F64)
        parts = {"lst": _partial(lst, n), "ndvi": _partial(ndvi, n), "moments": _partial(mom, n)}
        call = lambda: k.L.call("sifsrp_gather", lst_raw, nir, red, index, n_acc, lst, ndvi, mom, h, w, WS, cap, S())
        return call, parts
    return make


def _contract():
    c0, c1, c3 = (R.make_case(*R.CASES[i]) for i in (0, 1, 3))
    odd = clean_case(4, 68, 67)
    return {
        # (NaN-free results are part of the contract check: decode runs on rasters without a zero denominator)
        "sifsrp_decode": [decode_case(clean_case(1, 7, 5), 0), decode_case(clean_case(2, 64, 72), 1), decode_case(c3, 0), decode_case(odd, 1)],
        "sifsrp_census": [census_case(c0, 0), census_case(c0, 1), census_case(c1, 1), census_case(c3, 0), census_case(odd, 0)],
        "sifsrp_select": [select_case(c0, 0.0), select_case(c0, 0.01, extra=2), select_case(c1, 0.0), select_case(c3, 0.0)],
        "sifsrp_gather": [gather_case(c0, 0.0), gather_case(c0, 0.01, extra=1), gather_case(c1, 0.0), gather_case(c3, 0.0),
                          gather_case(odd, 0.0)],
    }


CONTRACT = _contract()
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output written where the header says and nowhere else -- NaN-free under the NaN poison, bit-identical under every
    poison, rows past n_accepted still holding their poison --, inputs untouched, nothing outside the buffers written, and the same
    bits on ordinary allocations."""
    run_contract(L, CONTRACT[name][idx], seed=sum(map(ord, name)) * 131 + idx, capacity=64 << 20)


# ---- 4. argument errors -------------------------------------------------------------------------------------------------------
def test_errors(sifsr, P, L):
    case = clean_case(8, 128, 64)
    lst_raw, nir, red, qc = rasters(case)
    b = raw_buffers(2, 1, 55)
    lk, nd = torch.full((128, 64), 55.0, device="cuda"), torch.full((512, 256), 55.0, device="cuda")
    h = L.lib()
    p = lambda t: t.data_ptr()
    assert h.sifsrp_decode(None, p(nir), p(red), p(lk), p(nd), 128, 64, 0, S()) == ARG_ERR
    assert h.sifsrp_decode(p(lst_raw), p(nir), p(red), p(lk), None, 128, 64, 0, S()) == ARG_ERR
    assert h.sifsrp_decode(p(lst_raw), p(nir), p(red), p(lk), p(nd), 0, 64, 0, S()) == SHAPE_ERR
    assert h.sifsrp_decode(p(lst_raw), p(nir), p(red), p(lk), p(nd) + 4, 128, 64, 0, S()) == ARG_ERR       # not 16-byte aligned
    assert h.sifsrp_census(p(lst_raw), None, p(nir), p(red), None, 128, 64, 64, 0, S()) == ARG_ERR
    assert h.sifsrp_census(p(lst_raw), None, p(nir), p(red), p(b["counts"]), 128, 64, 64, 1, S()) == ARG_ERR   # mode 1 needs qc
    assert h.sifsrp_census(p(lst_raw), p(qc), p(nir), p(red), p(b["counts"]), 128, 64, 64, 2, S()) == ARG_ERR  # bad qc_mode
    assert h.sifsrp_census(p(lst_raw), p(qc), p(nir), p(red), p(b["counts"]), 60, 64, 64, 0, S()) == SHAPE_ERR # h < window
    assert h.sifsrp_census(p(lst_raw), p(qc), p(nir), p(red), p(b["counts"]), 128, 64, 30, 0, S()) == SHAPE_ERR  # window % 4
    assert h.sifsrp_select(p(b["counts"]), p(b["index"]), None, 128, 64, 64, 0, 1, S()) == ARG_ERR
    assert h.sifsrp_select(p(b["counts"]), p(b["index"]), p(b["n"]), 128, 64, 64, 0, 0, S()) == SHAPE_ERR      # cap < the full windows
    assert h.sifsrp_select(p(b["counts"]), p(b["index"]), p(b["n"]), 128, 64, 62, 0, 1, S()) == SHAPE_ERR
    args = (p(b["index"]), p(b["n"]), p(b["lst"]), p(b["ndvi"]), p(b["moments"]))
    assert h.sifsrp_gather(p(lst_raw), p(nir), None, *args, 128, 64, 64, 1, S()) == ARG_ERR
    assert h.sifsrp_gather(p(lst_raw), p(nir), p(red), *args, 128, 64, 64, 0, S()) == SHAPE_ERR
    assert h.sifsrp_gather(p(lst_raw), p(nir), p(red), *args, 128, 32, 64, 1, S()) == SHAPE_ERR                # w < window
    torch.cuda.synchronize()
    assert (lk == 55).all() and (nd == 55).all() and all((t == 55).all() for t in b.values())                 # nothing was launched
    # the Python layer
    E = sifsr.SifsrError
    with pytest.raises(E):
        P.decode(lst_raw.cpu(), nir, red)                                      # no CPU path
    with pytest.raises(E):
        P.decode(nir, nir, red)                                                # int16 where uint16 is due
    with pytest.raises(ValueError):
        P.decode(lst_raw, nir[:100].contiguous(), red)
    with pytest.raises(ValueError):
        P.PatchMiner(qc_mode="MOD11A1").add(lst_raw, nir, red)                 # no QC raster
    with pytest.raises(ValueError):
        P.PatchMiner().add(lst_raw[:32].contiguous(), nir[:128].contiguous(), red[:128].contiguous())


# ---- 5. into the training loop ------------------------------------------------------------------------------------------------
def test_loader_train_epoch_and_predict_granule(sifsr, P):
    from sifsr import pipeline
    _, mined = run_miner(P, R.make_case(*R.CASES[1]))
    assert len(mined) == 7
    stats = mined.statistics(None)
    loader = mined.loader(None, 4, stats, shuffle=True, seed=3)
    assert len(loader) == 2
    order = loader.order(0)
    assert sorted(order.tolist()) == list(range(7)) and order.tolist() != list(range(7))
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [4, 3]
    mean_l, std_l = np.float32(stats["mean_lst"]), np.float32(stats["std_lst"])
    mean_n, std_n = np.float32(stats["mean_ndvi"]), np.float32(stats["std_ndvi"])
    for j, (lst_n, lst_up, ndvi_n) in enumerate(batches):
        rows = order[4 * j:4 * j + 4]
        sel = torch.from_numpy(rows).cuda()
        assert lst_n.shape == (len(rows), 1, 64, 64) and lst_up.shape == ndvi_n.shape == (len(rows), 1, 256, 256)
        assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (lst_n, lst_up, ndvi_n))
        want_l = (mined.lst[sel] - float(stats["mean_lst"])) / float(stats["std_lst"])
        assert bit_equal(lst_n, want_l) and bit_equal(lst_up, pipeline.bicubic_up4(want_l).contiguous())
        assert bit_equal(ndvi_n, (mined.ndvi[sel] - float(stats["mean_ndvi"])) / float(stats["std_ndvi"]))
        # and the z-score itself against NumPy: one float32 subtraction and one division, within one unit in the last place each
        ref = (mined.lst[sel].cpu().numpy() - mean_l) / std_l
        assert np.abs(lst_n.cpu().numpy() - ref).max() <= 2 * np.spacing(np.float32(np.abs(ref).max()))
        ref = (mined.ndvi[sel].cpu().numpy() - mean_n) / std_n
        assert np.abs(ndvi_n.cpu().numpy() - ref).max() <= 2 * np.spacing(np.float32(np.abs(ref).max()))
    assert list(loader)[0][0].shape[0] == 4 and loader.order(1).tolist() != order.tolist()      # a new permutation per epoch

    torch.manual_seed(0)
    model = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda()
    opt = sifsr.FlatAdam(model.parameters(), lr=1e-4)
    out = sifsr.train.train_epoch(model, mined.loader(None, 4, stats, seed=1), opt, stats, 0.5, -0.25)
    assert len(out) == 5 and all(np.isfinite(v) for v in out[:3])
    out = sifsr.train.eval_epoch(model, mined.loader(None, 4, stats, shuffle=False), stats, 0.5, -0.25)
    assert all(np.isfinite(v) for v in out[:3])

    case = R.make_case(*R.CASES[2])                                            # 128 x 64
    lst_raw, nir, red, _ = rasters(case)
    sr = sifsr.predict.predict_granule(model, *P.decode(lst_raw, nir, red), stats)
    assert tuple(sr.shape[-2:]) == (512, 256) and torch.isfinite(sr).all()
    assert float(sr[..., :256, :].abs().max()) > 0
