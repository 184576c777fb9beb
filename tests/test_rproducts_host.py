"""CPU: patch mining at a ratio -- what can be held without a GPU.

  * tests/rproducts_reference.py (the NumPy restatement the GPU tests compare the kernels with, bit for bit) at hr = 4 ws equals
    tests/products_reference.py -- which tests/test_products_host.py pins to the reference's recorded results -- on every one of
    its cases: counts, index, both patch arrays and the moments.  The reference has no other ratio; this is the anchor.
  * `patch_counts` and `expand_valid` of the restatement against a brute-force loop over the HR pixels,
  * the table of trainable pairs from the integer form of the sensor model's geometry (include/sifsr_degrade.h), and the
    library's own answer where it is built,
  * the pins of include/sifsr_rproducts.h (the gate itself is tests/test_capi_gate.py) and the error codes found before a launch,
  * `MinedPatches`: the default `hr`, `statistics()` at x4 bit for bit today's formula, the NDVI count at (8, 24).

Bounds.  Every comparison is for equality except the statistics, which use `check_statistics` of tests/test_products_host.py
(maxi / mini exactly, means and standard deviations to 1e-12 relative; argued there)."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from tests import products_reference as R4
from tests import rproducts_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)
from tests.test_products_host import STAT_KEYS, check_statistics

TRAINABLE = ((8, 24), (16, 40), (12, 24), (8, 32), (12, 40), (24, 56), (48, 160), (64, 160), (64, 192))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(R4.CASES)))
def test_restatement_at_x4_is_the_products_restatement(ci):
    seed, h, w = R4.CASES[ci]
    c4 = R4.make_case(seed, h, w)
    case = dict(c4, ws=64, hr=256)
    assert R.fine_shape(h, w, 64, 256) == (4 * h, 4 * w) and R.ratio_of(64, 256) == (4, 1)
    for mode in (0, 1):
        for cov in R4.COVERAGES:
            want = R4.mine(c4, 64, cov, mode)
            got = R.mine(case, cov, mode)
            for a, b, name in zip(got, want, ("counts", "index", "lst", "ndvi", "moments")):
                assert a.dtype == b.dtype and a.shape == b.shape, name
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), name
    assert len(R.mine(case, R4.COVERAGES[1], 0)[1]) >= 1


@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_make_case_plants_every_condition(ci):
    seed, h, w, ws, hr = R.CASES[ci]
    case = R.make_case(seed, h, w, ws, hr)                # (asserts the planted conditions itself)
    nfull = len(case["full"])
    assert nfull == (12, 2, 4, 6, 16, 1)[ci] and len(R.windows(h, w, ws)) == (20, 6, 6, 12, 20, 1)[ci]
    assert tuple(case["planted"]) == R.PLANTED[:min(nfull, 6)]
    assert case["nir"].shape == R.fine_shape(h, w, ws, hr) and case["nir"].shape[1] == (84, 45, 80, 76, 128, 192)[ci]
    assert R.max_bad(0.05, 8) == 3 and case["max_bad"] == R.max_bad(0.05, ws)
    if nfull >= 9:
        assert len(R.mine(case, 0.0, 0)[1]) >= 3
    counts, index, lst, ndvi, mom = R.mine(case, 0.05, 0)
    assert lst.shape == (len(index), 1, ws, ws) and ndvi.shape == (len(index), 1, hr, hr) and np.abs(ndvi).max() <= 1.0
    assert (mom[:, 0] == ws * ws).all() and len(index) >= 1


def brute_counts(valid, hr):
    ws = valid.shape[-1]
    out = np.zeros((len(valid), 2), np.int64)
    for n, v in enumerate(valid):
        out[n, 0] = int((v != 0).sum())
        for Y in range(hr):
            for X in range(hr):
                out[n, 1] += int(v[Y * ws // hr, X * ws // hr] != 0)
    return out


@pytest.mark.parametrize("ws,hr", [(8, 24), (16, 40), (12, 40)])
def test_patch_counts_and_expand_valid_vs_brute_force(ws, hr):
    rs = np.random.RandomState(ws + hr)
    valid = (rs.uniform(size=(5, ws, ws)) < 0.6).astype(np.uint8) * rs.randint(1, 256, (5, ws, ws)).astype(np.uint8)   # any non-zero byte
    valid[3], valid[4] = 0, 1
    want = brute_counts(valid, hr)
    got = R.patch_counts(valid, hr)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert want[3].tolist() == [0, 0] and want[4].tolist() == [ws * ws, hr * hr]
    if (ws, hr) == (16, 40):                               # a cell holds 2 or 3 pixels per axis
        one = np.zeros((2, 16, 16), np.uint8)
        one[0, 0, 0], one[1, 1, 1] = 1, 1
        assert R.patch_counts(one, 40).tolist() == [[1, 9], [1, 4]]
    H, W = hr, hr + 8 if (ws, hr) == (8, 24) else hr
    ex = R.expand_valid(valid, (H, W))
    assert ex.dtype == np.uint8 and ex.shape == (5, H, W) and set(np.unique(ex)) <= {0, 1}
    for Y in range(H):
        for X in range(W):
            assert np.array_equal(ex[:, Y, X], (valid[:, Y * ws // H, X * ws // W] != 0).astype(np.uint8))
    if W == hr:
        assert np.array_equal(ex.reshape(5, -1).sum(1), want[:, 1])


# ---- 2. the trainable pairs ------------------------------------------------------------------------------------------------------
def lr_side(hr, ws):
    """the side the sensor model at factor hr / ws leaves of hr pixels (include/sifsr_degrade.h: hw = ceil(factor), np = n + 2 hw,
    on = floor(np / factor), the crop cuts floor(hw / factor) on each side), in integers"""
    hw = -(-hr // ws)
    return (hr + 2 * hw) * ws // hr - 2 * (hw * ws // hr)


def is_trainable(ws, hr):
    tile = 1 <= ws <= 64 and hr % 8 == 0 and 24 <= hr <= 256 and ws < hr <= 16 * ws        # ratio.geometry of one tile
    return tile and hr <= 8 * ws and lr_side(hr, ws) == ws


def test_the_trainable_pairs():
    assert all(is_trainable(ws, hr) for ws, hr in TRAINABLE)
    assert not is_trainable(20, 24) and lr_side(24, 20) == 21
    assert not is_trainable(16, 20) and not is_trainable(8, 72) and not is_trainable(65, 256) and not is_trainable(8, 28)
    assert all(is_trainable(ws, hr) for _, _, _, ws, hr in R.CASES)


def test_the_library_agrees_on_the_pairs(L):
    """`rproducts.trainable` is host only (sifsrr_geometry and sifsrs_out_shape, the two calls the C entry points make)"""
    from sifsr import rproducts
    n = 0
    for ws in (4, 8, 9, 12, 16, 20, 24, 48, 64, 65):
        for hr in range(8, 272, 4):
            try:
                got = rproducts.trainable(ws, hr) == R.ratio_of(ws, hr)
            except L.SifsrError:
                got = False
            assert got == is_trainable(ws, hr), (ws, hr)
            n += got
    assert n >= 60
    for ws, hr in TRAINABLE:
        assert rproducts.trainable(ws, hr) == R.ratio_of(ws, hr)
    for (ws, hr), word in (((20, 24), "sensor model"), ((8, 72), "fused loss"), ((8, 28), "ratio.geometry"), ((65, 256), "ratio.geometry")):
        with pytest.raises(L.SifsrError, match=word):
            rproducts.trainable(ws, hr)
        with pytest.raises(L.SifsrError, match=word):
            rproducts.PatchMiner(ws, hr)
    with pytest.raises(L.SifsrError, match="multiple of 4"):
        rproducts.PatchMiner(9, 24)                                            # trainable, but the selection cannot take it


# ---- 3. the pins of include/sifsr_rproducts.h (the gate itself is tests/test_capi_gate.py) -------------------------------------------
def test_the_row_and_the_contract_cases(L):
    from tests import test_rproducts_gpu as T
    assert L.FAMILIES["rproducts"] == ("sifsr_rproducts.h", "sifsrn_") and list(L.FAMILIES)[17] == "rproducts" and len(L.FAMILIES) == 18
    assert L.declared("rproducts") == ["sifsrn_census", "sifsrn_decode", "sifsrn_expand_valid", "sifsrn_gather", "sifsrn_patch_counts"]
    writers = L.writers("rproducts")
    assert writers == {"sifsrn_decode": ["lst_k", "ndvi"], "sifsrn_census": ["counts"], "sifsrn_gather": ["lst", "ndvi", "moments"],
                       "sifsrn_patch_counts": ["counts"], "sifsrn_expand_valid": ["out"]}
    assert sorted(T.CONTRACT) == sorted(writers) and all(len(cases) >= 3 for cases in T.CONTRACT.values())
    assert "sifsrn_select" not in L.declared("rproducts") and "sifsrp_select" in L.declared("products")    # one selection
    assert L.call("sifsr_abi_version") == 3


def test_errors_found_before_a_launch(L):
    h = L.lib()
    one, odd2, odd4 = ctypes.c_void_p(4096), ctypes.c_void_p(4097), ctypes.c_void_p(4100)
    S, A = 1001, 1002
    # decode: (lst_raw, nir, red, lst_k, ndvi, h, w, fh, fw, clip, stream)
    assert h.sifsrn_decode(None, one, one, one, one, 8, 8, 24, 24, 0, None) == A
    assert h.sifsrn_decode(one, one, one, one, None, 8, 8, 24, 24, 0, None) == A
    assert h.sifsrn_decode(one, one, one, one, one, 8, 8, 24, 24, 2, None) == A
    assert h.sifsrn_decode(one, one, one, odd4, one, 8, 8, 24, 24, 0, None) == A            # float outputs: 16 bytes
    assert h.sifsrn_decode(one, odd2, one, one, one, 8, 8, 24, 24, 0, None) == A            # int16: 2 bytes
    assert h.sifsrn_decode(one, one, one, one, one, 8, 8, 24, 16, 0, None) == S             # unequal ratios
    assert h.sifsrn_decode(one, one, one, one, one, 8, 8, 4, 4, 0, None) == S               # a fine raster that is coarser
    assert h.sifsrn_decode(one, one, one, one, one, 0, 8, 0, 24, 0, None) == S
    assert h.sifsrn_decode(one, one, one, one, one, 8, 8, 136, 136, 0, None) == S           # above x16
    # census: (lst_raw, qc, nir, red, counts, h, w, window, hr, qc_mode, stream)
    assert h.sifsrn_census(one, None, one, one, None, 40, 28, 8, 24, 0, None) == A
    assert h.sifsrn_census(one, None, one, one, one, 40, 28, 8, 24, 1, None) == A           # mode 1 needs qc
    assert h.sifsrn_census(one, one, one, one, one, 40, 28, 8, 24, 2, None) == A
    assert h.sifsrn_census(one, one, odd2, one, one, 40, 28, 8, 24, 0, None) == A
    assert h.sifsrn_census(one, one, one, one, one, 40, 28, 20, 24, 0, None) == S           # not trainable: the crop leaves 21
    assert h.sifsrn_census(one, one, one, one, one, 35, 18, 16, 40, 0, None) == S           # h no multiple of q = 2
    assert h.sifsrn_census(one, one, one, one, one, 34, 14, 16, 40, 0, None) == S           # w < window
    assert h.sifsrn_census(one, one, one, one, one, 16386, 18, 16, 40, 0, None) == S
    # gather: (lst_raw, nir, red, index, n_accepted, lst, ndvi, moments, h, w, window, hr, cap, stream)
    g = lambda **kw: h.sifsrn_gather(*[kw.get(n, one) for n in ("lst_raw", "nir", "red", "index", "n", "lst", "ndvi", "moments")],
                                     kw.get("h", 40), kw.get("w", 28), kw.get("ws", 8), kw.get("hr", 24), kw.get("cap", 12), None)
    assert g(red=None) == A and g(moments=None) == A and g(ndvi=odd4) == A and g(lst=odd4) == A and g(nir=odd2) == A
    assert g(cap=11) == S and g(ws=20) == S and g(h=41, ws=16, hr=40) == S and g(hr=28) == S
    # patch_counts: (valid, counts, N, window, hr, stream); expand_valid: (valid, out, B, h, w, H, W, stream)
    assert h.sifsrn_patch_counts(None, one, 1, 8, 24, None) == A and h.sifsrn_patch_counts(one, odd4, 1, 8, 24, None) == A
    assert h.sifsrn_patch_counts(one, one, 0, 8, 24, None) == S and h.sifsrn_patch_counts(one, one, 1, 8, 7, None) == S
    assert h.sifsrn_patch_counts(one, one, 1, 0, 24, None) == S
    assert h.sifsrn_expand_valid(one, None, 1, 8, 8, 24, 24, None) == A
    assert h.sifsrn_expand_valid(one, one, 0, 8, 8, 24, 24, None) == S and h.sifsrn_expand_valid(one, one, 1, 8, 8, 7, 24, None) == S
    assert h.sifsrn_expand_valid(one, one, 65536, 8, 8, 24, 24, None) == S and h.sifsrn_expand_valid(one, one, 1, 8, 8, 24, 16385, None) == S


# ---- 4. MinedPatches carries hr --------------------------------------------------------------------------------------------------
def handmade(n, ws, hr, seed):
    rs = np.random.RandomState(seed)
    lst = (300 + 5 * rs.standard_normal((n, 1, ws, ws))).astype(np.float32)
    ndvi = np.clip(0.4 + 0.3 * rs.standard_normal((n, 1, hr, hr)) + 0.1 * rs.standard_normal((n, 1, 1, 1)), -1, 1).astype(np.float32)
    mom = np.array([R.moments_of(a[0], b[0]) for a, b in zip(lst, ndvi)])
    return lst, ndvi, mom


def test_statistics_at_x4_are_todays_bits():
    from sifsr import products as P
    lst, ndvi, mom = handmade(37, 8, 32, 3)
    for hr in (None, 32):
        mined = P.MinedPatches(torch.from_numpy(lst), torch.from_numpy(ndvi), np.zeros((37, 4), np.int64), mom, 8, hr)
        assert mined.hr == 32 and mined.window == 8
        got = mined.statistics(None)
        n, mean_l, m2_l = P.merge_moments(mom[:, 0], mom[:, 1], mom[:, 2])                 # the formula as it stood before `hr`
        nn, mean_n, m2_n = P.merge_moments(16.0 * mom[:, 0], mom[:, 5], mom[:, 6])
        want = {"maxi": float(mom[:, 4].max()), "mini": float(mom[:, 3].min()), "mean_lst": float(mean_l),
                "std_lst": float(math.sqrt(m2_l / n)), "mean_ndvi": float(mean_n), "std_ndvi": float(math.sqrt(m2_n / nn))}
        assert got == want and tuple(got) == STAT_KEYS
    assert P.MinedPatches(None, None, np.zeros((0, 4), np.int64), np.zeros((0, 8)), 64).hr == 256
    assert list(inspect.signature(P.MinedPatches.__init__).parameters) == ["self", "lst", "ndvi", "index", "moments", "window", "hr"]
    assert inspect.signature(P.MinedPatches.__init__).parameters["hr"].default is None


def test_the_ndvi_count_follows_hr():
    """(8, 24): 576 NDVI pixels per patch, not 16 * 64; with the x4 count the between-patch part of the variance is weighed
    1024 / 576 times too heavy, far outside the bound"""
    import sifsr
    from sifsr import products as P
    lst, ndvi, mom = handmade(41, 8, 24, 4)
    mined = P.MinedPatches(torch.from_numpy(lst), torch.from_numpy(ndvi), np.zeros((41, 4), np.int64), mom, 8, 24)
    want = R.statistics(lst, ndvi)
    check_statistics(mined.statistics(None), [want[k] for k in STAT_KEYS])
    wrong = P.MinedPatches(torch.from_numpy(lst), torch.from_numpy(ndvi), np.zeros((41, 4), np.int64), mom, 8).statistics(None)
    assert abs(wrong["std_ndvi"] - want["std_ndvi"]) / want["std_ndvi"] > 1e-6              # the count matters on this data
    mined.assign_split()
    with pytest.raises(sifsr.SifsrError, match="x4"):
        sifsr.MinedDataset(mined, "Train")                                                  # the host path is x4 only


def test_public_interface():
    import sifsr
    from sifsr import products, rloss, rproducts
    assert sifsr.rproducts is rproducts
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E_ = inspect.Parameter.empty
    assert sig(rproducts.decode) == [("lst_raw", E_), ("nir", E_), ("red", E_), ("clip", False)]
    assert sig(rproducts.PatchMiner.__init__) == [("self", E_), ("window", E_), ("hr", E_), ("coverage", 0.0), ("qc_mode", "MOD21A1D")]
    assert sig(rproducts.PatchMiner.add) == sig(products.PatchMiner.add)
    assert sig(rloss.eval_step) == [("model", E_), ("lst", E_), ("lst_up", E_), ("ndvi", E_), ("stats", E_), ("alpha", E_), ("gamma", E_),
                                    ("factor", E_), ("kind", "sr2"), ("valid", None), ("counts", None)]
    assert sig(rloss.train_epoch) == [("model", E_), ("loader", E_), ("optimizer", E_), ("stats", E_), ("alpha", E_), ("gamma", E_),
                                      ("factor", E_), ("kind", "sr2"), ("device", "cuda"), ("with_metrics", True), ("masked_metrics", False)]
    assert sig(rloss.fit) == [("model", E_), ("train_loader", E_), ("val_loader", E_), ("n_epochs", E_), ("optimizer", E_), ("stats", E_),
                              ("alpha", E_), ("gamma", E_), ("factor", E_), ("kind", "sr2"), ("checkpoint", None), ("masked_metrics", False)]
    assert rproducts.PatchMiner(8, 24, 0.05).max_bad == 3 and rproducts.PatchMiner(64, 192).max_bad == 0
    z = torch.zeros((8, 8), dtype=torch.uint16)
    f = torch.zeros((24, 24), dtype=torch.int16)
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        rproducts.decode(z, f, f)
    with pytest.raises(sifsr.SifsrError):
        rproducts.PatchMiner(8, 24).add(z, f, f)
    for text in (sifsr.ratio.__doc__, rloss.__doc__):
        assert "mining patches at a ratio" not in text
