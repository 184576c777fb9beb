"""CPU: patch mining from raw MODIS rasters -- what can be held without a GPU.

  * tests/products_reference.py (the NumPy restatement the GPU tests compare the kernels with, bit for bit) reproduces what the
    reference's own us.split / process_MOD21A1D / process_MOD11A1 / us.compute_NDVI gave on the same seeded inputs
    (tests/golden/golden_products_v1.npz): both counts per window, the accepted [k, row0, col0] lists per coverage and mode, the
    sha256 of every accepted patch, the 60/40 labels and statistics.json,
  * `MinedPatches.assign_split` / `.statistics` (host code: Chan merge of per-patch moments) on the restatement's patches give the
    golden labels and statistics; `MinedDataset` keeps the ModisDatasetB contract,
  * the pins of include/sifsr_products.h for the `sifsrp_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, every entry point that can write through a pointer has a memory-contract case in tests/test_products_gpu.py.

Bounds.  Statistics: maxi / mini exactly; means and standard deviations to 1e-12 relative -- Chan merging of 500 per-patch
float64 moments against np.mean / np.std of the concatenation differs by 7.6e-16 / 5.9e-16, while a one-pass E[x^2] - E[x]^2 loses
about (300 / 5)^2 = 3600 times that."""
import os

import numpy as np
import pytest
import torch

from tests import products_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(ci, m, vi) for ci in range(len(R.CASES)) for m in (0, 1) for vi in range(len(R.COVERAGES))]
STAT_KEYS = ("maxi", "mini", "mean_lst", "std_lst", "mean_ndvi", "std_ndvi")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_products_v1.npz"))


def check_statistics(got, want):
    """got: a statistics dict; want: the golden's six numbers"""
    assert tuple(got) == STAT_KEYS
    assert got["maxi"] == want[0] and got["mini"] == want[1]
    for k, v in zip(STAT_KEYS[2:], want[2:]):
        rel = abs(got[k] - v) / abs(v)
        print(f"{k}: {got[k]!r} vs {v!r}: rel {rel:.2e}")
        assert rel <= 1e-12, k


def test_golden_holds_what_it_should(golden):
    assert int(golden["window"]) == 64 and tuple(golden["coverages"]) == R.COVERAGES
    assert [tuple(c) for c in golden["cases"].tolist()] == list(R.CASES)
    assert tuple(golden["cases"][0][1:]) == (200, 136)
    # the order on the non-square raster is the generator's: rows inner, no ragged step between (128, 0) and (0, 64)
    assert golden["c0_m0_v1_index"].tolist() == [[1, 0, 0], [2, 64, 0], [6, 128, 64]]
    assert golden["c1_m0_v0_index"][:3].tolist() == [[1, 0, 0], [8, 128, 64], [12, 64, 128]]
    assert golden["c0_m0_counts"].shape == (12, 2) and (golden["c0_m0_counts"][6:] == -1).all()
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_products_v1.npz"))
    assert size <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                       if f != "golden_products_v1.npz")


@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_make_case_plants_every_condition(ci):
    seed, h, w = R.CASES[ci]
    case = R.make_case(seed, h, w)                       # (asserts the planted conditions itself)
    want = {"clean", "bad40", "bad41", "zero_den", "both", "qc_only"} if len(case["full"]) >= 6 else {"clean"}
    assert want <= set(case["planted"])
    assert ((case["nir"].astype(np.int32) + case["red"]) == 0).sum() == (0 if len(case["full"]) < 6 else 5 if ci == 0 else 6)


@pytest.mark.parametrize("ci,mode,vi", CONFIGS)
def test_restatement_vs_golden(golden, ci, mode, vi):
    seed, h, w = R.CASES[ci]
    case = R.make_case(seed, h, w)
    counts, index, lst, ndvi, mom = R.mine(case, 64, R.COVERAGES[vi], mode)
    key = f"c{ci}_m{mode}_v{vi}"
    assert np.array_equal(counts, golden[f"c{ci}_m{mode}_counts"]) and counts.dtype == np.int32
    assert np.array_equal(index, golden[key + "_index"])
    assert R.max_bad(R.COVERAGES[vi]) == (0, 40)[vi]
    ks = golden[f"c{ci}_sha_k"].tolist()
    for i, (k, _, _) in enumerate(index):
        assert R.sha(lst[i, 0]) == golden[f"c{ci}_sha_lst"][ks.index(k)]
        assert R.sha(ndvi[i, 0]) == golden[f"c{ci}_sha_ndvi"][ks.index(k)]
    labels = R.assign_split(len(index))
    assert labels.tolist() == golden[key + "_labels"].tolist()
    train = labels == "Train"
    if train.any():
        check_statistics(R.statistics(lst[train], ndvi[train]), golden[key + "_stats"])
    else:
        assert np.isnan(golden[key + "_stats"]).all()


def mined_from_restatement(ci, mode, vi):
    from sifsr import products as P
    seed, h, w = R.CASES[ci]
    _, index, lst, ndvi, mom = R.mine(R.make_case(seed, h, w), 64, R.COVERAGES[vi], mode)
    idx4 = np.concatenate([np.zeros((len(index), 1), np.int64), index.astype(np.int64)], 1)
    return P.MinedPatches(torch.from_numpy(lst), torch.from_numpy(ndvi), idx4, mom, 64)


@pytest.mark.parametrize("ci,mode,vi", [c for c in CONFIGS if c[0] < 2])
def test_host_split_and_statistics_vs_golden(golden, ci, mode, vi):
    import sifsr
    mined = mined_from_restatement(ci, mode, vi)
    key = f"c{ci}_m{mode}_v{vi}"
    assert mined.assign_split().tolist() == golden[key + "_labels"].tolist()
    assert mined.assign_split(seed=42, proportions=(0.6, 0.4)).tolist() == golden[key + "_labels"].tolist()
    if (mined.split == "Train").any():
        check_statistics(mined.statistics("Train"), golden[key + "_stats"])
    else:
        with pytest.raises(sifsr.SifsrError):
            mined.statistics("Train")
    n = len(mined)
    assert sorted(mined.rows("Train").tolist() + mined.rows("Val").tolist()) == list(range(n))


def test_statistics_survive_a_large_offset():
    """the merge is Chan's on centred moments: 500 patches at 300 K with a spread of 5 K, against the concatenation"""
    from sifsr import products as P
    rs = np.random.RandomState(5)
    patches = (300 + 5 * rs.standard_normal((500, 1, 8, 8))).astype(np.float32)
    fine = np.clip(0.4 + 0.3 * rs.standard_normal((500, 1, 32, 32)), -1, 1).astype(np.float32)
    mom = np.array([R.moments_of(a[0], b[0]) for a, b in zip(patches, fine)])
    mined = P.MinedPatches(torch.from_numpy(patches), torch.from_numpy(fine), np.zeros((500, 4), np.int64), mom, 8)
    want = R.statistics(patches, fine)
    check_statistics(mined.statistics(None), [want[k] for k in STAT_KEYS])


def test_mined_dataset_contract():
    import sifsr
    mined = mined_from_restatement(1, 0, 0)
    mined.assign_split()
    tr, va = sifsr.MinedDataset(mined, "Train"), sifsr.dataset.MinedDataset(mined, "Val")
    assert len(tr) == 3 and len(va) == 4 and len(tr) + len(va) == len(mined)
    assert tr.stats == va.stats == mined.statistics("Train")               # the training split's, for both
    lst, lst_up, ndvi = tr[0]
    for a, shape in ((lst, (1, 64, 64)), (lst_up, (1, 256, 256)), (ndvi, (1, 256, 256))):
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == shape
    row = mined.rows("Train")[0]
    st = tr.stats
    assert np.allclose(lst, (mined.lst[row].numpy() - st["mean_lst"]) / st["std_lst"], rtol=1e-6, atol=1e-6)
    assert np.allclose(ndvi, (mined.ndvi[row].numpy() - st["mean_ndvi"]) / st["std_ndvi"], rtol=1e-6, atol=1e-6)
    assert abs(float(lst_up.mean()) - float(lst.mean())) < 0.05
    with pytest.raises(IndexError):
        tr[len(tr)]
    from torch.utils.data import DataLoader
    a, b, c = next(iter(DataLoader(tr, batch_size=2)))
    assert a.shape == (2, 1, 64, 64) and b.shape == (2, 1, 256, 256) and c.shape == (2, 1, 256, 256)
    # the synthetic classes are what they were
    ds = sifsr.ModisDatasetB(length=2)
    assert ds.stats == sifsr.dataset.DEFAULT_STATS and ds[0][0].shape == (1, 64, 64)


def test_public_interface():
    import inspect

    import sifsr
    from sifsr import products as P
    assert sifsr.products is P
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(P.decode) == ["lst_raw", "nir", "red", "clip"]
    assert sig(P.PatchMiner.__init__) == ["self", "window", "coverage", "qc_mode"]
    assert sig(P.PatchMiner.add) == ["self", "lst_raw", "nir", "red", "qc", "granule_id"]
    assert sig(P.MinedPatches.assign_split) == ["self", "seed", "proportions"]
    assert sig(P.MinedPatches.loader) == ["self", "split", "batch", "stats", "shuffle", "seed"]
    d = {k: v.default for k, v in inspect.signature(P.PatchMiner.__init__).parameters.items()}
    assert (d["window"], d["coverage"], d["qc_mode"]) == (64, 0.0, "MOD21A1D")
    assert P.PatchMiner(coverage=0.01).max_bad == 40 and P.PatchMiner().max_bad == 0
    assert P.window_counts(1200, 1200) == (361, 324) and P.window_counts(200, 136) == (12, 6)
    with pytest.raises(ValueError):
        P.PatchMiner(window=30)
    with pytest.raises(ValueError):
        P.PatchMiner(qc_mode="MOD13")
    z = torch.zeros((64, 64), dtype=torch.uint16)
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        P.decode(z, torch.zeros((256, 256), dtype=torch.int16), torch.zeros((256, 256), dtype=torch.int16))
    with pytest.raises(sifsr.SifsrError):
        P.PatchMiner().add(z, torch.zeros((256, 256), dtype=torch.int16), torch.zeros((256, 256), dtype=torch.int16))


# ---- the pins of include/sifsr_products.h (the gate itself is tests/test_capi_gate.py) -----------------------------------------
def test_every_writing_product_entry_point_has_a_contract_case(L):
    from tests import test_products_gpu as T
    assert len(L.declared("products")) == 4
    writers = L.writers("products")
    assert writers == {"sifsrp_decode": ["lst_k", "ndvi"], "sifsrp_census": ["counts"], "sifsrp_select": ["index", "n_accepted"],
                       "sifsrp_gather": ["lst", "ndvi", "moments"]}
    assert all(len(cases) >= 3 for cases in T.CONTRACT.values())
