"""CPU: the numpy / scipy restatement of the per-pair ASTER evaluation table (tests/eval_reference.py)
reproduces the committed golden numbers of tests/golden/make_golden_eval.py (real ASTER crops, reference-pinned GSSIM and
get_output_ftm), and its percentile / strata conventions are the reference's."""
import os

import numpy as np
import pytest

from tests import eval_reference as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_eval_v1.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_restatement_reproduces_golden(gold):
    assert tuple(gold["names"]) == E.METRIC_NAMES
    for i in range(len(gold["kinds"])):
        row, ex = E.metrics(gold[f"a{i}"], gold[f"b{i}"])
        np.testing.assert_array_equal(row, gold[f"metrics{i}"])
        assert np.float32(ex["q25"]) == gold[f"q{i}"][0] and np.float32(ex["q75"]) == gold[f"q{i}"][1]
        assert tuple(ex["counts"]) == tuple(gold[f"counts{i}"])


def test_golden_cases_are_real_crops_with_ties(gold):
    a = gold["a0"]
    assert a.dtype == np.float32 and (a > 0).all() and 250 < float(a.mean()) < 340
    g = E.gradient_map(a)
    assert g.size - np.unique(g).size > 100
    row = gold[f"metrics{list(gold['kinds']).index('same')}"]
    assert row[0] == np.inf and row[1] == 1.0 and row[2] == row[3] == row[4] == row[5] == row[7] == 0.0


def test_strata_divide_by_n():
    """model_perf_aster_formatds.py:385-386: ``filter((0.0).__ne__, ...)`` keeps every np.float32 element (float.__ne__ of
    an np.float32 is NotImplemented, which is truthy), so the zeroed entries stay in the mean."""
    vals = list(np.array([0.0, 1.0, 0.0, 4.0], np.float32))
    assert len(list(filter((0.0).__ne__, vals))) == 4
    a = np.arange(256, dtype=np.float32).reshape(16, 16) % 7
    b = a + 1
    g = E.gradient_map(a)
    q25, q75, lo, mid, hi, counts = E.strata(a, b, g)
    n = a.size
    assert abs(lo - np.sqrt(counts[0] / n)) < 1e-6 and abs(hi - np.sqrt(counts[2] / n)) < 1e-6
    assert abs(mid - np.sqrt(counts[1] / n)) < 1e-6
