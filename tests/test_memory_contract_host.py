"""CPU: the test of the test.  tests/memcheck.py must flag every class of memory-contract bug it exists for -- shown here on fake
"kernels" written in Python against CPU tensors from the arena, so no real kernel has to be broken (or a GPU provoked) to prove
it -- and the contract table of tests/test_memory_contract_gpu.py must cover every entry point of include/sifsr_hip.h that can
write through a pointer."""
import os
import re

import pytest
import torch

from tests.capi_host import L  # noqa: F401  (the fixture)
from tests.memcheck import ALIGN, POISONS, Arena, ContractViolation, Partial, Plain, bit_equal, same_under_all_poisons

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 16 << 20
ROWS, COLS = 6, 40          # a "partials" scratch of 6 rows; payload sizes that are NOT multiples of 256 bytes


def _setup(poison):
    """The arguments of one fake operator: const input x, output y, a partials scratch, a reduced result."""
    A = Arena("cpu", poison=poison, capacity=CAP)
    x = A.input(torch.arange(1, COLS + 1, dtype=torch.float32), "x")
    y = A.output((COLS,), torch.float32, "y")
    part = A.scratch(ROWS * COLS * 4, "partials").view(torch.float32).view(ROWS, COLS)
    total = A.output((COLS,), torch.float32, "total")
    return A, x, y, part, total


def _good_kernel(x, y, part, total, rows_written=ROWS):
    y.copy_(2 * x)
    for r in range(rows_written):          # one partials row per "workgroup" ...
        part[r].copy_(x * (r + 1))
    total.copy_(part.sum(0))               # ... and a reduction over ALL rows


def _raw(A, t, delta):
    """the arena byte at `delta` bytes from the start of t's payload (what a kernel with a wrong index reaches)"""
    off = t.data_ptr() - A.buf.data_ptr() + delta
    return A.buf[off:off + 4].view(torch.float32)


def test_layout_alignment_guards_and_poisons():
    for p in POISONS:
        A, x, y, part, total = _setup(p)
        for t in (x, y, part, total):
            assert t.data_ptr() % ALIGN == 0
        assert y.data_ptr() - (x.data_ptr() + x.numel() * 4) >= 1 << 20      # a full guard between neighbours
        A.check()                                                           # untouched: passes
        if p == "zeros":
            assert (y == 0).all() and (part == 0).all()
        elif p == "nan":
            assert torch.isnan(y).all() and torch.isnan(part).all()
            assert torch.isnan(part.reshape(-1).view(torch.bfloat16).float()).all()       # NaN for bf16 tensors too ...
            assert torch.isnan(part.reshape(-1).view(torch.float64)).all()                # ... and for the float64 coefficients
        else:
            assert 0.5 < float(y.std()) < 2.0 and 0.5 < float(part.std()) < 2.0 and not torch.isnan(part).any()
    with pytest.raises(AssertionError):
        Arena("cpu", guard_bytes=1 << 16, capacity=CAP)


def test_well_behaved_kernel_passes():
    def run(p):
        A, x, y, part, total = _setup(p)
        _good_kernel(x, y, part, total)
        A.check()
        return {"y": y.clone(), "total": total.clone()}
    res = same_under_all_poisons(run)
    P = Plain("cpu")
    x = P.input(torch.arange(1, COLS + 1, dtype=torch.float32), "x")
    y, total = P.output((COLS,), torch.float32, "y"), P.output((COLS,), torch.float32, "total")
    part = P.scratch(ROWS * COLS * 4, "partials").view(torch.float32).view(ROWS, COLS)
    _good_kernel(x, y, part, total)
    assert bit_equal(res["y"], y) and bit_equal(res["total"], total)


@pytest.mark.parametrize("side", ["after", "before"])
def test_write_one_element_past_an_output_is_flagged(side):
    A, x, y, part, total = _setup("nan")
    _good_kernel(x, y, part, total)
    _raw(A, y, COLS * 4 if side == "after" else -4)[0] = 1.0
    with pytest.raises(ContractViolation) as e:
        A.check()
    v = e.value
    assert (v.kind, v.tensor, v.side) == ("guard", "y", side) and "'y'" in str(v)
    assert (v.first, v.last) == ((0, 3) if side == "after" else (-4, -1))


def test_write_into_the_far_end_of_a_guard_is_flagged():
    A, x, y, part, total = _setup("stale")
    _good_kernel(x, y, part, total)
    far = (1 << 20) - 4                      # the last word of the last guard, a whole tile band past `total`
    _raw(A, total, COLS * 4 + far)[0] = 0.0
    with pytest.raises(ContractViolation) as e:
        A.check()
    assert (e.value.kind, e.value.tensor, e.value.side) == ("guard", "total", "after")
    assert e.value.first >= far and e.value.last <= far + ALIGN


def test_modified_const_input_is_flagged():
    A, x, y, part, total = _setup("zeros")
    _good_kernel(x, y, part, total)
    x[7] += 1.0
    with pytest.raises(ContractViolation) as e:
        A.check()
    assert (e.value.kind, e.value.tensor) == ("input", "x") and 28 <= e.value.first <= e.value.last <= 31


def test_unwritten_scratch_row_that_is_reduced_is_flagged():
    """The stale-read class: the last 'workgroup' leaves its row unwritten and the reduction sums all rows.  Under zeros the
    result is even right; it differs under stale values and is NaN under NaN."""
    def run(p):
        A, x, y, part, total = _setup(p)
        _good_kernel(x, y, part, total, rows_written=ROWS - 1)
        A.check()                            # (no guard or input is touched: only the poisons can see it)
        return {"y": y.clone(), "total": total.clone()}
    with pytest.raises(AssertionError, match="total"):
        same_under_all_poisons(run)
    with pytest.raises(AssertionError, match="total"):
        same_under_all_poisons(run, poisons=("zeros", "stale"))      # also without the NaN: by bit comparison alone
    ok = run("zeros")
    assert torch.equal(ok["total"], torch.arange(1, COLS + 1, dtype=torch.float32) * 15)   # zeros hide it


def test_partially_written_output():
    """The documented partial output (the border scratch): the written part is compared, the rest must still hold the poison."""
    mask = torch.zeros(COLS, dtype=torch.bool)
    mask[0] = mask[-1] = True

    def run(p, stray=False):
        A = Arena("cpu", poison=p, capacity=CAP)
        b = A.output((COLS,), torch.float32, "border")
        init = b.clone()
        b[0], b[-1] = 3.0, 4.0
        if stray:
            b[5] = 1.0
        A.check()
        return {"border": Partial(b.clone(), mask, init)}
    res = same_under_all_poisons(run)
    assert res["border"][0] == 3.0 and res["border"][-1] == 4.0
    with pytest.raises(AssertionError, match="border"):
        same_under_all_poisons(lambda p: run(p, stray=True))


# ---- coverage gate -------------------------------------------------------------------------------------------------------
def test_every_writing_entry_point_has_a_contract_case(L):
    """what the header's writers are; that each has a row in CONTRACT (or an exemption with its reason) is held for every header
    family by tests/test_capi_gate.py"""
    writers = L.writers("core")
    assert len(L.declared("core")) >= 80 and len(writers) >= 55, (len(L.declared("core")), len(writers))
    assert writers["sifsr_bn_relu_bwd_coef"][0] == "g" and "workspace" in writers["sifsr_model_forward"]
    assert "sifsr_conv3x3_stat_blocks" not in writers and "sifsr_huber_bwd" in writers


def test_new_test_sources_hold_no_barred_instruction_names():
    words = ["store", "buffer_store", "scratch_store", "atomic", "buffer_atomic", "dcache_wb", "dcache_discard"]
    barred = re.compile("|".join("s" + "_" + w for w in words), re.I)      # (assembled, so this file does not hold them either)
    for f in ("memcheck.py", "test_memory_contract_host.py", "test_memory_contract_gpu.py", "test_workspace_poison_gpu.py"):
        assert not barred.search(open(os.path.join(ROOT, "tests", f)).read()), f
