"""What the memory-contract tests of every header family share (tests/test_memory_contract_gpu.py and the extension
tests/test_*_gpu.py): the GPU fixtures, the case-side view of the allocator `K`, and the one runner `run_contract`.  Importable
without a GPU: tests/test_capi_gate.py imports the GPU modules to read their CONTRACT tables."""
import numpy as np
import pytest
import torch

from tests.memcheck import Arena, Partial, Plain, bit_equal, same_under_all_poisons

F32 = torch.float32


@pytest.fixture(scope="module")
def sifsr():
    import sifsr as pkg
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return pkg


@pytest.fixture(scope="module")
def L(sifsr):
    return sifsr._lib


def S():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # (a copy: shared rasters are read-only)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class K:
    """One run's view of the allocator: seeded operands in, poisoned outputs out."""

    def __init__(self, A, L, seed):
        self.A, self.L, self.seed, self.rs = A, L, seed, np.random.RandomState(seed)

    def i(self, name, *shape, scale=1.0, shift=0.0, dtype=F32):
        t = torch.from_numpy((self.rs.standard_normal(shape) * scale + shift).astype(np.float32)).to(dtype)
        return self.A.input(t, name)

    def pos(self, name, n):
        return self.A.input(torch.from_numpy(self.rs.uniform(0.5, 1.5, n).astype(np.float32)), name)

    def t(self, name, tensor):
        return self.A.input(tensor, name)

    def o(self, name, *shape, dtype=F32):
        return self.A.output(shape, dtype, name)

    def s(self, name, nfloats):
        assert nfloats > 0, name
        return self.A.scratch(int(nfloats) * 4, name)

    def border(self, name, B, H, W, C, dtype=F32):
        """the border scratch: only the image-border pixels are written"""
        b = self.A.output((B, H, W, C), dtype, name)
        m = torch.zeros(1, H, W, 1, dtype=torch.bool)
        m[:, 0] = m[:, -1] = True
        m[:, :, 0] = m[:, :, -1] = True
        init = b.clone()
        return b, (lambda: Partial(b, m, init))


def execute(L, A, make, seed, view=None):
    """One call of the case `make(k) -> (call, {name: tensor | () -> Partial})` on the allocator A: synchronized on both sides, no
    guard byte and no const input changed, the outputs cloned (and passed through `view`)."""
    call, outs = make(K(A, L, seed))
    torch.cuda.synchronize()
    call()
    torch.cuda.synchronize()
    A.check()
    res = {}
    for n, v in outs.items():
        if callable(v):
            p = v()
            res[n] = Partial(p.tensor.clone(), p.written, p.initial)
        else:
            res[n] = v.clone()
    return view(res) if view else res


def run_contract(L, make, seed, capacity=None, view=None):
    """The memory contract of one case: bit-identical and NaN-free under every poison in a guarded arena (of `capacity` bytes), and
    the same bits on ordinary allocations.  `view` reinterprets outputs in which NaN is data before they are compared.  Returns the
    first poison's results."""
    size = {} if capacity is None else {"capacity": capacity}
    first = same_under_all_poisons(lambda p: execute(L, Arena("cuda", poison=p, **size), make, seed, view))
    plain = execute(L, Plain("cuda"), make, seed, view)
    for n, v in first.items():
        ref = plain[n]
        if isinstance(ref, Partial):
            w = ref.written.to(ref.tensor.device).expand_as(ref.tensor)
            v, ref = v[w], ref.tensor[w]
        assert bit_equal(v, ref), f"{n}: the arena run and the ordinary-allocation run differ"
    return first
