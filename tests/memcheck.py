"""A guarded arena for the memory contract of the C ABI (tests/test_memory_contract_*.py, tests/test_workspace_poison_gpu.py).

Every tensor of one call is carved out of ONE backing allocation laid out as [guard | payload | guard | payload | ... | guard]:
payload starts are 256-byte aligned (the workspace's own alignment, 64 floats), a guard begins at the very byte where the payload
before it ends and holds a fixed bit pattern that no kernel produces, and payloads that a kernel is to write start out POISONED.
After the call `Arena.check()` proves that no guard byte and no registered input changed, and `same_under_all_poisons` proves that
no result depends on what the written buffers held before (zeros, NaN, or N(0,1) "stale" values: what a recycled allocator block
holds).  Works on any device; the self-test of the harness runs on CPU tensors.

The guard (>= 1 MiB) is a condition, not a measurement: it is larger than the largest plausible overrun at the shapes used here,
one 16-row tile band of a 16-channel fp32 tensor 256 pixels wide (16 x 256 x 16 x 4 B = 256 KiB)."""
from collections import namedtuple

import torch

ALIGN = 256
MIN_GUARD = 1 << 20
POISONS = ("zeros", "nan", "stale")
# 0xEFBEADDE... as fp32: -1.2e29 / as bf16 pairs: -1.2e29, -2.5e-18 -- nothing a kernel of this library computes
GUARD_PATTERN = (0xDE, 0xAD, 0xBE, 0xEF, 0x5A, 0xC3, 0xA5, 0x3C)
# 0x7FF8 repeated is a quiet NaN read as bf16, as fp32 (0x7FF87FF8) and as float64 alike
NAN_PATTERN = (0xF8, 0x7F)

Partial = namedtuple("Partial", "tensor written initial")   # an output only partly written: bool mask of the written elements


class ContractViolation(AssertionError):
    """kind: 'guard' or 'input'; tensor: the registered name; first / last: offending byte offsets (guards: relative to the end of
    the named payload when `side` is 'after', to its start -- negative -- when 'before'; inputs: within the tensor)."""

    def __init__(self, kind, tensor, side, first, last, count):
        self.kind, self.tensor, self.side, self.first, self.last, self.count = kind, tensor, side, first, last, count
        where = {"after": "guard after", "before": "guard before", "in": "const input"}[side]
        super().__init__(f"{where} '{tensor}' modified: {count} byte(s), first at {first:+d}, last at {last:+d} "
                         f"(byte offsets relative to the payload's {'end' if side == 'after' else 'start'})")


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _tile(pattern, phase, n, device):
    p = torch.tensor(pattern, dtype=torch.uint8, device=device)
    k = len(pattern)
    return p.repeat((n + phase + k - 1) // k + 1)[phase:phase + n]


class Arena:
    def __init__(self, device, guard_bytes=MIN_GUARD, poison="nan", capacity=192 << 20, seed=1234):
        assert guard_bytes >= MIN_GUARD and guard_bytes % ALIGN == 0, "keep the guard at least 1 MiB"
        assert poison in POISONS
        self.device = torch.device(device)
        self.guard_bytes, self.poison, self.capacity = guard_bytes, poison, int(capacity)
        raw = torch.empty(self.capacity + ALIGN, dtype=torch.uint8, device=self.device)
        skew = -raw.data_ptr() % ALIGN                       # (host allocations are only 64-byte aligned)
        self.buf = raw[skew:skew + self.capacity]
        assert self.buf.data_ptr() % ALIGN == 0
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed)
        self._guard_image = _tile(GUARD_PATTERN, 0, guard_bytes + 2 * ALIGN, self.device)   # any guard span, at any phase, is a slice of it
        self._entries = []          # (name, start, nbytes, snapshot or None)
        self._end = 0
        self._write_guard(0, guard_bytes)
        self._end = guard_bytes

    # ---- layout -----------------------------------------------------------------------------------------------------
    def _guard_expected(self, a, b):
        ph = a % len(GUARD_PATTERN)
        return self._guard_image[ph:ph + (b - a)]

    def _write_guard(self, a, b):
        assert b <= self.capacity, f"arena capacity {self.capacity} exceeded ({b}): pass a larger capacity="
        self.buf[a:b] = self._guard_expected(a, b)

    def _carve(self, nbytes, name):
        nbytes = int(nbytes)
        assert nbytes > 0, name
        assert all(name != e[0] for e in self._entries), f"duplicate name {name}"
        start = self._end                                    # (256-byte aligned by construction)
        stop = start + nbytes
        nxt = (stop + self.guard_bytes + ALIGN - 1) // ALIGN * ALIGN   # the guard starts at `stop`, byte-exact
        self._write_guard(stop, nxt)
        self._end = nxt
        return start, self.buf[start:stop]

    def _poison(self, view):
        n = view.numel()
        if self.poison == "zeros":
            view.zero_()
        elif self.poison == "nan":
            view.copy_(_tile(NAN_PATTERN, 0, n, self.device))
        else:
            k = n // 4
            if k:
                view[:4 * k].view(torch.float32).copy_(torch.randn(k, generator=self._gen, device=self.device))
            view[4 * k:].fill_(0x3F)

    @staticmethod
    def _typed(view, shape, dtype):
        return view.view(dtype).view(shape)

    # ---- registration ---------------------------------------------------------------------------------------------
    def input(self, t, name):
        """Copy `t` in; check() asserts that it comes back bit-identical."""
        t = t.detach().contiguous()
        start, view = self._carve(t.numel() * t.element_size(), name)
        view.copy_(_bytes(t.to(self.device)))
        self._entries.append((name, start, view.numel(), view.clone()))
        return self._typed(view, t.shape, t.dtype)

    def inout(self, t, name):
        """Copy `t` in without a snapshot: an argument the header documents as updated in place."""
        t = t.detach().contiguous()
        start, view = self._carve(t.numel() * t.element_size(), name)
        view.copy_(_bytes(t.to(self.device)))
        self._entries.append((name, start, view.numel(), None))
        return self._typed(view, t.shape, t.dtype)

    def output(self, shape, dtype, name):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        start, view = self._carve(n * torch.empty(0, dtype=dtype).element_size(), name)
        self._poison(view)
        self._entries.append((name, start, view.numel(), None))
        return self._typed(view, shape, dtype)

    def scratch(self, nbytes, name):
        """`nbytes` poisoned bytes (uint8 tensor; .view(torch.float32) it to read a reduced result)."""
        start, view = self._carve(nbytes, name)
        self._poison(view)
        self._entries.append((name, start, view.numel(), None))
        return view

    def repoison(self, t, lo=0, hi=None):
        """Fill bytes [lo, hi) of a payload with the current poison again (a workspace range between two calls)."""
        b = t.reshape(-1).view(torch.uint8)
        self._poison(b[lo:b.numel() if hi is None else hi])

    # ---- the check --------------------------------------------------------------------------------------------------
    def _violations(self):
        out = []
        ents = sorted(self._entries, key=lambda e: e[1])
        # guards: [0, first start), then after every payload
        spans = [(0, ents[0][1] if ents else self._end, None, ents[0] if ents else None)]
        for i, e in enumerate(ents):
            stop = e[1] + e[2]
            nxt = ents[i + 1] if i + 1 < len(ents) else None
            spans.append((stop, nxt[1] if nxt else self._end, e, nxt))
        for a, b, prev, nxt in spans:
            bad = (self.buf[a:b] != self._guard_expected(a, b)).nonzero().flatten()
            if bad.numel() == 0:
                continue
            first, last = int(bad[0]), int(bad[-1])
            # attribute to the nearer payload: an overrun of `prev` starts at its end, an underrun of `nxt` ends at its start
            if prev is not None and (nxt is None or first <= (b - a) - 1 - last):
                out.append(ContractViolation("guard", prev[0], "after", first, last, int(bad.numel())))
            else:
                out.append(ContractViolation("guard", nxt[0], "before", first - (b - a), last - (b - a), int(bad.numel())))
        for name, start, nbytes, snap in ents:
            if snap is None:
                continue
            bad = (self.buf[start:start + nbytes] != snap).nonzero().flatten()
            if bad.numel():
                out.append(ContractViolation("input", name, "in", int(bad[0]), int(bad[-1]), int(bad.numel())))
        return out

    def check(self):
        """Every guard bit-identical to the pattern, every registered input bit-identical to its snapshot."""
        v = self._violations()
        if len(v) == 1:
            raise v[0]
        if v:
            err = ContractViolation(v[0].kind, v[0].tensor, v[0].side, v[0].first, v[0].last, v[0].count)
            err.args = ("; ".join(str(e) for e in v),)
            err.all = v
            raise err


class Plain:
    """The same registration interface on ordinary allocations (no guards): the run an arena run is compared with bit for bit, so
    that carving the tensors out of one block cannot change which kernel path runs."""
    poison = "nan"

    def __init__(self, device):
        self.device = torch.device(device)

    def input(self, t, name):
        return t.detach().contiguous().to(self.device).clone()

    inout = input

    def output(self, shape, dtype, name):
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (shape,)
        n = 1
        for s in shape:
            n *= int(s)
        raw = _tile(NAN_PATTERN, 0, n * torch.empty(0, dtype=dtype).element_size(), self.device)
        return raw.view(dtype).view(shape)

    def scratch(self, nbytes, name):
        return _tile(NAN_PATTERN, 0, int(nbytes), self.device).clone()

    def check(self):
        pass


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


def _has_nan(t):
    return bool(t.is_floating_point() and torch.isnan(t).any())


def same_under_all_poisons(run, poisons=POISONS):
    """run(poison) -> {name: tensor | Partial}.  All results bit-identical across the poisons (NaNs compared by bits) and NaN-free;
    of a Partial only the written elements, and its other elements must still hold what the buffer was poisoned with.  Returns the
    first poison's results (Partial -> its tensor) for further comparison."""
    results = {}
    for p in poisons:
        res = run(p)
        clean = {}
        for name, v in res.items():
            if isinstance(v, Partial):
                w = v.written.to(v.tensor.device).expand_as(v.tensor)
                assert bit_equal(v.tensor[~w], v.initial[~w]), f"{name}: written outside its declared part (poison {p})"
                assert not _has_nan(v.tensor[w]), f"{name}: NaN in its written part under poison {p}"
                clean[name] = v.tensor.clone()
                clean[name][~w] = 0
            else:
                assert not _has_nan(v), f"{name}: NaN under poison {p}: an unwritten or poisoned value reached the result"
                clean[name] = v
        results[p] = clean
    first = results[poisons[0]]
    for p in poisons[1:]:
        assert results[p].keys() == first.keys()
        for name in first:
            assert bit_equal(first[name], results[p][name]), \
                f"{name}: differs between poison {poisons[0]} and {p}: the call read memory it had not written"
    return first
