"""CPU: the overlapped tile layout of whole-granule prediction (csrc/mosaic.h, restated in sifsr.pipeline.tile_origins) and the
gate of the extension header include/sifsr_mosaic.h -- the same three conditions tests/test_capi_symbols.py and
tests/test_memory_contract_host.py hold include/sifsr_hip.h to, restated for the `sifsrx_` entry points: every declared symbol
is exported and nothing else with the prefix is, every entry point that can write through a pointer has a memory-contract case
in tests/test_mosaic_gpu.py, and the new test sources do not name the barred instructions."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (16, 64)


@pytest.fixture(scope="module")
def L():
    import sifsr  # noqa: F401
    from sifsr import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _sweep():
    for w in WINDOWS:
        for v in (0, 8, w // 2):
            for n in range(w, 5 * w + 1):
                yield n, w, v


def test_layout_properties():
    from sifsr.pipeline import tile_origins
    for n, w, v in _sweep():
        s = w - v
        for cover in (False, True):
            o = tile_origins(n, w, v, cover)
            assert o[0] == 0
            assert all(b > a for a, b in zip(o, o[1:])), (n, w, v, cover, o)          # strictly increasing
            assert all(b - a <= s for a, b in zip(o, o[1:])), (n, w, v, cover, o)     # no gap wider than the stride
            assert all(0 <= a and a + w <= n for a in o)                              # every tile inside the raster
            if cover:
                base = tile_origins(n, w, v, False)
                assert o[-1] == n - w                                                 # the raster is covered to its edge
                assert o == (base if base[-1] + w == n else base + [n - w])           # the regular tiles, plus at most one
            else:
                assert o == [k * s for k in range((n - w) // s + 1)]                  # every regular tile that fits
                assert n - (o[-1] + w) < s
        assert tile_origins(n, w) == list(range(0, n - w + 1, w))                     # defaults: the reference's tiles
    assert tile_origins(1200) == list(range(0, 1137, 64)) and len(tile_origins(1200)) == 18
    assert tile_origins(1200, cover_edges=True)[-2:] == [1088, 1136]
    assert tile_origins(1200, 64, 16, True) == list(range(0, 1105, 48)) + [1136]


def test_layout_agrees_with_the_library(L):
    from sifsr.pipeline import tile_origins
    for n, w, v in _sweep():
        for cover in (0, 1):
            o = tile_origins(n, w, v, bool(cover))
            assert L.call("sifsrx_tile_count", n, w, v, cover) == len(o), (n, w, v, cover)
            assert [L.call("sifsrx_tile_origin", k, n, w, v, cover) for k in range(len(o))] == o, (n, w, v, cover)
            assert L.call("sifsrx_tile_origin", len(o), n, w, v, cover) == -1
            assert L.call("sifsrx_tile_origin", -1, n, w, v, cover) == -1


@pytest.mark.parametrize("n,w,v", [(63, 64, 0), (100, 65, 0), (100, 128, 0), (100, 64, -1), (100, 64, 33), (100, 16, 9), (100, 0, 0)])
def test_invalid_layouts(L, n, w, v):
    from sifsr.pipeline import tile_origins
    for cover in (0, 1):
        assert L.call("sifsrx_tile_count", n, w, v, cover) == 0
        assert L.call("sifsrx_tile_origin", 0, n, w, v, cover) == -1
        with pytest.raises(L.SifsrError):
            tile_origins(n, w, v, bool(cover))


# ---- the gate, restated for include/sifsr_mosaic.h ------------------------------------------------------------------------
def _declarations():
    """{name: [non-const pointer argument names]} of every SIFSR_API declaration of the extension header, parsed as
    sifsr._lib.parse_header does but keeping `const`; the `stream` handle is not memory."""
    text = open(os.path.join(ROOT, "include", "sifsr_mosaic.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"SIFSR_API\s+([\w\s]+?)\s+(\w+)\s*\(([^)]*)\)\s*;", text):
        ptrs = []
        for a in m.group(3).split(","):
            a = " ".join(a.split())
            mm = re.match(r"(.+?)\s*(\w+)$", a)
            if mm and "*" in mm.group(1) and "const" not in mm.group(1) and mm.group(2) != "stream":
                ptrs.append(mm.group(2))
        out[m.group(2)] = ptrs
    return out


def test_every_writing_extension_entry_point_has_a_contract_case(L):
    from tests import test_mosaic_gpu as T
    decl = _declarations()
    assert set(decl) == set(L.declared_extension_symbols()) and len(decl) >= 4
    assert all(n.startswith("sifsrx_") and "sifsr_" not in n for n in decl)      # outside the main header's export check
    writers = {n: p for n, p in decl.items() if p}
    assert writers == {"sifsrx_tiles_prepare": ["x"], "sifsrx_tiles_blend": ["out"]}
    assert "sifsrx_tile_count" in decl and "sifsrx_tile_origin" in decl           # host-only, no pointers: not writers
    missing = sorted(set(writers) - set(T.CONTRACT))
    assert not missing, f"no memory-contract case for {missing}: add a row to CONTRACT in tests/test_mosaic_gpu.py"
    stale = sorted(set(T.CONTRACT) - set(writers))
    assert not stale, f"CONTRACT rows for entry points the extension header does not declare as writers: {stale}"
    assert all(len(cases) >= 1 for cases in T.CONTRACT.values())
    # the main header and the extension do not overlap, and the binding carries both
    assert not set(decl) & set(L.declared_symbols())
    handle = L.lib()
    assert all(hasattr(handle, n) for n in decl)


def test_exported_extension_symbols_are_the_declared_ones(L):
    names = L.declared_extension_symbols()
    handle = ctypes.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(handle, n)]
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("sifsrx_")}
    assert exported == set(names), exported ^ set(names)
    assert L.call("sifsr_abi_version") == 3


def test_new_test_sources_hold_no_barred_instruction_names():
    words = ["store", "buffer_store", "scratch_store", "atomic", "buffer_atomic", "dcache_wb", "dcache_discard"]
    barred = re.compile("|".join("s" + "_" + w for w in words), re.I)      # (assembled, so this file does not hold them either)
    for f in ("test_mosaic_host.py", "test_mosaic_gpu.py"):
        assert not barred.search(open(os.path.join(ROOT, "tests", f)).read()), f
