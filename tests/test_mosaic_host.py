"""CPU: the overlapped tile layout of whole-granule prediction (csrc/mosaic.h, restated in sifsr.pipeline.tile_origins) and the
pins of the extension header include/sifsr_mosaic.h for the `sifsrx_` entry points (the gate itself is tests/test_capi_gate.py):
which entry points write through a pointer and which are host only, and the new test sources do not name the barred
instructions."""
import os
import re

import pytest

from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (16, 64)


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


# ---- the pins of include/sifsr_mosaic.h (the gate itself is tests/test_capi_gate.py) -----------------------------------------
def test_every_writing_extension_entry_point_has_a_contract_case(L):
    decl = L.declared("mosaic")
    assert len(decl) >= 4
    writers = L.writers("mosaic")
    assert writers == {"sifsrx_tiles_prepare": ["x"], "sifsrx_tiles_blend": ["out"]}
    assert "sifsrx_tile_count" in decl and "sifsrx_tile_origin" in decl           # host-only, no pointers: not writers


def test_new_test_sources_hold_no_barred_instruction_names():
    words = ["store", "buffer_store", "scratch_store", "atomic", "buffer_atomic", "dcache_wb", "dcache_discard"]
    barred = re.compile("|".join("s" + "_" + w for w in words), re.I)      # (assembled, so this file does not hold them either)
    for f in ("test_mosaic_host.py", "test_mosaic_gpu.py"):
        assert not barred.search(open(os.path.join(ROOT, "tests", f)).read()), f
