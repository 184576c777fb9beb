"""What the CPU tests of the C ABI share: the host-flavoured binding fixture and the library's exported names."""
import functools
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def L():
    """sifsr._lib, with the library built if it is missing (no GPU is needed to build or to load it)"""
    import sifsr  # noqa: F401
    from sifsr import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


@functools.lru_cache(maxsize=None)
def exported(lib_path):
    """the names the library defines in its dynamic symbol table as functions: one `nm` run per library"""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    return frozenset(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
