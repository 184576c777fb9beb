"""CPU: the one gate of the C ABI.  It follows sifsr._lib.FAMILIES and the include/ directory and holds no list of families of its
own, so a new family -- a header, a row, tests/test_<family>_gpu.py with a CONTRACT -- passes without an edit here, and a header
without a row, a row without a header or a family without contract cases fails.  For each family: the library exports exactly the
declared names under the family's prefix, the binding carries them with the declared types, and every entry point that can write
through a pointer has memory-contract cases in the family's GPU module.  Across families: name sets and prefixes are pairwise
disjoint.  And the binding's own behaviour: which int returns are counts, the ABI version check of lib(), the status check of call().

The per-family tests/test_*_host.py keep the pins that are theirs alone (the row, the literal name lists, the writers dictionaries,
the case counts and shape coverage)."""
import ctypes
import importlib
import itertools
import os
import re
import subprocess
import sys

import pytest

import sifsr  # noqa: F401
from sifsr import _lib as TABLE          # read for the table alone: that needs no library (the L fixture builds a missing one)
from tests.capi_host import L, exported  # noqa: F401  (L is the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = list(TABLE.FAMILIES)
# what the table begins with; rows appended after these need no edit here
FIRST_ROWS = ["core", "mosaic", "baselines", "products", "gaps", "masked", "scores", "lpips", "conserve", "dms", "spectra", "degrade",
              "adapt", "sensor", "ratio", "rloss"]
# family -> the GPU module that holds its CONTRACT table: tests/test_<family>_gpu.py, with one override
GPU_MODULE = {"core": "test_memory_contract_gpu"}
# Entry points that take a non-const pointer but write no device memory.  A new exemption is a deliberate edit, here and in
# test_the_exemptions_are_the_known_ones.
EXEMPT = {
    "core": {
        "sifsr_layer_table": "introspection: fills a HOST int array, no GPU touched",
        "sifsr_model_workspace_regions": "introspection: fills a HOST size_t array, no GPU touched",
        "sifsr_profile_read": "measurement hook: writes two HOST scalars after synchronising its events",
        "sifsr_profile_read_slot": "measurement hook: writes two HOST scalars after synchronising its events",
    },
    "degrade": {"sifsrs_out_shape": "host only: two ints on the host"},
    "ratio": {"sifsrr_geometry": "host only: six ints on the host"},
}
# the entry points whose int return is a count and not a status, and the prefixes sifsr._lib.call() once told them by
COUNT_RETURNING = {
    "sifsr_abi_version", "sifsr_num_params", "sifsr_num_running", "sifsr_layer_table", "sifsr_model_workspace_regions",
    "sifsr_conv3x3_stat_blocks", "sifsr_conv3x3_stat_blocks_wino", "sifsr_conv3x3_bwd16_stat_rows", "sifsr_conv_in_stat_blocks",
    "sifsr_up2x_bwd_stat_rows", "sifsr_huber_partial_blocks", "sifsr_profile_add", "sifsrx_tile_count", "sifsrx_tile_origin",
}
OLD_COUNT_PREFIXES = ("sifsr_abi", "sifsr_num", "sifsr_layer", "sifsr_huber_partial", "sifsr_model_workspace_regions",
                      "sifsr_conv3x3_stat", "sifsr_conv_in_stat", "sifsr_conv3x3_bwd16_stat", "sifsr_profile_add",
                      "sifsr_up2x_bwd_stat", "sifsrx_tile_")


def gpu_module(family):
    return GPU_MODULE.get(family, f"test_{family}_gpu")


def test_the_table_is_the_binding_s(L):
    assert L is TABLE and list(L.FAMILIES)[:16] == FIRST_ROWS and len(L.FAMILIES) >= 16
    assert L.FAMILIES["core"] == ("sifsr_hip.h", "sifsr_") and L.header_path() == L.HEADER
    headers, prefixes = [h for h, _ in L.FAMILIES.values()], [p for _, p in L.FAMILIES.values()]
    on_disk = {f for f in os.listdir(os.path.join(ROOT, "include")) if re.fullmatch(r"sifsr.*\.h", f)}
    no_row, no_header = sorted(on_disk - set(headers)), sorted(set(headers) - on_disk)
    assert not no_row, f"headers under include/ without a row in sifsr._lib.FAMILIES: {no_row}"
    assert not no_header, f"rows of sifsr._lib.FAMILIES whose header is not under include/: {no_header}"
    assert len(set(headers)) == len(headers) == len(set(prefixes)), "two rows of FAMILIES share a header or a prefix"
    for family, (header, prefix) in L.FAMILIES.items():
        assert os.path.samefile(L.header_path(family), os.path.join(ROOT, "include", header)), family
        assert family == "core" or (header == f"sifsr_{family}.h" and re.fullmatch(r"sifsr\w+_", prefix) and prefix != "sifsr_"), \
            f"{family}: the row must be (sifsr_{family}.h, a prefix sifsr?*_ other than sifsr_), not {(header, prefix)}"
        assert os.path.exists(os.path.join(ROOT, "tests", gpu_module(family) + ".py")), \
            f"{family}: tests/{gpu_module(family)}.py, the GPU module that holds the family's CONTRACT, does not exist"
    assert sum(len(L.declared(f)) for f in L.FAMILIES) >= 143


def test_the_exemptions_are_the_known_ones(L):
    assert {f: sorted(names) for f, names in EXEMPT.items()} == {
        "core": ["sifsr_layer_table", "sifsr_model_workspace_regions", "sifsr_profile_read", "sifsr_profile_read_slot"],
        "degrade": ["sifsrs_out_shape"],
        "ratio": ["sifsrr_geometry"],
    }
    assert set(EXEMPT) <= set(L.FAMILIES) and all(reason for names in EXEMPT.values() for reason in names.values())


@pytest.mark.parametrize("family", FAMILIES)
def test_exported_symbols_are_the_declared_ones(L, family):
    prefix = L.FAMILIES[family][1]
    names = L.declared(family)
    stray = [n for n in names if not n.startswith(prefix)]
    assert names and not stray, f"{L.FAMILIES[family][0]} declares {stray} outside its prefix {prefix}"
    if family == "core":
        others = tuple(p for f, (_, p) in L.FAMILIES.items() if f != "core")
        under = {n for n in exported(L.LIB_PATH) if "sifsr_" in n and not n.startswith(others)}
        assert len(names) >= 40 and names == L.declared_symbols()
    else:
        assert not [n for n in names if "sifsr_" in n]                       # outside the core header's export check
        under = {n for n in exported(L.LIB_PATH) if n.startswith(prefix)}
    assert under == set(names), f"exported but not declared, or declared but not exported: {sorted(under ^ set(names))}"
    handle = ctypes.CDLL(L.LIB_PATH)
    assert not [n for n in names if not hasattr(handle, n)]
    assert not [n for n in names if not hasattr(L.lib(), n)]               # the binding carries the family
    for n, (ret, args) in L.parse_header(L.header_path(family)).items():    # ... with the declared types
        fn = getattr(L.lib(), n)
        assert fn.restype is ret and ret in (ctypes.c_int, ctypes.c_size_t), n
        assert list(fn.argtypes) == [t for _, t in args], n                 # non-empty wherever the declaration has arguments
    assert L.call("sifsr_abi_version") == L.ABI_VERSION == 3


def test_families_are_pairwise_disjoint(L):
    for a, b in itertools.permutations(FAMILIES, 2):
        both = set(L.declared(a)) & set(L.declared(b))
        assert not both, f"{sorted(both)} declared by both {L.FAMILIES[a][0]} and {L.FAMILIES[b][0]}"
        stray = [n for n in L.declared(a) if n.startswith(L.FAMILIES[b][1])]
        assert not stray, f"{L.FAMILIES[a][0]} declares {stray} under the prefix of {L.FAMILIES[b][0]}"
        assert not L.FAMILIES[a][1].startswith(L.FAMILIES[b][1]), f"the prefix of {b} is a prefix of the prefix of {a}"
    assert sum(len(L.declared(f)) for f in FAMILIES) == len(set().union(*(L.declared(f) for f in FAMILIES)))


@pytest.mark.parametrize("family", FAMILIES)
def test_every_writing_entry_point_has_a_contract_case(L, family):
    module = gpu_module(family)
    assert os.path.exists(os.path.join(ROOT, "tests", module + ".py")), f"{family}: tests/{module}.py does not exist"
    T = importlib.import_module("tests." + module)
    assert isinstance(getattr(T, "CONTRACT", None), dict), f"tests/{module}.py holds no CONTRACT dictionary"
    writers, exempt, covered = L.writers(family), EXEMPT.get(family, {}), set(T.CONTRACT)
    assert writers and all(writers.values()) and "stream" not in sum(writers.values(), [])
    for name in exempt:
        assert name in writers and name not in covered, name      # the exemption list stays minimal and current
    missing = sorted(set(writers) - covered - set(exempt))
    assert not missing, f"no memory-contract case for {missing}: add a row to CONTRACT in tests/{module}.py"
    stale = sorted(covered - set(writers))
    assert not stale, f"CONTRACT rows for entry points {L.FAMILIES[family][0]} does not declare as writers: {stale}"
    assert covered == set(writers) - set(exempt)
    for name, cases in T.CONTRACT.items():
        assert len(cases) >= 1, name
    if family == "core":
        # the model entry points are exercised through the engine module; its rows must name that module's cases
        src = open(os.path.join(ROOT, "tests", "test_workspace_poison_gpu.py")).read()
        for name in T.ENGINE_ENTRY_POINTS:
            assert name in covered and f'"{name}"' in src, name


def test_count_returning_entry_points(L):
    assert L.COUNT_RETURNING == COUNT_RETURNING and isinstance(L.COUNT_RETURNING, frozenset) and len(COUNT_RETURNING) == 14
    decls = {}
    for family in FAMILIES:
        decls.update(L.parse_header(L.header_path(family)))
    assert all(decls[n][0] is ctypes.c_int for n in COUNT_RETURNING)
    assert {n for n in decls if n.startswith(OLD_COUNT_PREFIXES)} == COUNT_RETURNING


def test_call_raises_on_a_status_from_any_other_entry_point(L):
    """sifsrs_out_shape returns a status (1001 for a shape it refuses) on the host alone; it is not in the count-returning set"""
    assert "sifsrs_out_shape" not in L.COUNT_RETURNING
    oh, ow = ctypes.c_int(), ctypes.c_int()
    assert L.call("sifsrs_out_shape", 40, 52, 2.0, 3, 0, ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oh.value, ow.value) == (23, 29)
    with pytest.raises(L.SifsrError, match="sifsrs_out_shape failed with status 1001"):
        L.call("sifsrs_out_shape", 40, 52, 1.0, 0, 0, ctypes.byref(oh), ctypes.byref(ow))
    assert L.call("sifsrx_tile_count", 100, 64, 0, 0) == 1                   # a non-zero count is no error


def test_lib_refuses_another_abi_version(L):
    """a fresh process, so that nothing is bound yet: the binding expects version 4 of a library that is version 3"""
    code = ("import sifsr\n"
            "from sifsr import _lib as L\n"
            "L.ABI_VERSION = 4\n"
            "try:\n"
            "    L.lib()\n"
            "except L.SifsrError as e:\n"
            "    print('REFUSED:', e)\n"
            "print('bound' if L._lib is not None else 'not bound')\n")
    for given in (False, True):
        env = {k: v for k, v in os.environ.items() if k != "SIFSR_LIB"}
        if given:
            env["SIFSR_LIB"] = L.LIB_PATH
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        said = out.stdout.strip().splitlines()
        assert said[-1] == "not bound" and said[0].startswith("REFUSED:"), out.stdout
        assert L.LIB_PATH in said[0] and "ABI version 3" in said[0] and "needs 4" in said[0]
        assert ("SIFSR_LIB" in said[0]) == given
