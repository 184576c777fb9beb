"""ctypes binding of libsifsr_hip.so.

The signatures are parsed from the headers under ``include/`` -- the headers are the single source of truth for the C ABI.
``FAMILIES`` below is the one table of them: ``include/sifsr_hip.h`` (``core``, prefix ``sifsr_``) and its extensions, one header
and one symbol prefix each.  ``tests/test_capi_gate.py`` checks, for every row, that the library exports exactly the declared
symbols and that every writing entry point has memory-contract cases.
There is NO fallback: if the library is missing, of another ABI version, or a call fails, we raise.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch  # noqa: F401  (must be imported first: the library binds to the libamdhip64 torch loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
# The C ABI: family -> (header under include/, symbol prefix).  A family is ONE row: `core` is the main header, every other row an
# extension in the same declaration style whose memory-contract cases are the CONTRACT of tests/test_<family>_gpu.py.  lib() binds
# every row; tests/test_capi_gate.py gates every row against the built library and the include/ directory, so a new family adds a
# header, a row and that GPU module, and no gate of its own.
FAMILIES = {
    "core": ("sifsr_hip.h", "sifsr_"),
    "mosaic": ("sifsr_mosaic.h", "sifsrx_"),
    "baselines": ("sifsr_baselines.h", "sifsrb_"),
    "products": ("sifsr_products.h", "sifsrp_"),
    "gaps": ("sifsr_gaps.h", "sifsrg_"),
    "masked": ("sifsr_masked.h", "sifsrm_"),
    "scores": ("sifsr_scores.h", "sifsrv_"),
    "lpips": ("sifsr_lpips.h", "sifsrl_"),
    "conserve": ("sifsr_conserve.h", "sifsrk_"),
    "dms": ("sifsr_dms.h", "sifsrd_"),
    "spectra": ("sifsr_spectra.h", "sifsrf_"),
    "degrade": ("sifsr_degrade.h", "sifsrs_"),
    "adapt": ("sifsr_adapt.h", "sifsra_"),
    "sensor": ("sifsr_sensor.h", "sifsrt_"),
    "ratio": ("sifsr_ratio.h", "sifsrr_"),
    "rloss": ("sifsr_rloss.h", "sifsrq_"),
    "rconserve": ("sifsr_rconserve.h", "sifsrc_"),
    "rproducts": ("sifsr_rproducts.h", "sifsrn_"),
}
ABI_VERSION = 3
# the entry points whose int return is a count, not a status: call() raises on a non-zero int from every other one
COUNT_RETURNING = frozenset({
    "sifsr_abi_version", "sifsr_num_params", "sifsr_num_running", "sifsr_layer_table", "sifsr_model_workspace_regions",
    "sifsr_conv3x3_stat_blocks", "sifsr_conv3x3_stat_blocks_wino", "sifsr_conv3x3_bwd16_stat_rows", "sifsr_conv_in_stat_blocks",
    "sifsr_up2x_bwd_stat_rows", "sifsr_huber_partial_blocks", "sifsr_profile_add", "sifsrx_tile_count", "sifsrx_tile_origin",
})


def header_path(family: str = "core") -> str:
    return os.path.join(_ROOT, "include", FAMILIES[family][0])


HEADER = header_path()
# SIFSR_LIB: another build of the same C ABI (same-device A/B of kernel variants, tools/ab/); default: the in-tree library
LIB_PATH = os.environ.get("SIFSR_LIB") or os.path.join(_HERE, "libsifsr_hip.so")

_CTYPES = {
    "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
}


class SifsrError(RuntimeError):
    pass


class Arg(tuple):
    """(name, ctype) as lib() binds it, plus what the declaration says of the memory: .pointer and .const"""

    def __new__(cls, name, ctype, pointer, const):
        self = super().__new__(cls, (name, ctype))
        self.pointer, self.const = pointer, const
        return self


def parse_header(path: str = HEADER):
    """-> {name: (restype, [Arg(argname, ctype)])} for every SIFSR_API declaration."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"SIFSR_API\s+([\w\s]+?)\s+(\w+)\s*\(([^)]*)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        parsed = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                mm = re.match(r"(.+?)\s*(\w+)$", a)
                typ, an = mm.group(1).strip(), mm.group(2)
                pointer, const = "*" in typ, "const" in typ
                parsed.append(Arg(an, ctypes.c_void_p if pointer else _CTYPES[typ.replace("const ", "")], pointer, const))
        decls[name] = (_CTYPES[ret], parsed)
    return decls


def declared(family: str = "core"):
    """The sorted names the family's header declares."""
    return sorted(parse_header(header_path(family)))


def declared_symbols():
    return declared()


def writers(family: str = "core"):
    """-> {name: [non-const pointer argument names]} of the family's entry points that have any: what a call may write through.
    The `stream` handle is not memory."""
    out = {}
    for name, (_, args) in parse_header(header_path(family)).items():
        ptrs = [a[0] for a in args if a.pointer and not a.const and a[0] != "stream"]
        if ptrs:
            out[name] = ptrs
    return out


_lib = None
_decls = None


def lib():
    """Load (once) and return the ctypes handle; raises SifsrError if the HIP library is absent or of another ABI version."""
    global _lib, _decls
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SifsrError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        decls = {}
        for family in FAMILIES:
            decls.update(parse_header(header_path(family)))
        for name, (ret, args) in decls.items():
            fn = getattr(handle, name)     # AttributeError if the library lacks a declared symbol
            fn.restype = ret
            fn.argtypes = [t for _, t in args]
        got = handle.sifsr_abi_version()
        if got != ABI_VERSION:
            via = " (given by SIFSR_LIB)" if os.environ.get("SIFSR_LIB") else ""
            raise SifsrError(f"{LIB_PATH}{via} has ABI version {got}, this binding needs {ABI_VERSION}: rebuild the library")
        _lib, _decls = handle, decls
    return _lib


def bind_header(path: str):
    """Bind the SIFSR_API declarations of a header that is NOT a row of FAMILIES (one inside the package, whose module gates it
    itself) on the handle of lib(), with the declared types.  -> {name: (restype, [Arg])}.  call() then serves them like any other."""
    handle, decls = lib(), parse_header(path)
    for name, (ret, args) in decls.items():
        fn = getattr(handle, name)         # AttributeError if the library lacks a declared symbol
        fn.restype = ret
        fn.argtypes = [t for _, t in args]
    return decls


def _conv(v):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return v


def call(name: str, *args):
    """Call a C-ABI function; tensors are passed as device pointers.  Raises on a non-zero status."""
    fn = getattr(lib(), name)
    rc = fn(*[_conv(a) for a in args])
    if fn.restype is ctypes.c_int and rc != 0 and name not in COUNT_RETURNING:
        raise SifsrError(f"{name} failed with status {rc}")
    return rc


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu(t: torch.Tensor, what: str = "tensor"):
    if not t.is_cuda:
        raise SifsrError(f"{what} is on {t.device}: this package only runs on a ROCm GPU (gfx950); "
                         "there is no CPU path.")
    if t.dtype != torch.float32:
        raise SifsrError(f"{what} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise SifsrError(f"{what} must be contiguous")
