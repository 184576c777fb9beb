"""ctypes binding of libsifsr_hip.so.

The signatures are parsed from ``include/sifsr_hip.h`` -- the header is the single source of truth
for the C ABI, and ``tests/test_capi_symbols.py`` checks that the library exports every declared
symbol -- and from its extensions ``include/sifsr_mosaic.h`` (prefix ``sifsrx_``, same declaration style,
gated by ``tests/test_mosaic_host.py``), ``include/sifsr_baselines.h`` (prefix ``sifsrb_``, gated by
``tests/test_baselines_host.py``), ``include/sifsr_products.h`` (prefix ``sifsrp_``, gated by
``tests/test_products_host.py``), ``include/sifsr_gaps.h`` (prefix ``sifsrg_``, gated by
``tests/test_gaps_host.py``), ``include/sifsr_masked.h`` (prefix ``sifsrm_``, gated by
``tests/test_masked_host.py``), ``include/sifsr_scores.h`` (prefix ``sifsrv_``, gated by
``tests/test_scores_host.py``), ``include/sifsr_lpips.h`` (prefix ``sifsrl_``, gated by
``tests/test_lpips_host.py``), ``include/sifsr_conserve.h`` (prefix ``sifsrk_``, gated by
``tests/test_conserve_host.py``), ``include/sifsr_dms.h`` (prefix ``sifsrd_``, gated by
``tests/test_dms_host.py``), ``include/sifsr_spectra.h`` (prefix ``sifsrf_``, gated by
``tests/test_spectra_host.py``), ``include/sifsr_degrade.h`` (prefix ``sifsrs_``, gated by
``tests/test_degrade_host.py``) and ``include/sifsr_adapt.h`` (prefix ``sifsra_``, gated by
``tests/test_adapt_host.py``).  There is NO fallback: if the library is missing or a call fails, we raise.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch  # noqa: F401  (must be imported first: the library binds to the libamdhip64 torch loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
HEADER = os.path.join(_ROOT, "include", "sifsr_hip.h")
EXTENSION_HEADER = os.path.join(_ROOT, "include", "sifsr_mosaic.h")
BASELINES_HEADER = os.path.join(_ROOT, "include", "sifsr_baselines.h")
PRODUCTS_HEADER = os.path.join(_ROOT, "include", "sifsr_products.h")
GAPS_HEADER = os.path.join(_ROOT, "include", "sifsr_gaps.h")
MASKED_HEADER = os.path.join(_ROOT, "include", "sifsr_masked.h")
SCORES_HEADER = os.path.join(_ROOT, "include", "sifsr_scores.h")
LPIPS_HEADER = os.path.join(_ROOT, "include", "sifsr_lpips.h")
CONSERVE_HEADER = os.path.join(_ROOT, "include", "sifsr_conserve.h")
DMS_HEADER = os.path.join(_ROOT, "include", "sifsr_dms.h")
SPECTRA_HEADER = os.path.join(_ROOT, "include", "sifsr_spectra.h")
DEGRADE_HEADER = os.path.join(_ROOT, "include", "sifsr_degrade.h")
ADAPT_HEADER = os.path.join(_ROOT, "include", "sifsr_adapt.h")
# SIFSR_LIB: another build of the same C ABI (same-device A/B of kernel variants, tools/ab/); default: the in-tree library
LIB_PATH = os.environ.get("SIFSR_LIB") or os.path.join(_HERE, "libsifsr_hip.so")

_CTYPES = {
    "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
}


class SifsrError(RuntimeError):
    pass


def parse_header(path: str = HEADER):
    """-> {name: (restype, [(argname, ctype)])} for every SIFSR_API declaration."""
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
                if "*" in typ:
                    parsed.append((an, ctypes.c_void_p))
                else:
                    parsed.append((an, _CTYPES[typ.replace("const ", "")]))
        decls[name] = (_CTYPES[ret], parsed)
    return decls


_lib = None
_decls = None


def lib():
    """Load (once) and return the ctypes handle; raises SifsrError if the HIP library is absent."""
    global _lib, _decls
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SifsrError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        _decls = {**parse_header(), **parse_header(EXTENSION_HEADER), **parse_header(BASELINES_HEADER),
                  **parse_header(PRODUCTS_HEADER), **parse_header(GAPS_HEADER), **parse_header(MASKED_HEADER),
                  **parse_header(SCORES_HEADER), **parse_header(LPIPS_HEADER), **parse_header(CONSERVE_HEADER),
                  **parse_header(DMS_HEADER), **parse_header(SPECTRA_HEADER), **parse_header(DEGRADE_HEADER),
                  **parse_header(ADAPT_HEADER)}
        for name, (ret, args) in _decls.items():
            fn = getattr(handle, name)     # AttributeError if the library lacks a declared symbol
            fn.restype = ret
            fn.argtypes = [t for _, t in args]
        _lib = handle
    return _lib


def declared_symbols():
    return sorted(parse_header().keys())


def declared_extension_symbols():
    """The names ``include/sifsr_mosaic.h`` declares (``sifsrx_*``); ``declared_symbols`` stays the main header's."""
    return sorted(parse_header(EXTENSION_HEADER).keys())


def declared_baseline_symbols():
    """The names ``include/sifsr_baselines.h`` declares (``sifsrb_*``)."""
    return sorted(parse_header(BASELINES_HEADER).keys())


def declared_product_symbols():
    """The names ``include/sifsr_products.h`` declares (``sifsrp_*``)."""
    return sorted(parse_header(PRODUCTS_HEADER).keys())


def declared_gap_symbols():
    """The names ``include/sifsr_gaps.h`` declares (``sifsrg_*``)."""
    return sorted(parse_header(GAPS_HEADER).keys())


def declared_masked_symbols():
    """The names ``include/sifsr_masked.h`` declares (``sifsrm_*``)."""
    return sorted(parse_header(MASKED_HEADER).keys())


def declared_score_symbols():
    """The names ``include/sifsr_scores.h`` declares (``sifsrv_*``)."""
    return sorted(parse_header(SCORES_HEADER).keys())


def declared_lpips_symbols():
    """The names ``include/sifsr_lpips.h`` declares (``sifsrl_*``)."""
    return sorted(parse_header(LPIPS_HEADER).keys())


def declared_conserve_symbols():
    """The names ``include/sifsr_conserve.h`` declares (``sifsrk_*``)."""
    return sorted(parse_header(CONSERVE_HEADER).keys())


def declared_dms_symbols():
    """The names ``include/sifsr_dms.h`` declares (``sifsrd_*``)."""
    return sorted(parse_header(DMS_HEADER).keys())


def declared_spectra_symbols():
    """The names ``include/sifsr_spectra.h`` declares (``sifsrf_*``)."""
    return sorted(parse_header(SPECTRA_HEADER).keys())


def declared_degrade_symbols():
    """The names ``include/sifsr_degrade.h`` declares (``sifsrs_*``)."""
    return sorted(parse_header(DEGRADE_HEADER).keys())


def declared_adapt_symbols():
    """The names ``include/sifsr_adapt.h`` declares (``sifsra_*``)."""
    return sorted(parse_header(ADAPT_HEADER).keys())


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
    if fn.restype is ctypes.c_int and rc != 0 and not name.startswith(("sifsr_abi", "sifsr_num", "sifsr_layer", "sifsr_huber_partial", "sifsr_model_workspace_regions", "sifsr_conv3x3_stat", "sifsr_conv_in_stat", "sifsr_conv3x3_bwd16_stat", "sifsr_profile_add", "sifsr_up2x_bwd_stat", "sifsrx_tile_")):
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
