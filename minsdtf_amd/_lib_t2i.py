"""ctypes binding of libminsdtf_hip_t2i.so (C ABI declared in include/minsdtf_hip_t2i.h): the T2I-Adapter library - the per-step
feature add and the three layer types of the adapter network the core has no kernel of - beside the core, the extension, the
dynamic-thresholding, the ControlNet-units, the IP-Adapter, the vision and the resampler library, so all seven of their ABIs stay
what their tests describe.

The same rules as :mod:`minsdtf_amd._lib`: there is no CPU or PyTorch fallback, and a missing library or symbol raises
:class:`HipExtensionError`.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipExtensionError

LIB_NAME = "libminsdtf_hip_t2i.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
ABI_VERSION = 1
MAX_UNITS = 3   # MSDA_MAX_UNITS
SITES = 4       # MSDA_SITES
CHUNK = 2048    # MSDA_CHUNK


class MsdaFeatureAdd(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("feat", C.c_void_p * MAX_UNITS), ("scales", C.c_void_p), ("step_ptr", C.c_void_p),
        ("rows", C.c_int32), ("n", C.c_int32), ("units", C.c_int32), ("site", C.c_int32), ("num_steps", C.c_int32),
    ]


# every symbol include/minsdtf_hip_t2i.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "msda_abi_version": (C.c_int, []),
    "msda_last_error": (C.c_char_p, []),
    "msda_feature_add": (C.c_int, [C.POINTER(MsdaFeatureAdd), C.c_void_p]),
    "msda_unshuffle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "msda_relu": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "msda_avgpool2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and type the shared library.  Raises HipExtensionError when it is unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no fallback path.")
    import torch  # noqa: F401  — torch's bundled libamdhip64.so.7 must be the HIP runtime the library binds to

    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise HipExtensionError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipExtensionError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.msda_abi_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI version mismatch: library {lib.msda_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().msda_last_error().decode(errors="replace")
        raise HipExtensionError(f"{what} failed (rc={rc}): {msg}")
