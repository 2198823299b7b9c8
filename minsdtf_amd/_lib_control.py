"""ctypes binding of libminsdtf_hip_control.so (C ABI declared in include/minsdtf_hip_control.h): the ControlNet-units library
beside the core, the extension and the dynamic-thresholding library, so all three of their ABIs stay what their tests describe.

The same rules as :mod:`minsdtf_amd._lib`: there is no CPU or PyTorch fallback, and a missing library or symbol raises
:class:`HipExtensionError`.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipExtensionError

LIB_NAME = "libminsdtf_hip_control.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
ABI_VERSION = 1
TAPS = 13        # MSDC_TAPS
MAX_UNITS = 3    # MSDC_MAX_UNITS
CHUNK = 2048     # MSDC_CHUNK


class MsdcControlCombine(C.Structure):
    _fields_ = [
        ("skip", C.c_void_p * TAPS), ("resid", (C.c_void_p * TAPS) * MAX_UNITS), ("scales", C.c_void_p), ("step_ptr", C.c_void_p),
        ("count", C.c_int32 * TAPS), ("chunk_prefix", C.c_int32 * (TAPS + 1)),
        ("rows", C.c_int32), ("rows_u", C.c_int32), ("units", C.c_int32), ("num_steps", C.c_int32),
    ]


# every symbol include/minsdtf_hip_control.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "msdc_abi_version": (C.c_int, []),
    "msdc_last_error": (C.c_char_p, []),
    "msdc_control_combine": (C.c_int, [C.POINTER(MsdcControlCombine), C.c_void_p]),
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
    if lib.msdc_abi_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI version mismatch: library {lib.msdc_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().msdc_last_error().decode(errors="replace")
        raise HipExtensionError(f"{what} failed (rc={rc}): {msg}")
