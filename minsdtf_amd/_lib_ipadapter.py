"""ctypes binding of libminsdtf_hip_ipadapter.so (C ABI declared in include/minsdtf_hip_ipadapter.h): the IP-Adapter library beside
the core, the extension, the dynamic-thresholding and the ControlNet-units library, so all four of their ABIs stay what their tests
describe.

The same rules as :mod:`minsdtf_amd._lib`: there is no CPU or PyTorch fallback, and a missing library or symbol raises
:class:`HipExtensionError`.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipExtensionError

LIB_NAME = "libminsdtf_hip_ipadapter.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
ABI_VERSION = 1
LAYERS = 16       # MSDI_LAYERS
KEYS = 96         # MSDI_KEYS
MAX_TOKENS = 16   # MSDI_MAX_TOKENS


class MsdiAttentionDecoupled(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("vt", C.c_void_p), ("k_ip", C.c_void_p), ("vt_ip", C.c_void_p), ("out", C.c_void_p),
        ("scales", C.c_void_p), ("step_ptr", C.c_void_p),
        ("batch", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32), ("s", C.c_int32), ("t", C.c_int32), ("n", C.c_int32),
        ("q_ld", C.c_int32), ("k_ld", C.c_int32), ("vt_ld", C.c_int32), ("kip_ld", C.c_int32), ("vtip_ld", C.c_int32), ("o_ld", C.c_int32),
        ("layer", C.c_int32), ("num_steps", C.c_int32),
    ]


# every symbol include/minsdtf_hip_ipadapter.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "msdi_abi_version": (C.c_int, []),
    "msdi_last_error": (C.c_char_p, []),
    "msdi_attention_decoupled": (C.c_int, [C.POINTER(MsdiAttentionDecoupled), C.c_void_p]),
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
    if lib.msdi_abi_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI version mismatch: library {lib.msdi_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().msdi_last_error().decode(errors="replace")
        raise HipExtensionError(f"{what} failed (rc={rc}): {msg}")
