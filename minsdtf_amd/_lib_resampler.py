"""ctypes binding of libminsdtf_hip_resampler.so (C ABI declared in include/minsdtf_hip_resampler.h): the resampler library - the
two-segment attention of an IP-Adapter "plus" Resampler layer - beside the core, the extension, the dynamic-thresholding, the
ControlNet-units, the IP-Adapter and the vision library, so all six of their ABIs stay what their tests describe.

The same rules as :mod:`minsdtf_amd._lib`: there is no CPU or PyTorch fallback, and a missing library or symbol raises
:class:`HipExtensionError`.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipExtensionError

LIB_NAME = "libminsdtf_hip_resampler.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
ABI_VERSION = 1
HEAD_DIM = 64       # MSDR_HEAD_DIM
MAX_QUERIES = 16    # MSDR_MAX_QUERIES
MAX_TX = 272        # MSDR_MAX_TX
KEY_TILE = 16       # MSDR_KEY_TILE


class MsdrPerceiverAttention(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k_x", C.c_void_p), ("vt_x", C.c_void_p), ("k_l", C.c_void_p), ("vt_l", C.c_void_p), ("out", C.c_void_p),
        ("scale", C.c_float),
        ("batch", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32), ("n", C.c_int32), ("t_x", C.c_int32),
        ("q_ld", C.c_int32), ("kx_ld", C.c_int32), ("vtx_ld", C.c_int32), ("kl_ld", C.c_int32), ("vtl_ld", C.c_int32), ("o_ld", C.c_int32),
    ]


# every symbol include/minsdtf_hip_resampler.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "msdr_abi_version": (C.c_int, []),
    "msdr_last_error": (C.c_char_p, []),
    "msdr_perceiver_attention": (C.c_int, [C.POINTER(MsdrPerceiverAttention), C.c_void_p]),
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
    if lib.msdr_abi_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI version mismatch: library {lib.msdr_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().msdr_last_error().decode(errors="replace")
        raise HipExtensionError(f"{what} failed (rc={rc}): {msg}")
