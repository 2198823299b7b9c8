"""ctypes binding of libminsdtf_hip_vision.so (C ABI declared in include/minsdtf_hip_vision.h): the vision library - the patch
embedding, the exact GELU and the pooled head of the CLIP ViT-H/14 vision tower - beside the core, the extension, the
dynamic-thresholding, the ControlNet-units and the IP-Adapter library, so all five of their ABIs stay what their tests describe.

The same rules as :mod:`minsdtf_amd._lib`: there is no CPU or PyTorch fallback, and a missing library or symbol raises
:class:`HipExtensionError`.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import HipExtensionError

LIB_NAME = "libminsdtf_hip_vision.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
ABI_VERSION = 1
IMAGE = 224       # MSDV_IMAGE
PATCH = 14        # MSDV_PATCH
GRID = 16         # MSDV_GRID
TOKENS = 257      # MSDV_TOKENS
WIDTH = 1280      # MSDV_WIDTH
PATCH_K = 588     # MSDV_PATCH_K
PROJ = 1024       # MSDV_PROJ
MAX_BATCH = 8     # MSDV_MAX_BATCH


class MsdvPatchEmbed(C.Structure):
    _fields_ = [
        ("pixels", C.c_void_p), ("w", C.c_void_p), ("cls", C.c_void_p), ("pos", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("out", C.c_void_p),
        ("scale", C.c_float * 3), ("shift", C.c_float * 3), ("eps", C.c_float),
        ("batch", C.c_int32), ("image", C.c_int32), ("patch", C.c_int32), ("width", C.c_int32),
        ("w_ld", C.c_int32), ("o_ld", C.c_int32),
    ]


class MsdvPoolProject(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("w", C.c_void_p), ("out", C.c_void_p),
        ("x_stride", C.c_int64), ("eps", C.c_float),
        ("batch", C.c_int32), ("width", C.c_int32), ("proj", C.c_int32), ("w_layout", C.c_int32),
    ]


# every symbol include/minsdtf_hip_vision.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "msdv_abi_version": (C.c_int, []),
    "msdv_last_error": (C.c_char_p, []),
    "msdv_patch_embed": (C.c_int, [C.POINTER(MsdvPatchEmbed), C.c_void_p]),
    "msdv_gelu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "msdv_pool_project": (C.c_int, [C.POINTER(MsdvPoolProject), C.c_void_p]),
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
    if lib.msdv_abi_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI version mismatch: library {lib.msdv_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().msdv_last_error().decode(errors="replace")
        raise HipExtensionError(f"{what} failed (rc={rc}): {msg}")
