"""Loader for the C-ABI shared library (syzygy_amd/csrc/libszg_hip.so)."""
import ctypes
import os
import sys

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class SzgError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, code, message):
        super().__init__(f"szg status {code}: {message}")
        self.code = code


def library_path():
    # SZG_HIP_LIBRARY: tests/test_gpu_spirv_pin.py, tests/test_gpu_contraction_whole_images.py and tests/test_gpu_literal_gates.py
    # point child processes at csrc/libszg_hip_literal.so (the same kernels with the contraction rule switched off); nothing
    # else sets it
    return os.environ.get("SZG_HIP_LIBRARY") or os.path.join(_HERE, "csrc", "libszg_hip.so")


def lib():
    """The bound ctypes library. Fails loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C syzygy_amd/csrc`). There is no CPU fallback for this path."
            )
        # torch bundles its own HIP runtime; import it first so that this library binds to the
        # SAME runtime instance (device pointers and streams are shared with torch).
        import torch  # noqa: F401

        handle = ctypes.CDLL(path)
        # the version first: a library of another ABI version lacks or mis-declares symbols, and binding it would fail
        # with an AttributeError that hides the real cause
        handle.szg_abi_version.restype = ctypes.c_int
        handle.szg_abi_version.argtypes = []
        version = handle.szg_abi_version()
        if version != abi.SZG_ABI_VERSION:
            raise RuntimeError(f"{path}: ABI version {version}, this package needs {abi.SZG_ABI_VERSION}; rebuild the library")
        for header, table, notice in abi.BINDINGS:
            try:
                abi.bind(handle, table)
            except AttributeError as e:
                if header is None:
                    raise
                # additive entry points do not move the ABI version (include/szg/abi.h): an older build of the same version lacks them
                if notice is None or "SZG_HIP_LIBRARY" not in os.environ:
                    raise RuntimeError(f"{path} predates include/szg/{header} ({e}); rebuild the library") from e
                # a library named explicitly for a comparison (tools/bench_raster_libraries.py --baseline: a parent commit's build)
                # may predate the header: everything else works, and one of its entry points raises AttributeError when it is called
                print(f"[szg] {path} predates include/szg/{header} ({e}): {notice}", file=sys.stderr)
        _LIB = handle
    return _LIB


def check(status):
    if status != abi.SZG_OK:
        raise SzgError(status, lib().szg_last_error().decode("utf-8", "replace"))
    return status
