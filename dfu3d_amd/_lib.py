"""ctypes binding of libdfu3d_hip.so (C ABI in include/dfu3d.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, every
entry point raises.  Signatures, structs and constants are READ from the header
when the package is imported (_header.py), so the binding cannot differ from it;
a declaration the reader does not understand raises there.  tests/test_abi.py
pins a few signatures by hand and compiles the struct layouts with a C compiler.
"""
import ctypes
import os

from . import _build
from ._header import CONSTANTS, HEADER, SIGNATURES, STRUCTS  # noqa: F401

BinGeom, Sizes, ChainCfg, EvalCombo = (STRUCTS["dfu3d_" + n] for n in ("bin_geom", "sizes", "chain_cfg", "eval_combo"))

_LIB = None


class Dfu3dError(RuntimeError):
    pass


def header_symbols():
    """Function names declared in include/dfu3d.h."""
    return sorted(SIGNATURES)


def header_version():
    """DFU3D_VERSION of include/dfu3d.h."""
    return CONSTANTS["DFU3D_VERSION"]


def bind(L):
    """Declare every entry point of include/dfu3d.h on the loaded library L; raises if L lacks one."""
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise Dfu3dError("%s does not export %s" % (L._name, name))
        fn.restype = res
        fn.argtypes = args
    return L


def lib():
    """Load (building in-tree if needed) libdfu3d_hip.so; raises if impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PyTorch-ROCm ships its own HIP runtime; it must be in the process before this
    # library is dlopen'ed so that both resolve the SAME libamdhip64 (otherwise torch's
    # streams and device pointers are foreign to our launches: hipErrorInvalid*).
    import torch  # noqa: F401
    path = _build.OUT
    try:
        _build.build()          # no-op when the library is newer than every source
    except Exception as e:      # no silent fallback: a stale library must not be mistaken for the sources
        if not os.path.exists(path):
            raise Dfu3dError("libdfu3d_hip.so is missing and could not be built: %r" % (e,))
        if _build.needs_build():
            raise Dfu3dError("libdfu3d_hip.so is older than its sources and could not be rebuilt: %r" % (e,))
    try:
        L = ctypes.CDLL(path)
    except OSError as e:
        raise Dfu3dError("cannot load %s: %s" % (path, e))
    _LIB = bind(L)
    return L


def load_variant(name):
    """A test / timing build of the library (dfu3d_amd/_build.py: VARIANTS) with the product's signatures.  For tests/ and
    tools/ only: lib() never returns one, whatever the environment says."""
    import torch  # noqa: F401
    return bind(ctypes.CDLL(_build.build_variant(name)))     # no-op when newer than every source


def check(code, what):
    if code != 0:
        msg = lib().dfu3d_strerror(int(code)).decode()
        raise Dfu3dError("%s failed: %s (%d)" % (what, msg, code))
