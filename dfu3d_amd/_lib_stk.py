"""ctypes binding of the stacked set-abstraction entry points (C ABI in csrc/dfu3d_stk.h), exported by the same
libdfu3d_hip.so as include/dfu3d.h's.  Signatures and constants are read from the header with the reader of dfu3d.h
(_header.parse); lib() binds them on _lib.lib() and raises naming every symbol the library lacks."""
import ctypes
import os

from . import _build, _lib
from ._header import parse
from ._lib import Dfu3dError

HEADER = os.path.join(_build.CSRC, "dfu3d_stk.h")

with open(HEADER) as _f:
    STRUCTS, SIGNATURES, CONSTANTS = parse(_f.read(), more_scalars={"size_t": ctypes.c_size_t})

_BOUND = None


def header_symbols():
    """Function names declared in csrc/dfu3d_stk.h."""
    return sorted(SIGNATURES)


def header_version():
    return CONSTANTS["DFU3D_STK_VERSION"]


def bind(L):
    missing = [name for name in sorted(SIGNATURES) if not hasattr(L, name)]
    if missing:
        raise Dfu3dError("%s does not export %s" % (L._name, ", ".join(missing)))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def lib():
    """_lib.lib() with the entry points of dfu3d_stk.h declared on it."""
    global _BOUND
    if _BOUND is None:
        _BOUND = bind(_lib.lib())
    return _BOUND


def check(code, what):
    _lib.check(code, what)
