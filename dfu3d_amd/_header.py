"""Reader of include/dfu3d.h: the one place the Python side learns the C ABI from.

parse() turns the header's text into its ctypes view -- a Structure class per struct, (restype, [argtypes]) per
prototype, the value of every integer macro -- so nothing of the boundary is typed a second time.  The header keeps to
a small regular subset of C: prototypes `ret dfu3d_name(args);` over the scalars below, pointers to them and to the
header's structs; structs of scalars and earlier structs; object-like macros.  Whatever falls outside raises, naming
the declaration; nothing is guessed.  The module reads the header once, when it is imported.
"""
import ctypes
import os
import re

from . import _build

HEADER = os.path.join(_build.INCLUDE, "dfu3d.h")

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = set(SCALARS) | {"void", "uint8_t"}       # device arrays and scalar out-parameters: void* to ctypes
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*\w*")
_LITERAL = re.compile(r"(0|[1-9]\d*)[uU]?")
_OPS = set("+-*()")


def _ctype(decl, structs, where, ret=False, scalars=SCALARS):
    m = _DECL.fullmatch(decl.strip())
    base, ptr = m.groups() if m else (None, None)
    if base in structs:
        return ctypes.POINTER(structs[base]) if ptr else structs[base]
    if ptr and ret and base == "char":
        return ctypes.c_char_p
    if ptr and base in _POINTEES:
        return ctypes.c_void_p
    if not ptr and base in scalars:
        return scalars[base]
    raise ValueError("dfu3d.h: %s: unknown type in %r" % (where, decl.strip()))


def _int_expr(body):
    """Value of a macro body made of integer literals, + - * and parentheses (as Python integers: no wrap-around);
    None for any other body, which is not looked at further."""
    toks = re.findall(r"\w+|\S", body)
    if not toks or not all(_LITERAL.fullmatch(t) or t in _OPS for t in toks):
        return None
    toks.append("")

    def atom():
        t = toks.pop(0)
        if t == "(":
            v = expr()
            if toks.pop(0) != ")":
                raise ValueError("unbalanced parentheses")
            return v
        if t in ("+", "-"):
            return atom() if t == "+" else -atom()
        return int(t.rstrip("uU"))

    def term():
        v = atom()
        while toks[0] == "*":
            toks.pop(0)
            v *= atom()
        return v

    def expr():
        v = term()
        while toks[0] in ("+", "-"):
            v = v + term() if toks.pop(0) == "+" else v - term()
        return v

    v = expr()
    if toks != [""]:
        raise ValueError("trailing %r" % toks[0])
    return v


def parse(text, more_scalars=None):
    """Header text -> (structs {C name: Structure class}, signatures {name: (restype, [argtypes])}, constants
    {DFU3D_NAME: int}).  more_scalars: {C name: ctypes type} a header other than dfu3d.h passes by value in its prototypes
    on top of SCALARS (dfu3d_post.h: size_t); dfu3d.h itself stays within SCALARS.  Function-like macros, the include
    guard and macros whose body is no integer expression are skipped (the library's size functions answer for
    DFU3D_SHADOW_BYTES / DFU3D_RF_QUEUE_INTS)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, params, body in re.findall(r"(?m)^[ \t]*#[ \t]*define[ \t]+(DFU3D_\w+)(\(?)(.*)$", text):
        try:
            value = None if params else _int_expr(body)
        except (ValueError, IndexError) as e:
            raise ValueError("dfu3d.h: %s: %s in %r" % (name, e, body.strip()))
        if value is not None:
            constants[name] = value
    text = re.sub(r"(?m)^[ \t]*#.*$", "", text)
    structs = {}
    struct_re = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)
    for name, body in struct_re.findall(text):
        fields = []
        for member in filter(None, (m.strip() for m in body.split(";"))):
            first, *more = (d.strip() for d in " ".join(member.split()).split(","))
            ctype, _, first = first.rpartition(" ")
            for field in [first] + more:
                if not re.fullmatch(r"\w+", field):
                    raise ValueError("dfu3d.h: %s: cannot read the member %r" % (name, member))
                fields.append((field, _ctype(ctype, structs, name)))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "%s (include/dfu3d.h)." % name})
    signatures = {}
    scalars = dict(SCALARS, **(more_scalars or {}))
    text = re.sub(r'extern\s+"C"\s*\{|\}', "", struct_re.sub("", text))
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(dfu3d_\w+)\s*\((.*)\)", decl, re.S)
        if not m:
            raise ValueError("dfu3d.h: cannot read the declaration %r" % decl)
        ret, name, args = m.groups()
        args = [] if args.strip() == "void" else args.split(",")
        signatures[name] = (_ctype(ret, structs, name, ret=True, scalars=scalars),
                            [_ctype(a, structs, name, scalars=scalars) for a in args])
    return structs, signatures, constants


with open(HEADER) as _f:
    STRUCTS, SIGNATURES, CONSTANTS = parse(_f.read())
