"""The one reader of the C headers (include/tomo.h, include/tomo_<name>.h), used ONLY by the tests: what a header declares -- functions,
numeric constants, structs -- in a form that can be held against the hand-written ctypes table of its binding module, and the two
comparisons.  tests/test_binding.py runs them over every library of __graft_entry__.LIBRARIES; a test that needs one value of a header
takes it from parse_header.  Nothing in the product imports this module."""
import collections
import ctypes
import importlib
import os
import re

from conftest import ROOT

import __graft_entry__ as entry
from tomography_alignment_amd import _binding

Library = collections.namedtuple("Library", "module name prefix header build_dir handle errors")
Header = collections.namedtuple("Header", "functions constants structs")

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
           "double": ctypes.c_double, "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "char": ctypes.c_char}


def header_path(sub):
    """include/tomo_<sub>.h; include/tomo.h for ""."""
    return os.path.join(ROOT, "include", "tomo_%s.h" % sub if sub else "tomo.h")


def libraries():
    """One record per entry of __graft_entry__.LIBRARIES: the binding module, the library name ("hip" for csrc/ itself), the prefix of
    its symbols, its header, the directory of its Makefile, the _binding.Handle subclass the module defines (None for _lib) and the
    exception classes it defines (TomoError subclasses all, which tests/test_binding.py asserts)."""
    out = []
    for sub, modname in entry.LIBRARIES:
        mod = importlib.import_module("tomography_alignment_amd." + modname)
        own = [v for v in vars(mod).values() if isinstance(v, type) and v.__module__ == mod.__name__]
        handles = [c for c in own if issubclass(c, _binding.Handle)]
        assert len(handles) == (1 if sub else 0), (modname, handles)
        out.append(Library(mod, sub or "hip", "tomo_%s_" % sub if sub else "tomo_", header_path(sub),
                           "tomography_alignment_amd/csrc" + ("/" + sub if sub else ""), handles[0] if handles else None,
                           tuple(c for c in own if issubclass(c, Exception))))
    return out


_NUMBER = r"(?:0[xX][0-9a-fA-F]+|(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?)"


def _value(expr):
    """The value of integer or float arithmetic over literals, None for anything else (a name, a string, an attribute)."""
    expr = re.sub(r"(?<![\w.])(%s)[uUlLfF]*(?![\w.])" % _NUMBER, r"\1", expr.strip())
    if not expr or not re.match(r"^(?:\s|%s|<<|>>|[-+*/%%()|&^~])+$" % _NUMBER, expr):
        return None
    if not re.search(r"[.eE]", re.sub(r"0[xX][0-9a-fA-F]+", "0", expr)):
        expr = expr.replace("/", "//")          # C divides integers as integers
    try:
        return eval(expr, {"__builtins__": {}}, {})        # noqa: S307 -- digits, operators and parentheses only
    except Exception:      # noqa: BLE001
        return None


def _type(text, named):
    """(base type, pointer depth) of a parameter or return type: const dropped, a trailing [n] one pointer level, the name dropped."""
    text, n_arrays = re.subn(r"\[[^\]]*\]", " ", text)
    words = [w for w in text.replace("*", " ").split() if w not in ("const", "struct", "enum", "volatile", "restrict")]
    if named and len(words) > 1 and words[-1] not in ("int", "char", "long", "short", "unsigned", "signed", "float", "double"):
        words.pop()
    return " ".join(words), text.count("*") + n_arrays


def parse_header(path):
    with open(path) as f:
        return parse_text(f.read())


def parse_text(text):
    """What a header declares, comments stripped first.  functions: name -> (return type, [parameter types]), a type being (base type,
    pointer depth).  constants: every #define TOMO_... and enumerator TOMO_... = <expr> whose expression is arithmetic over literals ->
    its value.  structs: typedef name -> [(field, base type, array length or None)] in order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    constants = collections.OrderedDict()
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(TOMO_\w+)[ \t]+(\S[^\n]*)$", text, flags=re.M):
        if _value(expr) is not None:
            constants[name] = _value(expr)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    for body in re.findall(r"\benum\b[^{;]*\{([^{}]*)\}", text):
        for name, expr in re.findall(r"\b(TOMO_\w+)\s*=\s*([^,]+)", body):
            if _value(expr) is not None:
                constants[name] = _value(expr)
    structs = collections.OrderedDict()
    for body, name in re.findall(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base = _type(decl.split(",")[0], True)[0]
            for d in decl[decl.index(base) + len(base):].split(","):            # int flags, ja, i0: one type, several fields
                n = re.search(r"\[([^\]]*)\]", d)
                fields.append((re.sub(r"\[[^\]]*\]", "", d).replace("*", " ").split()[-1], base + " *" * d.count("*"),
                               int(_value(n.group(1))) if n else None))
        structs[name] = fields
    functions = collections.OrderedDict()
    for ret, name, params in re.findall(r"\bTOMO_API\b([^;(]*?)\b(\w+)\s*\(([^;]*?)\)\s*;", text):
        params = [] if params.strip() in ("void", "") else [_type(p, True) for p in params.split(",")]
        functions[name] = (_type(ret, False), params)
    return Header(functions, constants, structs)


def _is_pointer_to(got, what):
    """got is ctypes.POINTER(T) with T a subclass of `what`."""
    return isinstance(got, type) and issubclass(got, ctypes._Pointer) and isinstance(got._type_, type) and issubclass(got._type_, what)


def _fits(ctype, base, depth, returned):
    if depth == 0:
        return ctype is (None if base == "void" else SCALARS.get(base, ()))
    if base == "char" and depth == 1:
        return ctype is ctypes.c_char_p or (not returned and ctype in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_char)))
    if depth >= 2:
        return ctype is ctypes.POINTER(ctypes.c_void_p)
    if base in SCALARS:
        return ctype in (ctypes.c_void_p, ctypes.POINTER(SCALARS[base]))
    return ctype is ctypes.c_void_p or (base != "void" and _is_pointer_to(ctype, ctypes.Structure))


def _c(base, depth):
    return base + " " + "*" * depth if depth else base


def compare_signature(decl, sig):
    """The differences (texts; none: they agree) between one parsed declaration and its (restype, argtypes).  A scalar is exactly the
    ctypes type of its C type; a returned const char * is c_char_p; a pointer to a scalar T is c_void_p (a device pointer, by the
    package's convention) or POINTER(T); void * is c_void_p, and so is a pointer to a handle or a struct, or else
    POINTER(a ctypes.Structure); a pointer to a pointer is POINTER(c_void_p).  A different arity is one difference."""
    (ret, params), (restype, argtypes) = decl, sig
    out = []
    if not _fits(restype, ret[0], ret[1], True):
        out.append("returns %s, bound as %s" % (_c(*ret), getattr(restype, "__name__", restype)))
    if len(params) != len(argtypes):
        return out + ["%d parameters, %d argtypes" % (len(params), len(argtypes))]
    for i, ((base, depth), ctype) in enumerate(zip(params, argtypes)):
        if not _fits(ctype, base, depth, False):
            out.append("parameter %d is %s, bound as %s" % (i, _c(base, depth), getattr(ctype, "__name__", ctype)))
    return out


def compare_struct(fields, struct):
    """The differences between the parsed fields of a struct and a ctypes.Structure: names, order, scalar types, array lengths."""
    mirrored = list(struct._fields_)
    if [f[0] for f in fields] != [f[0] for f in mirrored]:
        return ["fields %s, mirrored as %s" % ([f[0] for f in fields], [f[0] for f in mirrored])]
    out = []
    for (name, base, length), (_, ctype) in zip(fields, mirrored):
        expect = SCALARS.get(base)
        if length is not None and expect is not None:
            expect = expect * length            # ctypes caches array types: the same (T, n) is the same class
        if expect is None or ctype is not expect:
            out.append("%s is %s%s, mirrored as %s" % (name, base, "" if length is None else "[%d]" % length, ctype.__name__))
    return out
