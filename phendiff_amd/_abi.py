"""The ctypes view of ``include/phendiff_hip.h``, read from the header itself: structs, prototypes, enumerators and integer
``#define``s.  The header is regular (one declaration style, no macros in declarations, no nested braces), so this is a few regular
expressions and not a C parser; anything outside the tables below raises and names what it met -- nothing is guessed.
"""
from __future__ import annotations

import ctypes as C
import re

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "long long": C.c_longlong, "size_t": C.c_size_t}
RESTYPES = {"int": C.c_int, "size_t": C.c_size_t, "char *": C.c_char_p}

_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(pd_\w+)\s*\(([^()]*)\)\s*;")


def python_name(cname: str) -> str:
    """pd_foo_bar_args -> FooBarArgs"""
    return "".join(w.capitalize() for w in cname[len("pd_"):].split("_"))


def _words(spec):
    return [w for w in re.findall(r"\w+|\*", spec) if w != "const"]


def _declarators(decl, where):
    """``const float *a, *b`` -> ("float", 1, "a", None), ("float", 1, "b", None): base type, pointer depth, name, array length."""
    base = None
    for part in decl.split(","):
        m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[(\d+)\])?", part.strip(), flags=re.S)
        words = _words(m.group(1)) if m else []
        base = " ".join(w for w in words if w != "*") or base
        if m is None or base is None:
            raise TypeError(f"{where}: cannot read the declaration {part.strip()!r}")
        yield base, words.count("*"), m.group(2), m.group(3)


def _ctype(base, stars, dim, where):
    """Every pointer is a c_void_p, ``char name[N]`` a c_char array, a scalar what SCALARS says; anything else is refused."""
    if stars:
        return C.c_void_p
    if dim and base == "char":
        return C.c_char * int(dim)
    if dim or base not in SCALARS:
        raise TypeError(f"{where}: C type {base + ('[' + dim + ']' if dim else '')!r} has no ctypes mapping")
    return SCALARS[base]


def read(text: str, out_params: dict):
    """(structs, symbols, constants) of a header's text: C struct name -> ctypes.Structure class, function name -> (restype,
    argtypes), enumerator / ``#define PD_*`` name -> int.  ``out_params`` maps (function, parameter) to the argtype of a host
    out-parameter that is passed with byref (a scalar pointer would otherwise be a c_void_p)."""
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    constants = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PD_\w+)[ \t]+(-?\d+)[ \t]*$", src, flags=re.M)}
    for body in re.findall(r"\benum\s*\{([^{}]*)\}", src):
        pairs = re.findall(r"(\w+)\s*=\s*(-?\d+)", body)
        if len(pairs) != len([e for e in body.split(",") if e.strip()]):
            raise TypeError(f"enum {{{' '.join(body.split())}}}: every enumerator needs an explicit integer value")
        constants.update((n, int(v)) for n, v in pairs)

    structs = {}
    for body, cname in re.findall(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(pd_\w+)\s*;", src):
        fields = [(name, _ctype(base, stars, dim, f"{cname}.{name}"))
                  for decl in body.split(";") if decl.strip()
                  for base, stars, name, dim in _declarators(decl, cname)]
        structs[cname] = type(python_name(cname), (C.Structure,), {"_fields_": fields})

    # what is left once the typedefs, the anonymous enum and the preprocessor lines are gone is the prototypes
    rest = re.sub(r"\btypedef\b[^;{]*\{[^{}]*\}[^;]*;|\benum\s*\{[^{}]*\}\s*;|^[ \t]*#.*$", "", src, flags=re.M)
    symbols, pending = {}, dict(out_params)
    for ret, fname, params in _PROTOTYPE.findall(rest):
        ret = " ".join(_words(ret))
        if ret not in RESTYPES:
            raise TypeError(f"{fname}: return type {ret!r} has no ctypes mapping")
        argtypes = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            (base, stars, pname, dim), = _declarators(param, fname)
            where = f"{fname}({pname})"
            if dim:
                raise TypeError(f"{where}: an array parameter has no ctypes mapping")
            if (fname, pname) in pending:
                argtypes.append(pending.pop((fname, pname)))
            elif base.startswith("pd_"):
                if base not in structs or stars != 1:
                    raise TypeError(f"{where}: expected a pointer to a struct the header defines, not {param.strip()!r}")
                argtypes.append(C.POINTER(structs[base]))
            elif base == "void" and stars == 2:
                argtypes.append(C.POINTER(C.c_void_p))
            else:
                argtypes.append(_ctype(base, stars, dim, where))
        symbols[fname] = (RESTYPES[ret], argtypes)
    if pending:
        raise TypeError(f"out-parameters the header does not declare: {sorted(pending)}")
    if "pd_" in _PROTOTYPE.sub("", rest):
        raise TypeError("a pd_* declaration in the header is neither a struct typedef nor a prototype this reader understands: "
                        + " ".join(_PROTOTYPE.sub("", rest).split())[:200])
    return structs, symbols, constants
