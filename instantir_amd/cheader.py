"""Strict parser of the C subset include/instantir_hip.h is written in: the single source of the ctypes binding (lib.py).

`parse(text)` returns the three things such a header declares: the integer macros, the structs as generated
`ctypes.Structure` classes and the prototypes as (restype, [(parameter name, ctype), ...]).  Whatever is left once the
comments, the preprocessor lines and the recognised declarations are taken out, other than the `extern "C"` braces, raises
HipLibraryError with the offending text: nothing is skipped silently.  No torch, no GPU.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple


class HipLibraryError(RuntimeError):
    pass


class Header(NamedTuple):
    macros: dict       # IIR_NAME -> int
    structs: dict      # C typedef name -> ctypes.Structure subclass, in declaration order
    functions: dict    # name -> (restype, [(parameter name, ctype), ...])


# The type rule.  Scalars map by name; a pointer to a struct the header declared is POINTER(that struct), in fields and in
# parameters; every other pointer, whatever it points to, is a raw address.
SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float,
           "int": C.c_int}
POINTEES = ("void", "double")      # types the subset knows behind a `*` only


def _ctype(base, pointer, structs, where):
    if base not in SCALARS and base not in structs and base not in POINTEES:
        raise HipLibraryError(f"unknown type `{base}` in `{where}`")
    if pointer:
        return C.POINTER(structs[base]) if base in structs else C.c_void_p
    if base in POINTEES:
        raise HipLibraryError(f"`{base}` by value in `{where}`")
    return SCALARS.get(base) or structs[base]


def _declaration(text, structs, field, where):
    """`[const] type declarator[, declarator ...]` -> [(name, ctype)].  A parameter is one declarator and never an array."""
    text = " ".join(text.split())
    m = re.fullmatch(r"(?:const )?(\w+)\b ?(.+)", text)
    decls = [re.fullmatch(r"(\*?) ?(\w+) ?(?:\[(\d+)\])?", d.strip()) for d in m.group(2).split(",")] if m else [None]
    if None in decls or (not field and (len(decls) > 1 or decls[0].group(3))):
        raise HipLibraryError(f"unsupported declaration `{text}` in `{where}`")
    out = []
    for star, name, count in (d.groups() for d in decls):
        ct = _ctype(m.group(1), star, structs, where)
        out.append((name, ct * int(count) if count else ct))
    return out


def parse(text: str) -> Header:
    macros, structs, functions = {}, {}, {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    if "//" in text:
        raise HipLibraryError("`//` comment: `" + re.search(r"//.*", text).group(0)[:120] + "`")

    def directive(m):
        line = " ".join(m.group(0).split())
        value = re.fullmatch(r"# ?define (IIR_\w+) (\d+)u?", line)
        if value:
            macros[value.group(1)] = int(value.group(2))
        elif not re.fullmatch(r"# ?(define \w+|include <\w+\.h>|ifdef \w+|ifndef \w+|endif)", line):
            raise HipLibraryError(f"unsupported preprocessor line `{line}`")
        return ""

    def struct(m):
        fields = [f for d in m.group(1).split(";") if d.strip() for f in _declaration(d, structs, True, "struct " + m.group(2))]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return ""

    def prototype(m):
        ret, star, name, params = m.group(1), m.group(2).strip(), m.group(3), m.group(4)
        where = " ".join(m.group(0).split())
        params = [] if params.strip() == "void" else [_declaration(p, structs, False, where)[0] for p in params.split(",")]
        functions[name] = (None if (ret, star) == ("void", "") else _ctype(ret, star, structs, where), params)
        return ""

    text = re.sub(r"^[ \t]*#.*$", directive, text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"(?:\bconst\s+)?\b(\w+)(\s*\*\s*|\s+)(\w+)\s*\(([^()]*)\)\s*;", prototype, text)
    rest = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S).split()
    if rest:
        raise HipLibraryError("unrecognised text in the header: `" + " ".join(rest)[:120] + "`")
    return Header(macros, structs, functions)


def parse_file(path: str) -> Header:
    with open(path) as f:
        return parse(f.read())
