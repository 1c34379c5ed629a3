"""Reader of the C ABI header include/vexpress_hip.h: the ABI version, the enum constants, the parameter structs and the
prototypes, as ctypes types.  lib.py binds both libraries from it, so the header is the only statement of the contract.
include/vexpress_hip_guidance.h, include/vexpress_hip_samplers.h, include/vexpress_hip_solvers.h,
include/vexpress_hip_reuse.h and include/vexpress_hip_resize.h, the second to sixth header (entry points added without touching the earlier ones), are read
the same way.
Pure Python: no torch, no shared library.  It fails closed: once comments, preprocessor lines, the extern "C" braces and
every declaration it has understood are taken out, anything but whitespace left over is an ImportError naming it."""
import collections
import ctypes as C
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vexpress_hip.h")
GUIDANCE_HEADER = os.path.join(os.path.dirname(HEADER), "vexpress_hip_guidance.h")
SAMPLERS_HEADER = os.path.join(os.path.dirname(HEADER), "vexpress_hip_samplers.h")
SOLVERS_HEADER = os.path.join(os.path.dirname(HEADER), "vexpress_hip_solvers.h")
REUSE_HEADER = os.path.join(os.path.dirname(HEADER), "vexpress_hip_reuse.h")
RESIZE_HEADER = os.path.join(os.path.dirname(HEADER), "vexpress_hip_resize.h")

# version: int; enums: {name: value}; structs: {C name: [(field, ctypes type, array length or 0)]}; classes: {C name: the
# ctypes.Structure built from those fields}; functions: {name: (restype, [(parameter, ctypes type)])}, all in header order
Abi = collections.namedtuple("Abi", "version enums structs classes functions")

_SCALAR = {"int": C.c_int32, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "float": C.c_float}
_DECL = re.compile(r"\s*(const\s+)?(\w+)(\s*\*\s*|\s+)(\w+)\s*(?:\[(\d+)\])?\s*")      # [const] type [*] name [[n]]
_MORE = re.compile(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*")                                     # , name [[n]]
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_PROTO = re.compile(r"([\w\s*]*?)(\b\w+)\s*\(([^()]*)\)\s*;")


def _ctype(m, classes, where):
    const, base, star = m.group(1), m.group(2), "*" in m.group(3)
    if not star and not const and base in _SCALAR:
        return _SCALAR[base]
    if star and base in classes:
        return C.POINTER(classes[base])
    if star and not const and base == "int":
        return C.POINTER(C.c_int32)                  # a HOST array the library fills (vx_device_info)
    if star and (base == "void" or base in _SCALAR):
        return C.c_void_p                            # device pointers travel as integers
    raise ImportError(f"{where}: no ctypes type for {' '.join(m.group(0).split())!r}")


def parse(text, where=HEADER, macro="VX_ABI_VERSION"):
    """The Abi that the header `text` declares, its version the value of `macro`; ImportError (naming the text) for
    anything it does not understand."""
    abi = Abi(None, {}, {}, {}, {})

    def bad(what, s):
        return ImportError(f"{where}: {what} {' '.join(s.split())!r}")

    def enum(m):
        for item in filter(str.strip, m.group(1).split(",")):
            im = re.fullmatch(r"\s*(VX_[A-Z0-9_]+)\s*=\s*(-?\d+)\s*", item)
            if not im:
                raise bad("cannot read the enum constant", item)
            abi.enums[im.group(1)] = int(im.group(2))
        return ""

    def struct(m):
        name, fields = m.group(2), []
        if not re.fullmatch(r"vx_\w+_params", name):
            raise bad("a struct must be named vx_*_params, not", name)
        for decl in filter(str.strip, m.group(1).split(";")):
            first, *more = decl.split(",")
            dm, mm = _DECL.fullmatch(first), [_MORE.fullmatch(s) for s in more]
            if not dm or not all(mm) or (mm and "*" in dm.group(3)):
                raise bad(f"cannot read the field of {name}", decl)
            ctype = _ctype(dm, abi.classes, where)
            names = [dm.group(4, 5)] + [x.group(1, 2) for x in mm]
            fields += [(f, ctype, int(n or 0)) for f, n in names]
        abi.structs[name] = fields
        abi.classes[name] = type(name, (C.Structure,), {"_fields_": [(f, t * n if n else t) for f, t, n in fields]})
        return ""

    def proto(m):
        ret, name, params = " ".join(m.group(1).replace("*", " * ").split()), m.group(2), []
        restype = C.c_char_p if ret == "const char *" else _SCALAR.get(ret)
        if restype is None or not name.startswith("vx_") or name in abi.functions:
            raise bad("cannot bind the prototype", m.group(0))
        for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            pm = _DECL.fullmatch(p)
            if not pm or pm.group(5):
                raise bad(f"cannot read the parameter of {name}", p)
            params.append((pm.group(4), _ctype(pm, abi.classes, where)))
        abi.functions[name] = (restype, params)
        return ""

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+" + re.escape(macro) + r"[ \t]+(\d+)[ \t]*$", text, flags=re.M)
    if not version:
        raise ImportError(f"{where}: no `#define {macro} <number>`")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, count=1, flags=re.S)
    for pattern, reader in ((_ENUM, enum), (_STRUCT, struct), (_PROTO, proto)):     # structs before the prototypes that point to them
        text = pattern.sub(reader, text)
    if text.strip():
        raise bad("cannot read", text)
    return abi._replace(version=int(version.group(1)))


@functools.lru_cache(maxsize=None)
def header():
    """include/vexpress_hip.h, parsed once per process."""
    with open(HEADER) as f:
        return parse(f.read())


@functools.lru_cache(maxsize=None)
def guidance_header():
    """include/vexpress_hip_guidance.h, parsed once per process (version macro VX_GUIDANCE_ABI_VERSION)."""
    with open(GUIDANCE_HEADER) as f:
        return parse(f.read(), GUIDANCE_HEADER, "VX_GUIDANCE_ABI_VERSION")


@functools.lru_cache(maxsize=None)
def samplers_header():
    """include/vexpress_hip_samplers.h, parsed once per process (version macro VX_SAMPLERS_ABI_VERSION)."""
    with open(SAMPLERS_HEADER) as f:
        return parse(f.read(), SAMPLERS_HEADER, "VX_SAMPLERS_ABI_VERSION")


@functools.lru_cache(maxsize=None)
def solvers_header():
    """include/vexpress_hip_solvers.h, parsed once per process (version macro VX_SOLVERS_ABI_VERSION)."""
    with open(SOLVERS_HEADER) as f:
        return parse(f.read(), SOLVERS_HEADER, "VX_SOLVERS_ABI_VERSION")


@functools.lru_cache(maxsize=None)
def reuse_header():
    """include/vexpress_hip_reuse.h, parsed once per process (version macro VX_REUSE_ABI_VERSION)."""
    with open(REUSE_HEADER) as f:
        return parse(f.read(), REUSE_HEADER, "VX_REUSE_ABI_VERSION")


@functools.lru_cache(maxsize=None)
def resize_header():
    """include/vexpress_hip_resize.h, parsed once per process (version macro VX_RESIZE_ABI_VERSION)."""
    with open(RESIZE_HEADER) as f:
        return parse(f.read(), RESIZE_HEADER, "VX_RESIZE_ABI_VERSION")
