"""CPU tests of the binding derived from include/vexpress_hip.h (v_express_amd/abi.py): struct layout against a compiled C
probe, the whole binding against the copy pinned in tests/golden/abi_binding.json, both libraries bound, and the header
reader refusing what it does not understand.

Run as a script, this module re-records the pinned copy from the binding in force (after an ABI bump):
    python tests/test_abi_cpu.py"""
import ast
import ctypes
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = os.path.join(ROOT, "tests", "golden", "abi_binding.json")
STRUCTS = {"vx_gemm_params": "GemmParams", "vx_ff_params": "FfParams", "vx_tblock_params": "TBlockParams",
           "vx_axattn_params": "AxAttnParams"}           # C name -> attribute of v_express_amd.lib


def binding(lib):
    """The binding in force, as JSON data: what the loaded bf16 library's functions and lib's four structs carry, whoever set it."""
    names = {ctypes.c_int32: "c_int32", ctypes.c_uint32: "c_uint32", ctypes.c_int64: "c_int64", ctypes.c_float: "c_float",
             ctypes.c_void_p: "c_void_p", ctypes.c_char_p: "c_char_p"}
    names.update({getattr(lib, py): c for c, py in STRUCTS.items()})

    def name(t):
        return names[t] if t in names else f"POINTER({names[t._type_]})"

    def field(f, t):
        return [f, name(t._type_), t._length_] if issubclass(t, ctypes.Array) else [f, name(t), 0]
    functions = {n: [name(getattr(lib.lib, n).restype), [name(t) for t in getattr(lib.lib, n).argtypes or []]]
                 for n in lib.declared_symbols()}
    structs = {c: [field(*f) for f in getattr(lib, py)._fields_] for c, py in STRUCTS.items()}
    return {"abi": lib.lib.vx_abi_version(), "functions": functions, "structs": structs}


def record():
    sys.path.insert(0, ROOT)
    from v_express_amd import lib
    with open(PINNED, "w") as f:
        json.dump(binding(lib), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {PINNED}")


@functools.lru_cache(maxsize=None)
def probed_layout():
    """{struct: (sizeof, {field: (offsetof, sizeof)})} of every parsed field, as gcc lays include/vexpress_hip.h out."""
    from v_express_amd import abi
    structs = abi.header().structs
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "vexpress_hip.h"\nint main(void){\n'
    for s, fields in structs.items():
        src += f'printf("{s} %zu\\n", sizeof({s}));\n'
        src += "".join(f'printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));\n' for f, _, _ in fields)
    src += "return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.dirname(abi.HEADER), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        lines = subprocess.check_output([os.path.join(d, "p")], text=True).splitlines()
    out = {s: [None, {}] for s in structs}
    for s, *rest in map(str.split, lines):
        if len(rest) == 1:
            out[s][0] = int(rest[0])
        else:
            out[s][1][rest[0]] = (int(rest[1]), int(rest[2]))
    return out


def ctypes_layout(cls):
    return [ctypes.sizeof(cls), {f: (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_}]


def test_param_structs_match_header_layout():
    """sizeof, and offsetof / sizeof of EVERY field, of the four parameter structs: the ctypes classes against a C probe
    compiled from include/vexpress_hip.h."""
    from v_express_amd import abi, lib
    assert sorted(abi.header().structs) == sorted(STRUCTS)
    for c, py in STRUCTS.items():
        cls = getattr(lib, py)
        assert cls is abi.header().classes[c] and [f for f, _ in cls._fields_] == [f for f, _, _ in abi.header().structs[c]]
        assert ctypes_layout(cls) == probed_layout()[c], c
    assert {c: len(f) for c, f in abi.header().structs.items()} == {"vx_gemm_params": 58, "vx_ff_params": 15,
                                                                    "vx_tblock_params": 15, "vx_axattn_params": 19}


def test_axattn_params_struct_matches_header_layout():
    """vx_axattn_params (ABI 15): the ctypes mirror against a C probe compiled from include/vexpress_hip.h; and the entry
    point validates its arguments before any launch (no GPU needed)."""
    from v_express_amd import lib
    A = lib.AxAttnParams
    assert ctypes_layout(A) == probed_layout()["vx_axattn_params"]
    assert lib.lib.vx_audio_xattn_supported(320, 8, 5, 4096) == 1 and lib.lib.vx_audio_xattn_supported(1280, 8, 5, 64) == 1
    assert lib.lib.vx_audio_xattn_supported(320, 8, 4, 4096) == 0 and lib.lib.vx_audio_xattn_supported(64, 8, 5, 64) == 0
    assert lib.lib.vx_audio_xattn_packed_bytes(320, 16) == 16 * 320 * 96
    rc = lib.lib.vx_audio_xattn(ctypes.byref(A()), None)
    assert rc < 0 and b"vx_audio_xattn" in lib.lib.vx_last_error_string()


def test_binding_equals_the_pinned_copy():
    """tests/golden/abi_binding.json was recorded from the hand-written binding this one replaced (the six `(void)` functions,
    whose argtypes that one left unset, as []).  The derived binding must equal it as long as the ABI version does: a
    signature that changes without an ABI bump fails here."""
    from v_express_amd import abi, lib
    with open(PINNED) as f:
        pinned = json.load(f)
    assert abi.header().version == pinned["abi"], (
        f"include/vexpress_hip.h is ABI {abi.header().version}, tests/golden/abi_binding.json pins ABI {pinned['abi']}: "
        "review the change and re-record the file (python tests/test_abi_cpu.py)")
    got = binding(lib)
    assert sorted(got["functions"]) == sorted(pinned["functions"])
    for n, sig in pinned["functions"].items():
        assert got["functions"][n] == sig, n
    assert got["structs"] == pinned["structs"]
    assert [n for n, sig in got["functions"].items() if not sig[1]] == sorted(
        ["vx_abi_version", "vx_build_id", "vx_element_type", "vx_gemm_last_kernel", "vx_last_error_string", "vx_last_kernel"])


def test_both_libraries_are_bound_from_one_parse():
    from v_express_amd import abi, lib
    functions = abi.header().functions
    assert abi.header() is abi.header() and lib.declared_symbols() == sorted(functions) and len(functions) == 59
    assert (lib.VX_EPI_STORE, lib.VX_EPI_GEGLU, lib.VX_EPI_SPLIT, lib.VX_PART_ROWS, lib.VX_PART_VT, lib.VX_ACT_NONE,
            lib.VX_ACT_SILU, lib.VX_ACT_GELU) == (0, 1, 2, 0, 1, 0, 1, 2) and len(abi.header().enums) == 8
    for so in (lib.lib, lib.lib_f16()):
        bound = 0
        for n in lib.declared_symbols():
            fn, (restype, params) = so.__dict__[n], functions[n]        # __dict__: the function objects _load touched
            assert fn.restype is restype and fn.argtypes is not None and list(fn.argtypes) == [t for _, t in params], n
            bound += 1
        assert bound == 59


def test_header_reader_is_pure_python():
    from v_express_amd import abi
    tree = ast.parse(open(abi.__file__).read())
    imported = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    assert not [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert imported == {"collections", "ctypes", "functools", "os", "re"}
    assert "CDLL" not in open(abi.__file__).read()


SYNTHETIC = '''/* a header in the style of include/vexpress_hip.h */
#ifndef DEMO_H
#define DEMO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define VX_ABI_VERSION 7
enum { VX_A = 0, VX_B = 2 };   /* comment */
typedef struct {
  const void* a;             /* a comment; with, punctuation (and brackets) */
  int c1, c2;
  void* part_out[3];
  int32_t part_ld[3];
  const float* bias;
  float alpha;
} vx_demo_params;
const char* vx_name(void);
int vx_run(const vx_demo_params* p, int* out4, const int32_t* ids,
           uint32_t seed, int64_t n, float s, void* stream);
int64_t vx_bytes(int m);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_synthetic_header_parses_to_the_expected_structure():
    from v_express_amd import abi
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    a = abi.parse(SYNTHETIC, "demo.h")
    assert a.version == 7 and a.enums == {"VX_A": 0, "VX_B": 2}
    assert a.structs == {"vx_demo_params": [("a", vp, 0), ("c1", i32, 0), ("c2", i32, 0), ("part_out", vp, 3),
                                            ("part_ld", i32, 3), ("bias", vp, 0), ("alpha", ctypes.c_float, 0)]}
    D = a.classes["vx_demo_params"]
    assert issubclass(D, ctypes.Structure) and [f for f, _ in D._fields_] == ["a", "c1", "c2", "part_out", "part_ld", "bias", "alpha"]
    assert D.part_out.size == 24 and D.part_ld.offset == 40 and D.part_ld.size == 12 and ctypes.sizeof(D) == 72
    assert list(a.functions) == ["vx_name", "vx_run", "vx_bytes"]
    assert a.functions["vx_name"] == (ctypes.c_char_p, [])
    assert a.functions["vx_run"] == (i32, [("p", ctypes.POINTER(D)), ("out4", ctypes.POINTER(i32)), ("ids", vp),
                                           ("seed", ctypes.c_uint32), ("n", ctypes.c_int64), ("s", ctypes.c_float), ("stream", vp)])
    assert a.functions["vx_bytes"] == (ctypes.c_int64, [("m", i32)])


@pytest.mark.parametrize("old,new,named", [
    ("int64_t vx_bytes(int m);", "int64_t vx_bytes(double m);", "double m"),                              # unknown type
    ("int64_t vx_bytes(int m);", "int vx_each(void (*cb)(int), void* stream);", "void (*cb)(int)"),       # function pointer
    ("int64_t vx_bytes(int m);", "static int x;\nint64_t vx_bytes(int m);", "static int x;"),             # not a declaration of the ABI
    ("int64_t vx_bytes(int m);", "int64_t foo(int m);", "foo(int m)"),                                    # outside the vx_ namespace
    ("  float alpha;", "  double alpha;", "double alpha"),                                                # untypable field
    ("#define VX_ABI_VERSION 7", "", "VX_ABI_VERSION"),                                                   # no version
    ("int64_t vx_bytes(int m);", "double vx_bytes(int m);", "double vx_bytes"),                           # unknown return type
    ("  int c1, c2;", "  void* c1, c2;", "void* c1, c2"),                                                 # `*` binds to c1 only
    ("int64_t vx_bytes(int m);", "int64_t vx_bytes(int m[4]);", "int m[4]"),                              # array parameter
    ("int64_t vx_bytes(int m);", "int64_t vx_bytes(int m);\nint vx_name(int again);", "vx_name(int again)"),   # declared twice
    ("enum { VX_A = 0, VX_B = 2 };", "enum { VX_A = 0, VX_B };", "VX_B"),                                 # implicit enum value
    ("} vx_demo_params;", "} demo_t;", "demo_t"),                                                         # struct outside the namespace
])
def test_header_reader_fails_closed(old, new, named):
    from v_express_amd import abi
    assert SYNTHETIC.count(old) == 1
    with pytest.raises(ImportError) as e:
        abi.parse(SYNTHETIC.replace(old, new), "demo.h")
    assert named in str(e.value) and "demo.h" in str(e.value)


if __name__ == "__main__":
    record()
