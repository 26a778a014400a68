"""The ctypes binding is derived from include/diffute_hip.h at import (diffute_amd/_cheader.py, _cabi.py).  No GPU: the parser on a synthetic
header that holds every construct it has to read, its refusal of what it does not know, the host C compiler as the oracle for every struct
layout and constant of the real header, and the symbol list against an independent regex over the raw text."""
import ctypes
import keyword
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_ubyte, c_uint, c_uint64, c_void_p

import pytest

from diffute_amd import _cabi, _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diffute_hip.h")

SYNTHETIC = r"""
/* a comment with a declaration inside: int not_declared(int x); */
#ifndef T_H
#define T_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define T_OK 0
#define T_ERR_ARG (-1)          /* parenthesised negative */
#define T_MAX_W 0x7fffff00      // hex
#define T_RATIO 1.5
#define T_SHIFTED (1 << 3)
typedef void* t_stream_t;
typedef struct t_model t_model;
enum { T_KIND_A = 0, T_KIND_B = 1, T_KIND_C };
typedef struct t_coefs { float a, b; double c; } t_coefs;        /* tagged, multi-declarator */
typedef struct {                                                 /* anonymous */
  const void* in; int ld;       /* a Python keyword as a field name */
  long long* timing;
  int heads[4], n;
  unsigned long long addr; uint64_t addr2;
  unsigned int count; unsigned char tag, pad;
  t_coefs one;                  /* nested by value */
  t_coefs many[3];              /* array of structs */
  int64_t t; size_t bytes;
} t_desc;
int t_version(void);
const char* t_last_error(void);
void t_destroy(t_model* m);
t_model* t_create(const t_desc* d);
size_t t_bytes(const t_model* m, int B, long long ticks, unsigned flags);
int t_step(float* sample,
           size_t n, t_coefs coefs,
           int shape[4], t_stream_t stream);
int t_names(const t_model* m, const char** name, void* const* events, const char* key, char* buf, double scale, const int64_t* t);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_construct():
    h = _cheader.parse(SYNTHETIC, {"t_desc": "TDescIrregular"})
    assert list(h.structs) == ["t_coefs", "t_desc"]
    Coefs, Desc = h.structs["t_coefs"], h.structs["t_desc"]
    assert (Coefs.__name__, Desc.__name__) == ("Coefs", "TDescIrregular") and issubclass(Desc, ctypes.Structure)
    assert Coefs._fields_ == [("a", c_float), ("b", c_float), ("c", c_double)]
    assert Desc._fields_ == [("in_", c_void_p), ("ld", c_int), ("timing", c_void_p), ("heads", c_int * 4), ("n", c_int), ("addr", c_uint64),
                             ("addr2", c_uint64), ("count", c_uint), ("tag", c_ubyte), ("pad", c_ubyte), ("one", Coefs), ("many", Coefs * 3),
                             ("t", c_int64), ("bytes", c_size_t)]
    assert h.protos == {
        "t_version": (c_int, []),
        "t_last_error": (c_char_p, []),
        "t_destroy": (None, [c_void_p]),
        "t_create": (c_void_p, [c_void_p]),                       # a struct pointer is NOT POINTER(Struct): call sites pass c_void_p(device address)
        "t_bytes": (c_size_t, [c_void_p, c_int, c_int64, c_uint]),
        "t_step": (c_int, [c_void_p, c_size_t, Coefs, c_void_p, c_void_p]),
        "t_names": (c_int, [c_void_p, c_void_p, c_void_p, c_char_p, c_char_p, c_double, c_void_p]),
    }
    for argtypes in (a for _, a in h.protos.values()):
        assert all(a is not None for a in argtypes)
    assert "not_declared" not in h.protos
    assert [h.constant(n) for n in ("T_OK", "T_ERR_ARG", "T_MAX_W", "T_KIND_A", "T_KIND_B", "T_KIND_C")] == [0, -1, 0x7fffff00, 0, 1, 2]
    ctypes.c_void_p.from_param(ctypes.byref(Desc()))              # what the call sites pass where the header has a struct pointer
    ctypes.c_void_p.from_param(c_void_p(5))
    with pytest.raises(TypeError):
        ctypes.POINTER(Desc).from_param(c_void_p(5))              # ... and why the rule does not type them


@pytest.mark.parametrize("decl,named", [
    ("int t_f(long x);", "int t_f(long x)"),                                   # a scalar type the table does not hold
    ("int t_f(int a, t_unknown b);", "int t_f(int a, t_unknown b)"),           # an unknown struct by value
    ("typedef struct t_m t_m; int t_f(t_m m);", "int t_f(t_m m)"),             # an opaque handle by value
    ("int t_f(void (*cb)(int), int n);", "int t_f(void (*cb)(int), int n)"),   # a function-pointer parameter
    ("typedef struct t_s { short x; } t_s;", "t_s: short x"),                  # an unknown field type
    ("typedef struct t_s { int x[T_N]; } t_s;", "t_s: int x[T_N]"),            # an array length that is no literal
    ("typedef struct t_s { int x : 3; } t_s;", "t_s: int x : 3"),              # a bit field
    ("enum t_kind { T_A = 0 };", "enum t_kind { T_A = 0 }"),                   # a named enum
    ("enum { T_A = 1 << 2 };", "T_A = 1 << 2"),                                # an enumerator that is no plain integer
    ("#define T_F(x) (x)\nint t_f(int x);", "#define T_F(x) (x)"),             # a function-like macro
    ("#if 1\nint t_f(int x);\n#endif", "#if 1"),                               # a directive that could hide or change declarations
    ("int t_f(int x)", "int t_f(int x)"),                                      # a declaration that never ends
])
def test_parser_refuses_what_it_does_not_know(decl, named):
    with pytest.raises(_cheader.HeaderError) as e:
        _cheader.parse(decl)
    assert named in str(e.value), str(e.value)


def test_non_integer_macro_raises_when_asked_for():
    h = _cheader.parse(SYNTHETIC)                                  # holding such a macro is fine (an include guard has no value at all) ...
    for name in ("T_RATIO", "T_SHIFTED", "T_H", "T_NOT_THERE"):    # ... binding it is not
        with pytest.raises(_cheader.HeaderError) as e:
            h.constant(name)
        assert name in str(e.value)


def test_missing_header_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_cabi, "_HEADER_PATH", str(tmp_path / "include" / "diffute_hip.h"))
    with pytest.raises(RuntimeError, match="header is missing"):
        _cabi._read_header()


def _c_name(field):
    return field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field


def test_layouts_and_constants_match_the_c_compiler(tmp_path):
    """every struct size, field offset, field size and integer constant of the real header, as the host C compiler sees them"""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler on this machine")
    abi = _cabi._abi
    assert len(abi.structs) >= 17 and {"dmx_glyph_image", "dmx_multi_chunk"} <= set(abi.structs)
    consts = [n for n in list(abi.macros) + list(abi.enums) if n.startswith("DMX_")]
    assert len(consts) >= 30
    lines, want = [], []
    for cname, cls in abi.structs.items():
        assert getattr(_cabi, cls.__name__) is cls
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append((f"sizeof({cname})", ctypes.sizeof(cls)))
        for fname, _ in cls._fields_:
            lines.append(f'printf("%zu\\n%zu\\n", offsetof({cname}, {_c_name(fname)}), sizeof((({cname}*)0)->{_c_name(fname)}));')
            want += [(f"offsetof({cname}, {fname})", getattr(cls, fname).offset), (f"sizeof({cname}.{fname})", getattr(cls, fname).size)]
    for n in consts:
        lines.append(f'printf("%lld\\n", (long long)({n}));')
        want.append((n, getattr(_cabi, n[4:])))
    src = tmp_path / "abi_probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "diffute_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "abi_probe"
    r = subprocess.run([cc, "-x", "c", "-std=c99", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == len(want)
    bad = [(what, w, g) for (what, w), g in zip(want, got) if w != g]
    assert not bad, f"(what, ctypes, C compiler): {bad}"
    # the short names the host mirror uses for the decoder's state words
    assert all(getattr(_cabi, n[len("DMX_TROCR_"):]) == abi.constant(n) for n in consts if n.startswith(("DMX_TROCR_BEAM_", "DMX_TROCR_STATE_")))
    assert (_cabi.BEAM_WORDS, _cabi.STATE_FINISHED) == (abi.constant("DMX_TROCR_BEAM_WORDS"), abi.constant("DMX_TROCR_STATE_FINISHED"))


def test_every_declared_symbol_is_bound():
    raw = open(HEADER).read()
    declared = set(re.findall(r"\b(dmx_[a-z0-9_]+)\s*\(", raw))       # the independent reading tests/test_host.py uses
    assert declared == set(_cabi.exported_symbols()) and len(declared) >= 240
    for sym in declared:
        restype, argtypes = _cabi._PROTOS[sym]
        assert restype is None or isinstance(restype, type), sym
        assert isinstance(argtypes, list) and all(isinstance(a, type) for a in argtypes), sym
        n_params = re.search(r"(?m)^[A-Za-z_][\w \*]*\b" + sym + r"\s*\(([^()]*)\)\s*;", raw).group(1)     # (a declaration starts its line)
        assert len(argtypes) == (0 if n_params.strip() == "void" else len(n_params.split(","))), sym
