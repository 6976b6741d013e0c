"""CPU: `instantir_amd.cheader`, the strict parser the ctypes binding is derived with, on small header strings -- every
construct include/instantir_hip.h uses is accepted, and everything else raises and names the text (nothing is skipped)."""
import ctypes as C

import pytest

from instantir_amd.cheader import HipLibraryError, parse, parse_file

KV = "typedef struct kv { const void* K; int64_t ldk, k_batch_stride; int32_t T; } kv;\n"


def fields(cls):
    return [(name, t, getattr(cls, name).offset) for name, t in cls._fields_]


def test_integer_macros():
    h = parse("#ifndef GUARD_H\n#define GUARD_H\n#include <stdint.h>\n#define IIR_A 3\n#define IIR_B  8u   /* bit */\n#endif\n")
    assert h.macros == {"IIR_A": 3, "IIR_B": 8} and not h.structs and not h.functions


def test_several_declarators_const_and_data_pointers():
    h = parse(KV + "typedef struct s { const float *x, *y;  float *z; uint32_t g; uint64_t seed; float f; int n; double* out; } s;")
    assert list(h.structs) == ["kv", "s"]
    assert fields(h.structs["kv"]) == [("K", C.c_void_p, 0), ("ldk", C.c_int64, 8), ("k_batch_stride", C.c_int64, 16), ("T", C.c_int32, 24)]
    assert [(n, t) for n, t, _ in fields(h.structs["s"])] == [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("g", C.c_uint32),
                                                              ("seed", C.c_uint64), ("f", C.c_float), ("n", C.c_int), ("out", C.c_void_p)]


def test_pointer_to_and_array_of_an_earlier_struct():
    h = parse(KV + "typedef struct d { const kv* one; kv two[2]; int32_t after; } d;")
    kv, d = h.structs["kv"], h.structs["d"]
    assert d._fields_[0][1] is C.POINTER(kv) and d._fields_[1][1] is kv * 2
    assert d.after.offset == 8 + 2 * C.sizeof(kv) and C.sizeof(kv) == 32


def test_anonymous_struct_typedef():
    h = parse("typedef struct {\n    const void* src; int32_t src_u8;\n    float* dst;\n} IirDesc;\nint run(const IirDesc* d, void* stream);")
    assert list(h.structs) == ["IirDesc"] and h.structs["IirDesc"].__name__ == "IirDesc"
    assert h.functions["run"] == (C.c_int, [("d", C.POINTER(h.structs["IirDesc"])), ("stream", C.c_void_p)])


def test_prototypes():
    h = parse(KV + 'extern "C" {\nvoid* create(void);\nvoid destroy(void* e);\nint64_t bytes(int32_t B, uint64_t seed);\n'
              "int run(const kv* a, const float* w, float eps, int64_t ld,\n"
              "        uint32_t bits,\n"
              "        void* stream);\n}\n")
    assert h.functions["create"] == (C.c_void_p, []) and h.functions["destroy"] == (None, [("e", C.c_void_p)])
    assert h.functions["bytes"] == (C.c_int64, [("B", C.c_int32), ("seed", C.c_uint64)])
    assert h.functions["run"] == (C.c_int, [("a", C.POINTER(h.structs["kv"])), ("w", C.c_void_p), ("eps", C.c_float), ("ld", C.c_int64),
                                            ("bits", C.c_uint32), ("stream", C.c_void_p)])
    assert list(h.functions) == ["create", "destroy", "bytes", "run"]


def test_comments_may_hold_declaration_punctuation(tmp_path):
    text = "/* f(x); { int y; } // not a comment\n * int hidden(void); */\nint shown(void); /* (a; b) { */\n"
    assert list(parse(text).functions) == ["shown"]
    (tmp_path / "h.h").write_text(text)
    assert list(parse_file(str(tmp_path / "h.h")).functions) == ["shown"]


@pytest.mark.parametrize("text, named", [
    ("typedef struct s { unsigned long n; } s;", "unsigned long n"),
    ("typedef struct s { int (*cb)(int); } s;", "int (*cb)(int)"),
    ("int (*cb)(int);", "int (*cb)(int);"),
    ("int run(int (*cb)(int));", "int (*cb)(int)"),
    ("#define IIR_X (1 << 3)", "#define IIR_X (1 << 3)"),
    ("#define IIR_F(x) 3", "#define IIR_F(x) 3"),
    ("#if 0\nint f(void);\n#endif", "#if 0"),
    ("typedef struct s { int32_t a : 3; } s;", "int32_t a : 3"),
    ("int f(void); // int g(void);", "// int g(void);"),
    ("int32_t iir_global;", "int32_t iir_global;"),
    ("struct tagged;", "struct tagged;"),
    ("enum { IIR_E = 1 };", "enum { IIR_E = 1 };"),
    ("static inline int f(void);", "static inline"),
    ("int f(size_t n);", "size_t"),
    ("int f(kv a);", "kv"),
    ("int f(int32_t a[2]);", "int32_t a[2]"),
    ("int f(void v);", "void v"),
    ("int f();", "int f();"),
    ("typedef struct s { later* p; } s; typedef struct later { int n; } later;", "later"),
])
def test_anything_else_raises_and_names_the_text(text, named):
    with pytest.raises(HipLibraryError) as e:
        parse(text)
    assert named in str(e.value)
