"""CPU: the C-ABI library builds, loads and exports every symbol include/instantir_hip.h declares
(no compute calls -- there is no GPU here)."""
import ctypes
import os

from instantir_amd import lib


def test_header_symbols_have_bindings():
    syms = lib.declared_symbols()
    assert len(syms) >= 17 and "iir_gemm_f16" in syms and "iir_attention_d64_f16" in syms
    assert sorted(syms) == sorted(lib.SIGNATURES)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(lib.LIB_PATH), "build instantir_amd/csrc/build.sh first (python -c 'import __graft_entry__ as g; g.build()')"
    h = ctypes.CDLL(lib.LIB_PATH)
    for s in lib.declared_symbols():
        assert hasattr(h, s), s
    h.iir_abi_version.restype = ctypes.c_int
    assert h.iir_abi_version() == 3
    # and the other way round: every function the library exports under the iir_ prefix is one the header declares
    import shutil
    import subprocess
    nm = shutil.which("nm") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] == "T"]
    assert len(exported) >= len(lib.SIGNATURES)
    assert [s for s in exported if s.startswith("iir_") and s not in lib.SIGNATURES] == []


def test_k_split_workspace_has_left_the_abi():
    """The two-slice K split went out of the library with ABI version 2: no workspace field of it in either descriptor, neither
    of its two query functions declared -- nothing in the header or its ctypes mirror names a split any more."""
    for desc in (lib.GemmDesc, lib.ConvDesc):
        assert not [name for name, _ in desc._fields_ if "split" in name]
    assert not [s for s in list(lib.declared_symbols()) + list(lib.SIGNATURES) if "split" in s]
    assert "split" not in open(lib.HEADER_PATH).read().lower()


def test_positional_step_entries_have_left_the_abi():
    """The CFG + scheduler step went onto a descriptor with ABI version 3 (iir_sched_desc, iir_sched_step, iir_cfg_rescale_factor):
    none of the positional spellings of the same two launches is declared, bound or exported any more."""
    gone = ("iir_sched_step_hist", "iir_sched_step_pag", "iir_sched_step_hist_pag", "iir_sched_step_keep", "iir_sched_step_apg",
            "iir_cfg_rescale_factor_pag")
    h = ctypes.CDLL(lib.LIB_PATH)
    syms = lib.declared_symbols()
    for s in gone:
        assert s not in syms and s not in lib.SIGNATURES and not hasattr(h, s), s
    # the seventh, the 14-argument iir_sched_step, gave its name to the descriptor entry
    assert lib.SIGNATURES["iir_sched_step"][1][0] == ctypes.POINTER(lib.SchedDesc) and len(lib.SIGNATURES["iir_sched_step"][1]) == 2
    assert lib.SIGNATURES["iir_cfg_rescale_factor"][1][0] == ctypes.POINTER(lib.SchedDesc)
    text = open(lib.HEADER_PATH).read()
    assert "iir_sched_step(const iir_sched_desc* d, void* stream)" in text


def _kind(t):
    """A ctypes restype / argtype / field type as the probe program prints it: class, size and, for a pointer to a declared
    struct, which struct."""
    if t is None:
        return "void 0 -"
    if t is ctypes.c_void_p:
        return "pointer %d -" % ctypes.sizeof(t)
    if hasattr(t, "contents"):
        return "pointer %d %s" % (ctypes.sizeof(t), t._type_.__name__)
    code = t._type_
    return "%s %d -" % ("float" if code in "fd" else "signed" if code.islower() else "unsigned", ctypes.sizeof(t))


def _abi_facts(header):
    """Everything `cheader` derived from a header, as {key: value} strings: the layout of every struct and field, the class of
    every return value and parameter, the value of every macro."""
    facts = {"macro " + name: str(value) for name, value in header.macros.items()}
    for name, cls in header.structs.items():
        facts["struct " + name] = "%d %d" % (ctypes.sizeof(cls), ctypes.alignment(cls))
        for field, _ in cls._fields_:
            facts["field %s.%s" % (name, field)] = "%d %d" % (getattr(cls, field).offset, getattr(cls, field).size)
    for name, (restype, params) in header.functions.items():
        facts["arity " + name] = str(len(params))
        for i, t in enumerate([restype] + [ct for _, ct in params]):
            facts["type %s %d" % (name, i - 1)] = _kind(t)            # -1: the return value
    return facts


_PROBE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "%(header)s"
template <class T> const char* struct_name() { return "-"; }
%(names)s
template <class T> void kind(const char* fn, int i) {
    using U = std::remove_cv_t<T>;
    const char* k = std::is_void_v<U> ? "void" : std::is_pointer_v<U> ? "pointer" : std::is_floating_point_v<U> ? "float"
                  : !std::is_integral_v<U> ? "other" : std::is_signed_v<U> ? "signed" : "unsigned";
    size_t size = 0;
    if constexpr (!std::is_void_v<U>) size = sizeof(U);
    std::printf("type %%s %%d|%%s %%zu %%s\n", fn, i, k, size, struct_name<std::remove_cv_t<std::remove_pointer_t<U>>>());
}
template <class F> struct signature;
template <class R, class... A> struct signature<R (*)(A...)> {
    static void print(const char* fn) {
        std::printf("arity %%s|%%zu\n", fn, sizeof...(A));
        int i = -1;
        kind<R>(fn, i++);
        (kind<A>(fn, i++), ...);
    }
};
int main() {
%(body)s
}
"""


def _probe_source(header, header_path):
    """The C++17 program that prints the same facts as `_abi_facts`, as the compiler sees the header at `header_path`."""
    names = ['template <> const char* struct_name<%s>() { return "%s"; }' % (s, s) for s in header.structs]
    body = ['std::printf("macro %s|%%lld\\n", (long long)%s);' % (m, m) for m in header.macros]
    for s, cls in header.structs.items():
        body.append('std::printf("struct %s|%%zu %%zu\\n", sizeof(%s), alignof(%s));' % (s, s, s))
        body += ['std::printf("field %s.%s|%%zu %%zu\\n", offsetof(%s, %s), sizeof(%s::%s));' % (s, f, s, f, s, f) for f, _ in cls._fields_]
    body += ['signature<decltype(&%s)>::print("%s");' % (f, f) for f in header.functions]        # unevaluated: nothing to link
    return _PROBE % dict(header=header_path, names="\n".join(names), body="\n".join("    " + b for b in body))


def _compiler_facts(header, header_path, workdir):
    import shutil
    import subprocess
    import pytest
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("g++") or shutil.which("c++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or ROCm's clang++) to ask about the header's layout")
    src, exe = os.path.join(workdir, "abi_probe.cpp"), os.path.join(workdir, "abi_probe")
    with open(src, "w") as f:
        f.write(_probe_source(header, header_path))
    subprocess.run([cxx, "-std=c++17", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return dict(line.split("|") for line in out.splitlines())


def test_derived_binding_matches_the_compiler(tmp_path):
    """Everything the binding derives from the header, against a host C++ compiler that includes the same header: sizeof and
    alignof of every struct, offsetof and sizeof of every field, the class and size of every return value and parameter (and the
    struct behind a struct pointer), the value of every macro.  A field or function the header lacks fails at compile time."""
    header = lib.HEADER
    derived = _abi_facts(header)
    assert len(header.structs) >= 8 and len(header.functions) >= 62 and len(header.macros) >= 27 and len(derived) > 600
    assert all(ctypes.sizeof(s) % 8 == 0 for s in header.structs.values()) and ctypes.sizeof(lib.AttnKV) == 56
    compiled = _compiler_facts(header, lib.HEADER_PATH, str(tmp_path))
    assert {k: (v, compiled.get(k)) for k, v in derived.items() if v != compiled.get(k)} == {}
    assert sorted(derived) == sorted(compiled)
    # the names the package exports are those classes and values
    exported = dict(iir_attn_kv=lib.AttnKV, iir_gemm_desc=lib.GemmDesc, iir_conv_desc=lib.ConvDesc, iir_attn_desc=lib.AttnDesc,
                    iir_adaln_job=lib.AdaLNJob, iir_sched_desc=lib.SchedDesc, IirResampleDesc=lib.ResampleDesc,
                    iir_metrics_desc=lib.MetricsDesc)
    assert list(header.structs) == list(exported) and all(header.structs[n] is exported[n] for n in exported)
    assert lib.MACROS is header.macros and sorted(lib.SIGNATURES) == sorted(header.functions)


def test_signatures_follow_the_type_rule_but_for_device_tables():
    """lib.SIGNATURES is the header's prototypes under cheader's type rule.  lib.DEVICE_TABLES, the one exception, names
    parameters the header has, each a pointer to a declared struct that the rule alone binds as POINTER(struct); there the
    binding takes an integer device address."""
    import pytest
    assert lib.DEVICE_TABLES == {("iir_adaln_batch_f16", "jobs_dev")}
    seen = set()
    for fn, (restype, params) in lib.HEADER.functions.items():
        bound_ret, bound = lib.SIGNATURES[fn]
        assert bound_ret is restype and len(bound) == len(params), fn
        for (param, ct), b in zip(params, bound):
            if (fn, param) in lib.DEVICE_TABLES:
                seen.add((fn, param))
                assert ct is ctypes.POINTER(lib.AdaLNJob) and b is ctypes.c_void_p, (fn, param)
                b.from_param(0x7F0000001000)
                with pytest.raises(TypeError):
                    ct.from_param(0x7F0000001000)
            else:
                assert b is ct, (fn, param)
    assert seen == lib.DEVICE_TABLES


def _mutated_facts(tmp_path, old, new):
    from instantir_amd import cheader
    text = open(lib.HEADER_PATH).read()
    assert text.count(old) == 1
    path = tmp_path / "mutated.h"
    path.write_text(text.replace(old, new))
    real, mutated = _abi_facts(lib.HEADER), _abi_facts(cheader.parse_file(str(path)))
    assert sorted(real) == sorted(mutated)
    return {k: (real[k], mutated[k]) for k in real if real[k] != mutated[k]}


def test_swapped_fields_change_exactly_their_offsets(tmp_path):
    """Two adjacent int32_t fields of iir_gemm_desc swapped in a copy of the header: the facts the compiler is asked about differ
    in those two offsets and nowhere else, so the comparison above sees such a swap."""
    diff = _mutated_facts(tmp_path, "int32_t epi, act;\n    float out_scale;               /* 0 means 1",
                          "int32_t act, epi;\n    float out_scale;               /* 0 means 1")
    epi, act = lib.GemmDesc.epi.offset, lib.GemmDesc.act.offset
    assert act == epi + 4
    assert diff == {"field iir_gemm_desc.epi": ("%d 4" % epi, "%d 4" % act), "field iir_gemm_desc.act": ("%d 4" % act, "%d 4" % epi)}


def test_widened_parameter_changes_exactly_its_type(tmp_path):
    """One int32_t parameter of iir_layernorm_f16 declared int64_t in a copy of the header: one fact differs."""
    diff = _mutated_facts(tmp_path, "int32_t rows, int32_t C, const void* gamma,\n                      const void* beta",
                          "int64_t rows, int32_t C, const void* gamma,\n                      const void* beta")
    assert diff == {"type iir_layernorm_f16 4": ("signed 4 -", "signed 8 -")}


def test_invalid_arguments_are_rejected_without_a_gpu():
    """Argument validation happens before any HIP call, so it can be exercised on CPU."""
    h = lib.load()
    d = lib.GemmDesc()
    assert h.iir_gemm_f16(ctypes.byref(d), None) == -1            # null pointers
    d.A = d.W = d.C = 4096
    d.M, d.N, d.K = 8, 8, 48                                       # K not a multiple of 64
    assert h.iir_gemm_f16(ctypes.byref(d), None) == -1
    c = lib.ConvDesc()
    c.X = c.Wt = c.Y = c.zero_page = 4096
    c.ksize, c.Cin, c.stride = 5, 64, 1
    assert h.iir_conv2d_nhwc_f16(ctypes.byref(c), None) == -1
    a = lib.AttnDesc()
    a.Q = a.O = 4096
    a.nseg = 3
    assert h.iir_attention_d64_f16(ctypes.byref(a), None) == -1
    assert h.iir_silu_f16(4096, 4096, 7, None) == -1              # n % 8
    import torch
    if torch.cuda.is_available():      # the calls below are valid but for one argument: on a GPU a miss would launch on address 4096
        return
    P = 4096
    ln = lambda C=64, ldx=64, ldy=64, tr=0, rows=4: h.iir_layernorm_f16(P, ldx, P, ldy, rows, C, None, None, 1e-5, None, None, 0, 1, tr, 1, 0, None)
    assert ln() != -1                                              # the valid call passes validation (and fails at the launch)
    assert ln(C=0) == -1 and ln(C=-8) == -1 and ln(ldx=56) == -1 and ln(ldy=56) == -1 and ln(tr=2, ldy=56) == -1
    assert ln(tr=1, ldy=4) != -1                                   # transposed: ldy is the stride of the transposed rows
    for entry in (h.iir_groupnorm_nhwc, None):
        def gn(C=64, ldx=64, ldy=64, groups=32, ldp=64, HW=64):
            if entry is None:
                return h.iir_groupnorm_from_partials(P, ldp, P, ldx, P, ldy, 1, HW, C, groups, P, P, 1e-5, 0, P, 1 << 20, 0, None)
            return entry(P, ldx, P, ldy, 1, HW, C, groups, P, P, 1e-5, 0, P, 1 << 20, 0, None)
        assert gn() != -1
        assert gn(C=0) == -1 and gn(C=-64) == -1 and gn(ldx=56) == -1 and gn(ldy=56) == -1 and gn(C=8, groups=16) == -1
        assert gn(C=24, groups=64) == -1
    assert h.iir_groupnorm_from_partials(P, 56, P, 64, P, 64, 1, 64, 64, 32, P, P, 1e-5, 0, P, 1 << 20, 0, None) == -1      # ldp < C
    assert h.iir_softmax_rows_f16(P, 64, 2, 64, None) != -1 and h.iir_softmax_rows_f16(P, 56, 2, 64, None) == -1
    assert h.iir_softmax_rows_f32(P, 64, P, 64, 2, 64, 0, None) != -1
    assert h.iir_softmax_rows_f32(P, 60, P, 64, 2, 64, 0, None) == -1 and h.iir_softmax_rows_f32(P, 64, P, 60, 2, 64, 1, None) == -1


def test_norm_wrappers_refuse_mismatched_shapes():
    """The `ops` checks that come before the device test: shapes and column counts of groupnorm / layernorm / adaln_job_table /
    softmax_rows_f32, on CPU tensors."""
    import pytest
    import torch
    from instantir_amd import ops
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)
    x, g = z(128, 64), z(64)
    for bad in (dict(out=z(128, 72)), dict(out=z(64, 64)), dict(R=3), dict(gamma=z(72)), dict(beta=z(32)), dict(x=z(128, 64)[:, :56], out=z(128, 56))):
        a = dict(x=x, out=z(128, 64), R=2, HW=64, gamma=g, beta=g, eps=1e-5, silu=False)
        a.update(bad)
        with pytest.raises(ValueError, match="groupnorm"):
            ops.groupnorm(**a)
    for bad in (dict(out=z(128, 72)), dict(out=z(120, 64)), dict(gamma=z(72)), dict(beta=z(8)), dict(shift=z(8, 72), scale=z(8, 64), rows_per_mod=16),
                dict(shift=z(8, 64), scale=z(8, 56), rows_per_mod=16), dict(shift=z(8, 64), rows_per_mod=16), dict(shift=z(7, 64), scale=z(7, 64), rows_per_mod=16),
                dict(out=z(64, 100), transposed=True, tr_rows=16, tr_bstride=16), dict(out=z(72, 128), transposed=True, tr_rows=16, tr_bstride=16),
                dict(out=z(64, 128), transposed=True, tr_rows=16, tr_bstride=24), dict(out=z(128, 72, dt=torch.uint8))):
        a = dict(x=x, out=z(128, 64))
        a.update(bad)
        with pytest.raises(ValueError, match="layernorm"):
            ops.layernorm(**a)
    ok = (z(32, 64), z(32, 64), z(2, 64), z(2, 64), False)
    for i, bad in ((0, z(32, 2568)), (0, z(32, 4)), (0, z(32, 60)), (1, z(32, 72)), (1, z(31, 64)), (2, z(2, 72)), (3, z(2, 56))):
        job = list(ok)
        job[i] = bad
        if i == 0:
            job[1] = torch.zeros_like(bad)
        with pytest.raises(ValueError, match="adaln job 0"):
            ops.adaln_job_table([tuple(job)], "cpu")
    for out in (z(60, 32), z(64, 31)):
        with pytest.raises(ValueError, match="adaln job 0"):
            ops.adaln_job_table([(z(32, 64), out, z(2, 64), z(2, 64), True)], "cpu")
    s32 = z(4, 64, dt=torch.float32)
    for s_, p_ in ((s32, z(4, 72)), (s32, z(4, 64, dt=torch.float32)), (s32, z(4, 128)[:, ::2]), (z(4, 64), z(4, 64)), (s32, z(4, 64))):
        with pytest.raises(ValueError, match="softmax_rows_f32"):
            ops.softmax_rows_f32(s_, p_)


def test_xattn_epilogue_arguments_are_validated_without_a_gpu():
    """IIR_EPI_XATTN (to_q + cross-attention in one launch): every precondition the header states is refused with -1 before
    any HIP call."""
    h = lib.load()

    def desc():
        d = lib.GemmDesc()
        d.A = d.W = d.C = 4096
        d.lda = d.ldc = 256
        d.M, d.N, d.K = 128, 256, 256
        d.epi = lib.EPI_XATTN
        kv = (lib.AttnKV * 2)()
        for i, t in enumerate((77, 64)):
            kv[i].K = kv[i].Vt = 4096
            kv[i].ldk, kv[i].k_batch_stride, kv[i].ldvt, kv[i].vt_batch_stride, kv[i].Tkv = 256, 256 * t, 160, 80, t
        d.xattn_kv, d.xattn_tq = kv, 64
        return d, kv

    d, kv = desc()
    d.xattn_kv = None
    assert h.iir_gemm_f16(ctypes.byref(d), None) == -1            # no K / V
    for field, bad in (("xattn_tq", 72), ("xattn_tq", 0), ("N", 192), ("M", 96), ("act", lib.ACT_SILU), ("res", 4096), ("dtype", 1),
                       ("tile", 5), ("c_f32", 1)):
        d, kv = desc()
        setattr(d, field, bad)
        assert h.iir_gemm_f16(ctypes.byref(d), None) == -1, field
    for seg, field, bad in ((0, "Tkv", 81), (1, "Tkv", 65), (0, "Tkv", 0), (1, "ldk", 100), (0, "vt_batch_stride", 77), (1, "K", 4100)):
        d, kv = desc()
        setattr(kv[seg], field, bad)
        assert h.iir_gemm_f16(ctypes.byref(d), None) == -1, (seg, field)
    d, kv = desc()
    assert h.iir_gemm_resolve_tile(ctypes.byref(d)) == 93         # the valid descriptor resolves to the head-aligned 64 x 128 tile
