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


def test_descriptor_layouts_match_header():
    """ctypes mirrors of the structs: natural alignment, sizes as a C compiler lays them out."""
    import shutil
    import subprocess
    import tempfile
    sizes = (ctypes.sizeof(lib.GemmDesc), ctypes.sizeof(lib.ConvDesc), ctypes.sizeof(lib.AttnKV), ctypes.sizeof(lib.AttnDesc),
             ctypes.sizeof(lib.AdaLNJob), ctypes.sizeof(lib.SchedDesc))
    assert all(s % 8 == 0 for s in sizes) and sizes[2] == 56
    if shutil.which("gcc"):      # ask the C compiler itself
        with tempfile.TemporaryDirectory() as td:
            src = os.path.join(td, "sz.c")
            open(src, "w").write('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu", sizeof(iir_gemm_desc),'
                                 'sizeof(iir_conv_desc), sizeof(iir_attn_kv), sizeof(iir_attn_desc), sizeof(iir_adaln_job),'
                                 'sizeof(iir_sched_desc));}' % lib.HEADER_PATH)
            subprocess.run(["gcc", src, "-o", os.path.join(td, "sz")], check=True)
            out = subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout
        assert tuple(int(x) for x in out.split()) == sizes


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
