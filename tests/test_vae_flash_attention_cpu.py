"""CPU: the single-head VAE attention entry (`iir_attention_1h`, csrc/attention_1h.hip) is exported, bound, rejects bad arguments
before any HIP call, its kernels use no scratch in the gfx950 code object, and the switches that reach it exist and default off."""
import ctypes
import os
import re
import subprocess

import pytest

from instantir_amd import lib

ROCM_LLVM = "/opt/rocm/llvm/bin"
NEW_KERNELS = ("attn_1h_kernel",)          # the kernels of csrc/attention_1h.hip
HEAD_DIMS = (128, 256, 512)
SIG = (ctypes.c_int, [ctypes.POINTER(lib.AttnDesc), ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p])


def test_entry_is_exported_and_bound():
    assert "iir_attention_1h" in lib.declared_symbols()
    assert lib.SIGNATURES["iir_attention_1h"] == SIG
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "iir_attention_1h")
    assert lib.load().iir_abi_version() == 3


def _valid_desc(D=512, T=333):
    a = lib.AttnDesc()
    a.Q = a.O = 4096                       # never dereferenced: every case below is refused first
    a.ldq, a.ldo = D, D + 8
    a.q_batch_stride, a.o_batch_stride = T * D, T * (D + 8)
    a.batch, a.heads, a.Tq, a.nseg, a.scale = 2, 1, T, 1, D ** -0.5
    a.kv[0].K = a.kv[0].Vt = 4096
    tp = (T + 7) // 8 * 8
    a.kv[0].ldk, a.kv[0].k_batch_stride, a.kv[0].ldvt, a.kv[0].vt_batch_stride, a.kv[0].Tkv = D, T * D, 2 * tp, tp, T
    return a


CASES = ["heads2", "heads0", "nseg2", "nseg0", "causal", "fp8", "qpre", "dtype2", "dtype-1", "nullq", "nullk", "nullvt", "nullo",
         "ldq", "qbs", "ldo", "obs", "ldk", "kbs", "ldvt", "vbs", "tq", "tkv", "batch0", "batch-1", "nulldesc"]


@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("case", CASES)
def test_invalid_arguments_are_rejected_without_a_gpu(case, D):
    h = lib.load()
    a, dt = _valid_desc(D), 1
    if case == "heads2":
        a.heads = 2
    elif case == "heads0":
        a.heads = 0
    elif case == "nseg2":
        a.nseg = 2
        a.kv[1] = a.kv[0]
    elif case == "nseg0":
        a.nseg = 0
    elif case == "causal":
        a.causal = 1
    elif case == "fp8":
        a.o_fp8 = 1
    elif case == "qpre":
        a.q_prescaled = 1
    elif case.startswith("dtype"):
        dt = int(case[5:])
    elif case == "nullq":
        a.Q = None
    elif case == "nullk":
        a.kv[0].K = None
    elif case == "nullvt":
        a.kv[0].Vt = None
    elif case == "nullo":
        a.O = None
    elif case == "ldq":
        a.ldq += 4
    elif case == "qbs":
        a.q_batch_stride += 4
    elif case == "ldo":
        a.ldo += 4
    elif case == "obs":
        a.o_batch_stride += 4
    elif case == "ldk":
        a.kv[0].ldk += 4
    elif case == "kbs":
        a.kv[0].k_batch_stride += 4
    elif case == "ldvt":
        a.kv[0].ldvt += 4
    elif case == "vbs":
        a.kv[0].vt_batch_stride += 4
    elif case == "tq":
        a.Tq = 0
    elif case == "tkv":
        a.kv[0].Tkv = 0
    elif case == "batch0":
        a.batch = 0
    elif case == "batch-1":
        a.batch = -1
    if case == "nulldesc":
        assert h.iir_attention_1h(None, D, dt, None, None) == -1
    else:
        assert h.iir_attention_1h(ctypes.byref(a), D, dt, None, None) == -1
        if case == "dtype2":                   # both element types are refused alike for a bad descriptor
            assert h.iir_attention_1h(ctypes.byref(a), D, 7, None, None) == -1


@pytest.mark.parametrize("D", [64, 80, 104, 0, 96, 384, 1024])
@pytest.mark.parametrize("dt", [0, 1])
def test_head_dims_without_a_build_are_refused(D, dt):
    assert lib.load().iir_attention_1h(ctypes.byref(_valid_desc(max(D, 8))), D, dt, None, None) == -1


def test_ops_wrapper_and_switches_exist():
    import inspect

    import torch

    from instantir_amd import ops
    from instantir_amd.config import VAEConfig
    from instantir_amd.vae import HipVAE
    assert list(inspect.signature(ops.attention_1h).parameters) == ["q", "o", "k", "vt", "vt_batch_stride", "batch", "Tq", "Tkv",
                                                                    "scale", "bias"]
    assert callable(HipVAE.enable_flash_attention) and callable(HipVAE.disable_flash_attention)
    hv = HipVAE.__new__(HipVAE)                  # (the constructor allocates on the device; the switch itself is host state)
    hv.cfg = VAEConfig.sdxl()
    hv.use_flash_attention = False
    hv.enable_flash_attention()
    assert hv.use_flash_attention is True
    hv.disable_flash_attention()
    assert hv.use_flash_attention is False
    hv.enable_flash_attention(False)
    assert hv.use_flash_attention is False
    src = inspect.getsource(HipVAE.__init__)
    assert "self.use_flash_attention = False" in src
    # the verified size limit (largest activation below 2 GiB): decode T < 65536, encode T < 131072 at the SDXL widths
    hv._check_flash_geometry("decode", 1, 65535)
    hv._check_flash_geometry("decode", 1, 192 * 128)
    hv._check_flash_geometry("encode", 1, 131071)
    for what, R, T in [("decode", 1, 65536), ("decode", 2, 32768), ("encode", 1, 131072), ("encode", 4, 32768)]:
        with pytest.raises(ValueError):
            hv._check_flash_geometry(what, R, T)
    assert torch.bfloat16 in ops._DT and torch.float16 in ops._DT


def test_cli_flag_parses():
    from instantir_amd.infer import apply_vae_flash_attention, build_parser
    bp = build_parser()
    assert bp.parse_args(["--test_path", "x"]).vae_flash_attention is False
    args = bp.parse_args(["--test_path", "x", "--vae_flash_attention"])
    assert args.vae_flash_attention is True

    class _V:
        on = False

        def enable_flash_attention(self):
            self.on = True

    class _P:
        vae = _V()

    p = _P()
    apply_vae_flash_attention(p, bp.parse_args(["--test_path", "x"]))
    assert p.vae.on is False
    apply_vae_flash_attention(p, args)
    assert p.vae.on is True
    p.vae = None
    with pytest.raises(SystemExit):
        apply_vae_flash_attention(p, args)


def _scratch_of_new_kernels(tmp_path):
    """{kernel symbol: private segment bytes} of the attention_1h.hip kernels in the library's gfx950 code objects.  The
    .hip_fatbin section holds one offload bundle per translation unit; clang-offload-bundler reads only the first, so the
    section is split at every bundle magic and each piece is unbundled on its own.  Reads kernel metadata only."""
    tools = {t: os.path.join(ROCM_LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    missing = [t for t, p in tools.items() if not os.path.exists(p)]
    if missing:
        pytest.skip(f"ROCm LLVM tools not found: {missing}")
    fat = tmp_path / "fat.bin"
    subprocess.run([tools["llvm-objcopy"], "--dump-section", f".hip_fatbin={fat}", lib.LIB_PATH, os.devnull], check=True,
                   capture_output=True)
    data = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    assert starts, "no offload bundle in .hip_fatbin"
    found = {}
    for i, s in enumerate(starts):
        piece = tmp_path / f"tu{i}.bundle"
        piece.write_bytes(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = tmp_path / f"tu{i}.co"
        r = subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={piece}", f"--output={co}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True, text=True)
        if r.returncode != 0 or not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([tools["llvm-readelf"], "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for rec in re.split(r"\n\s*- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", rec)
            priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec)
            if name and priv and any(k in name.group(1) for k in NEW_KERNELS):
                found[name.group(1)] = int(priv.group(1))
    return found


def test_new_kernels_use_no_scratch(tmp_path):
    assert os.path.exists(lib.LIB_PATH)
    found = _scratch_of_new_kernels(tmp_path)
    # 3 head dims x 2 element types x 2 workgroup sizes (64 / 32 query rows)
    assert len(found) == 12, f"expected 12 instantiations, found {sorted(found)}"
    for D in HEAD_DIMS:
        assert sum(f"Li{D}E" in k for k in found) == 4, (D, sorted(found))
    assert all(v == 0 for v in found.values()), found
