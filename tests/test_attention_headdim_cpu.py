"""CPU: the head-dim 80 / 104 attention entry (`iir_attention_f16`, CLIP ViT-H/14 and bigG/14 vision towers) is exported,
bound, rejects bad arguments before any HIP call, and its kernels use no scratch in the gfx950 code object."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from instantir_amd import lib

ROCM_LLVM = "/opt/rocm/llvm/bin"
NEW_KERNELS = ("attn_hd_kernel",)          # the kernels of csrc/attention_hd.hip


def test_entry_is_exported_and_bound():
    assert "iir_attention_f16" in lib.declared_symbols()
    assert lib.SIGNATURES["iir_attention_f16"] == (ctypes.c_int, [ctypes.POINTER(lib.AttnDesc), ctypes.c_int32, ctypes.c_void_p])
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "iir_attention_f16")


def _valid_desc():
    a = lib.AttnDesc()
    a.Q = a.O = 4096                       # never dereferenced: every case below is refused first
    a.ldq, a.ldo = 2 * 16 * 80, 16 * 80
    a.batch, a.heads, a.Tq, a.nseg, a.scale = 2, 16, 257, 1, 80 ** -0.5
    a.kv[0].K = a.kv[0].Vt = 4096
    a.kv[0].ldk, a.kv[0].ldvt, a.kv[0].vt_batch_stride, a.kv[0].Tkv = 2 * 16 * 80, 2 * 264, 264, 257
    return a


@pytest.mark.parametrize("case", ["hd0", "hd96", "hd128", "nseg3", "nseg0", "fp8", "ldq", "ldo", "ldk", "ldvt", "vbs", "tq", "tkv",
                                  "heads", "batch", "nullq", "nullk"])
def test_invalid_arguments_are_rejected_without_a_gpu(case):
    h = lib.load()
    a, hd = _valid_desc(), 80
    if case.startswith("hd"):
        hd = int(case[2:])
    elif case == "nseg3":
        a.nseg = 3
    elif case == "nseg0":
        a.nseg = 0
    elif case == "fp8":
        a.o_fp8 = 1
    elif case == "ldq":
        a.ldq += 4
    elif case == "ldo":
        a.ldo += 2
    elif case == "ldk":
        a.kv[0].ldk += 4
    elif case == "ldvt":
        a.kv[0].ldvt += 4
    elif case == "vbs":
        a.kv[0].vt_batch_stride += 4
    elif case == "tq":
        a.Tq = 0
    elif case == "tkv":
        a.kv[0].Tkv = 0
    elif case == "heads":
        a.heads = 0
    elif case == "batch":
        a.batch = -1
    elif case == "nullq":
        a.Q = None
    elif case == "nullk":
        a.kv[0].K = None
    assert h.iir_attention_f16(ctypes.byref(a), hd, None) == -1
    if case == "fp8":                      # D = 104 refuses it too
        assert h.iir_attention_f16(ctypes.byref(a), 104, None) == -1


def test_head_dim_64_is_validated_the_same_way():
    h = lib.load()
    a = _valid_desc()
    a.nseg = 3
    assert h.iir_attention_f16(ctypes.byref(a), 64, None) == -1


def _scratch_of_new_kernels(tmp_path):
    """{kernel symbol: private segment bytes} of the attention_hd.hip kernels in the library's gfx950 code objects.  The
    .hip_fatbin section holds one offload bundle per translation unit; clang-offload-bundler reads only the first, so the
    section is split at every bundle magic and each piece is unbundled on its own."""
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
        # the kernel list of the AMDGPU metadata: each kernel's record has `.name:` and `.private_segment_fixed_size:`
        for rec in re.split(r"\n\s*- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", rec)
            priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec)
            if name and priv and any(k in name.group(1) for k in NEW_KERNELS):
                found[name.group(1)] = int(priv.group(1))
    return found


def test_new_kernels_use_no_scratch(tmp_path):
    assert os.path.exists(lib.LIB_PATH)
    found = _scratch_of_new_kernels(tmp_path)
    assert len(found) == 2, f"expected the D = 80 and D = 104 instantiations, found {sorted(found)}"
    assert all(v == 0 for v in found.values()), found
