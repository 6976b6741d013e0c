"""Instruction counts per kernel of a gfx950 assembly listing (DESIGN.md 5.14's tables).

    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -w -S --cuda-device-only instantir_amd/csrc/gemm_conv.hip -o gemm_conv.s
    python tools/isa_count.py gemm_conv.s [substring of the mangled name ...]

Per kernel: instruction lines between its label and its `.Lfunc_end`, those after the last `v_mfma`, and in that part the
`s_cbranch`, `v_exp_f32`, `ds_bpermute_b32`, `v_permlane32_swap`, `s_waitcnt` and `v_fma_mixlo_f16` lines."""
import re
import sys

WHAT = ("s_cbranch", "v_exp_f32", "ds_bpermute_b32", "v_permlane32_swap", "s_waitcnt", "v_fma_mixlo_f16")


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                yield name, body
                name = None
            else:
                s = line.strip()
                if s and not s.startswith((";", ".", "//")) and not s.endswith(":"):
                    body.append(s.split()[0])


def short(name):
    """gemm_kernel<E, BM, BN, ST, CONV, WAVES_M, W8, LW, F8> from the mangled template arguments."""
    m = re.search(r"gemm_kernelI(DF16_|DF16b)Li(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)E", name)
    if not m:
        return name[:60]
    e, bm, bn, st, conv, wm, w8, lw, f8 = m.groups()
    return f"{'bf16' if e == 'DF16b' else 'f16'} {bm}x{bn} st{st}{' lw' if lw == '1' else ''}{' 8w' if wm == '4' else ''}" \
           f"{' w8' if w8 == '1' else ''}{' f8' if f8 == '1' else ''} {'conv' if conv == '1' else 'gemm'}"


if __name__ == "__main__":
    want = sys.argv[2:]
    print("| build | instructions | before the first v_mfma | after the last v_mfma | " + " / ".join(WHAT) + " |")
    print("|---|---|---|---|---|")
    for name, body in kernels(sys.argv[1]):
        if want and not any(w in name or w in short(name) for w in want):
            continue
        mf = [i for i, op in enumerate(body) if op.startswith("v_mfma")]
        first, last = (mf[0], mf[-1]) if mf else (0, -1)
        tail = body[last + 1:]
        print(f"| {short(name)} | {len(body)} | {first} | {len(tail)} | " + " / ".join(str(sum(op.startswith(w) for op in tail)) for w in WHAT) + " |")
