#!/usr/bin/env python3
"""Instruction mix of vfn_mlp16_kernel<MODE> from the unit's device assembly, per wave and per pass of 128 points (the kernel is
straight-line code: one pass = the kernel's instruction stream), and what stands between one tile's last matrix instruction and the
next tile's first (a tile = a run of matrix instructions into the same accumulator registers); and the three phases of a pass that carry
no matrix instruction at all: the prologue (before the first), the longest gap between two (in a fused launch: the encoding of the rendering
net's operand between the vector head and the rendering net's first tile) and the tail (after the last).

    hipcc <csrc/build.sh's flags for vfn_mlp16> --cuda-device-only -S vf_nerf_amd/csrc/vfn_mlp16.hip -o mlp16.s      (no GPU needed)
    python tools/mlp16_instruction_mix.py mlp16.s 3 132                                                             (markdown on stdout)

A mode number names vfn_mlp16_kernel<MODE>; the run-time-geometry twin vfn_mlp16_anyenc_kernel<MODE> is printed beside it when the
assembly holds one.

Counts mnemonics (and compares register operands of one instruction with each other); nothing else is looked for."""
import re
import sys
from collections import Counter
from statistics import median


def kernel_bodies(path):
    lines = open(path).read().split("\n")
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\S*vfn_mlp16_(anyenc_)?kernel\S*:", l)]
    for k, (i, name) in enumerate(starts):
        end = starts[k + 1][0] if k + 1 < len(starts) else len(lines)
        body = []
        for x in lines[i + 1:end]:
            if x.startswith(".Lfunc_end"):
                break
            x = x.split(";")[0].strip()
            if x and not x.startswith(".") and not x.endswith(":"):
                body.append(x)
        yield name, body


def mnemonic(x):
    return re.sub(r"_(e32|e64|dpp|sdwa)$", "", x.split()[0])     # the encoding suffix is not part of the operation


def mix(body):
    c = Counter(mnemonic(x) for x in body)
    mfma = sum(n for op, n in c.items() if op.startswith("v_mfma"))
    valu = sum(n for op, n in c.items() if op.startswith("v_") and not op.startswith("v_mfma"))
    dma = sum(1 for x in body if x.startswith("buffer_load") and x.endswith(" lds"))
    self_max = 0
    for x in body:
        if x.startswith("v_max_f32"):
            ops = [o.strip() for o in x.split(None, 1)[1].split(",")]
            self_max += len(ops) == 3 and ops[1] == ops[2]
    rows = [("matrix (`v_mfma_*`)", mfma), ("other VALU", valu), ("`ds_read_b128`", c["ds_read_b128"]), ("LDS-DMA `buffer_load ... lds`", dma),
            ("`s_waitcnt`", c["s_waitcnt"]), ("`s_nop` instructions", c["s_nop"]),
            ("`s_nop` wait states (cycles)", sum(int(x.split()[1]) + 1 for x in body if x.startswith("s_nop"))), ("`s_barrier`", c["s_barrier"]),
            ("`v_max_f32`", c["v_max_f32"]), ("`v_max_f32 vX, vY, vY` (canonicalising)", self_max), ("`v_max3_f32`", c["v_max3_f32"]),
            ("`v_max_i32`", c["v_max_i32"]), ("`v_max3_i32`", c["v_max3_i32"]), ("`v_med3_f32`", c["v_med3_f32"]),
            ("`v_cmp_le_f32` + `v_cmp_ge_f32`", c["v_cmp_le_f32"] + c["v_cmp_ge_f32"]),
            ("`v_cmp_*_i32`", sum(n for op, n in c.items() if re.match(r"v_cmp_\w+_i32", op))),
            ("`v_writelane_b32`", c["v_writelane_b32"]), ("`v_accvgpr_write_b32`", c["v_accvgpr_write_b32"]),
            ("`v_fma_mix_f32`", c["v_fma_mix_f32"]), ("all instructions", len(body))]
    return rows


def boundaries(body):
    """Per tile boundary: the mnemonics between the last matrix instruction into one accumulator set and the first into the next."""
    gaps, prev_dst, since = [], None, []
    for x in body:
        op = mnemonic(x)
        if op.startswith("v_mfma"):
            dst = x.split(None, 1)[1].split(",")[0].strip()
            if prev_dst is not None and dst != prev_dst:
                gaps.append(list(since))
            prev_dst, since = dst, []
        else:
            since.append(op)
    return gaps


PHASE_OPS = ("v_cndmask_b32", "ds_bpermute_b32", "v_permlane32_swap_b32", "s_cbranch_execz", "s_cbranch_vccnz", "s_cselect_b64", "s_cmp_eq_u32",
             "v_readlane_b32", "v_writelane_b32", "s_or_b64", "v_max_f32", "v_max3_f32", "v_max3_i32", "scratch_load_dwordx4")


def phases(body):
    """(name, mnemonics) of the prologue, the longest stretch between two matrix instructions, and the tail."""
    at = [i for i, x in enumerate(body) if mnemonic(x).startswith("v_mfma")]
    ops = [mnemonic(x) for x in body]
    k = max(range(len(at) - 1), key=lambda i: at[i + 1] - at[i])
    return (("prologue, before the first matrix instruction", ops[:at[0]]),
            (f"longest gap between two matrix instructions (after matrix instruction {k + 1} of {len(at)})", ops[at[k] + 1:at[k + 1]]),
            ("tail, after the last matrix instruction", ops[at[-1] + 1:]))


def main():
    path, modes = sys.argv[1], [int(m) for m in sys.argv[2:]] or [3, 132]
    for name, body in kernel_bodies(path):
        m = re.search(r"vfn_mlp16_(anyenc_)?kernelILi(\d+)E", name)
        if not m or int(m.group(2)) not in modes:
            continue
        print(f"### `vfn_mlp16_{m.group(1) or ''}kernel<{m.group(2)}>`\n\n| class | count |\n|---|---|")
        for label, n in mix(body):
            print(f"| {label} | {n} |")
        gaps = boundaries(body)
        sizes = [len(g) for g in gaps]
        valu = [sum(1 for op in g if op.startswith("v_")) for g in gaps]
        nops = [sum(1 for op in g if op == "s_nop") for g in gaps]
        inside = Counter(op for g in gaps for op in g)
        print(f"\nTile boundaries: {len(gaps)}.  Non-matrix instructions between a tile's last matrix instruction and the next tile's first: "
              f"median {median(sizes):g}, min {min(sizes)}, max {max(sizes)}, total {sum(sizes)}; of them VALU: median {median(valu):g}, "
              f"total {sum(valu)}; `s_nop`: total {sum(nops)}.")
        print("Most frequent there: " + ", ".join(f"`{op}` x {n}" for op, n in inside.most_common(8)) + ".\n")
        whole = Counter(mnemonic(x) for x in body)
        print("| phase | instructions | of them VALU | " + " | ".join(f"`{op}`" for op in PHASE_OPS) + " |\n|---|---|---|" + "---|" * len(PHASE_OPS))
        for label, ops in phases(body) + (("the whole kernel", [mnemonic(x) for x in body]),):
            c = Counter(ops)
            valu = sum(1 for op in ops if op.startswith("v_") and not op.startswith("v_mfma"))
            print(f"| {label} | {len(ops)} | {valu} | " + " | ".join(str(c[op]) for op in PHASE_OPS) + " |")
        print(f"\n`v_writelane_b32` / `v_readlane_b32` in the whole kernel: {whole['v_writelane_b32']} / {whole['v_readlane_b32']}.\n")


if __name__ == "__main__":
    main()
