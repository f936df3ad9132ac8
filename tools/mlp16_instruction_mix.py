#!/usr/bin/env python3
"""Instruction mix of vfn_mlp16_kernel<MODE> from the unit's device assembly, per wave and per pass of 128 points (the kernel is
straight-line code: one pass = the kernel's instruction stream), and what stands between one tile's last matrix instruction and the
next tile's first (a tile = a run of matrix instructions into the same accumulator registers); and the three phases of a pass that carry
no matrix instruction at all: the prologue (before the first), the longest gap between two (in a fused launch: the encoding of the rendering
net's operand between the vector head and the rendering net's first tile) and the tail (after the last).

    hipcc <csrc/build.sh's flags for vfn_mlp16> --cuda-device-only -S vf_nerf_amd/csrc/vfn_mlp16.hip -o mlp16.s      (no GPU needed)
    python tools/mlp16_instruction_mix.py mlp16.s 3 132                                                             (markdown on stdout)
    python tools/mlp16_instruction_mix.py --gaps mlp16.s 3                                       (the issue budget of every gap instead)

A mode number names vfn_mlp16_kernel<MODE>; the run-time-geometry twin vfn_mlp16_anyenc_kernel<MODE> is printed beside it when the
assembly holds one.

--gaps prices what stands between every two consecutive matrix instructions (a GAP) with the issue costs below and sets it against the
24 cycles a 32x32x16 matrix instruction leaves free: per tile the priced cost of every gap, their histogram, the empty gaps, and the
overrun split into gaps that hold an LDS-DMA piece and gaps that hold six or more vector-ALU instructions.  The longest gap (the
exposed encoding boundary of a fused launch, see above) is not a steady-state gap and is left out, as are prologue and tail.

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


# Issue cost in cycles of one instruction standing between two matrix instructions.  Source: MI355X_MICROARCH.md, rows
# "vector-instruction ISSUE cost" (VALU 4, v_cvt_pk_f16_f32 5, transcendental 8, ds_read_b128 4, s_nop n = max(4, n + 1), SALU 1) and
# "LDS-DMA piece ... issue cost" (60; measured there between 25 and 185 depending on what surrounds the piece).  A
# v_mfma_f32_32x32x16 holds issue for 8 of its 32 cycles: GAP_BUDGET = 24 cycles of other issue hide behind it, and a gap runs about
# max(32, 8 + priced cost).  The prices were taken on other kernels: this is a model to place instructions by, not a measurement.
GAP_BUDGET = 24
PRICE_VALU, PRICE_CVT_PK, PRICE_TRANS, PRICE_DS, PRICE_SALU, PRICE_PIECE, PRICE_VMEM = 4, 5, 8, 4, 1, 60, 4
TRANS_OPS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
MANY_VALU = 6           # a gap with this many vector-ALU instructions overruns on them alone
HIST_EDGES = (0, 8, 16, 24, 32, 48, 64, 96)      # histogram classes: 0, 1-8, 9-16, 17-24, 25-32, 33-48, 49-64, 65-96, above


def is_piece(x):
    return x.startswith("buffer_load") and x.endswith(" lds")


def price(x):
    op = mnemonic(x)
    if is_piece(x):
        return PRICE_PIECE
    if op == "s_nop":
        return max(4, int(x.split()[1]) + 1)
    if op.startswith("s_"):
        return PRICE_SALU
    if op.startswith("ds_"):
        return PRICE_DS
    if op.startswith("v_cvt_pk_f16_f32"):
        return PRICE_CVT_PK
    if op.startswith(TRANS_OPS):
        return PRICE_TRANS
    if op.startswith("v_"):
        return PRICE_VALU
    return PRICE_VMEM      # any other vector-memory instruction (buffer / global / scratch)


def gap_budget(body):
    """The gaps between consecutive matrix instructions, tile by tile (a tile = a run of matrix instructions into one accumulator).
    -> list of tiles, each a list of gaps (cost, pieces, valu); the gap that ends a tile belongs to it.  The longest gap is dropped."""
    tiles, since, prev_dst = [[]], None, None
    for x in body:
        if mnemonic(x).startswith("v_mfma"):
            dst = x.split(None, 1)[1].split(",")[0].strip()
            if since is not None:
                ops = [mnemonic(y) for y in since]
                tiles[-1].append((sum(price(y) for y in since), sum(1 for y in since if is_piece(y)),
                                  sum(1 for op in ops if op.startswith("v_")), len(since)))
                if dst != prev_dst:
                    tiles.append([])
            prev_dst, since = dst, []
        elif since is not None:
            since.append(x)
    flat = [(g[3], ti, gi) for ti, t in enumerate(tiles) for gi, g in enumerate(t)]
    if len(flat) > 1:
        _, ti, gi = max(flat)
        del tiles[ti][gi]
    return [t for t in tiles if t]


def print_gaps(tiles):
    gaps = [g for t in tiles for g in t]
    cost = [g[0] for g in gaps]
    over = lambda g: max(0, g[0] - GAP_BUDGET)
    with_piece = [g for g in gaps if g[1]]
    many = [g for g in gaps if not g[1] and g[2] >= MANY_VALU]
    rest = [g for g in gaps if not g[1] and g[2] < MANY_VALU]
    print(f"Steady-state gaps: {len(gaps)}; empty: {sum(1 for g in gaps if g[3] == 0)}; priced cost: total {sum(cost)}, "
          f"mean {sum(cost) / max(1, len(gaps)):.1f} against a budget of {GAP_BUDGET}; priced above {GAP_BUDGET} without a piece: "
          f"{sum(1 for g in gaps if not g[1] and g[0] > GAP_BUDGET)}; pieces that share their gap: {sum(1 for g in with_piece if g[3] > g[1])}.\n")
    print("| priced cost of a gap | gaps |\n|---|---|")
    labels = ["0"] + [f"{a + 1}-{b}" for a, b in zip(HIST_EDGES, HIST_EDGES[1:])] + [f"above {HIST_EDGES[-1]}"]
    counts = [0] * len(labels)
    for c in cost:
        counts[next((i for i, e in enumerate(HIST_EDGES) if c <= e), len(HIST_EDGES))] += 1
    for label, n in zip(labels, counts):
        print(f"| {label} | {n} |")
    print("\n| overrun (priced cost above the budget) | gaps | cycles |\n|---|---|---|")
    own = sum(g[1] * PRICE_PIECE - GAP_BUDGET for g in with_piece)
    print(f"| gap with a piece | {len(with_piece)} | {sum(over(g) for g in with_piece)} |")
    print(f"| ... of it the pieces themselves ({PRICE_PIECE} does not fit into {GAP_BUDGET}) | | {own} |")
    print(f"| ... of it what shares the gap with them | | {sum(over(g) for g in with_piece) - own} |")
    print(f"| gap with >= {MANY_VALU} VALU, no piece | {len(many)} | {sum(over(g) for g in many)} |")
    print(f"| any other gap | {sum(1 for g in rest if over(g))} | {sum(over(g) for g in rest)} |")
    print("\nPer tile, the priced cost of every gap in order (`p`: the gap holds a piece; the last gap of a tile is its boundary):\n")
    for i, t in enumerate(tiles):
        print(f"    tile {i:3d}: " + " ".join(f"{g[0]}{'p' * g[1]}" for g in t))
    print()


def main():
    argv = [a for a in sys.argv[1:] if a != "--gaps"]
    path, modes = argv[0], [int(m) for m in argv[1:]] or [3, 132]
    for name, body in kernel_bodies(path):
        m = re.search(r"vfn_mlp16_(anyenc_)?kernelILi(\d+)E", name)
        if not m or int(m.group(2)) not in modes:
            continue
        if "--gaps" in sys.argv[1:]:
            print(f"### `vfn_mlp16_{m.group(1) or ''}kernel<{m.group(2)}>`: gap budget\n")
            print_gaps(gap_budget(body))
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
