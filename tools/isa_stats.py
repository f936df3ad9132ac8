#!/usr/bin/env python3
"""What hipcc made of a kernel, in numbers: the device assembly of one translation unit of csrc/ (hipcc -S --cuda-device-only with the
unit's build flags), and per kernel the instruction count, matrix instructions, branches (waterfall loops = s_cbranch_execnz), EXEC-masked
blocks (s_and_saveexec), v_readfirstlane, scratch accesses, s_waitcnt by kind, and the wait states (s_nop cycles) by the instruction
before / after them.  Round 5 found its four largest kernel gains this way: run-time storage forms compiled to a
branch per stored register quad, scalar offsets hipcc could not prove uniform compiled to a waterfall loop per store, compare + select
masks through SGPR pairs, divergent blocks in the middle of a pipelined K loop.

    python tools/isa_stats.py vfn_bwd16 [kernel-name substring] [--dump] [--table] [--csrc DIR]        (needs hipcc; no GPU)"""
import hashlib
import os
import re
import subprocess
import sys
from collections import Counter

unit = sys.argv[1] if len(sys.argv) > 1 else "vfn_mlp16"
needle = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].startswith("--") else ""
dump = "--dump" in sys.argv
table = "--table" in sys.argv          # one markdown row per kernel instead: instructions, branches, VGPRs, SGPRs, scratch, histogram digest
root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vf_nerf_amd", "csrc")
if "--csrc" in sys.argv:               # another checkout's csrc/ (to compare two commits)
    root = sys.argv[sys.argv.index("--csrc") + 1]
# the unit's own flags are build.sh's: its extra_flags function (and the MFMA16 it names) is run, not restated here
recipe = open(os.path.join(root, "build.sh")).read()
pieces = [re.search(r"^MFMA16=.*$", recipe, re.M).group(0), re.search(r"^extra_flags\(\) \{.*?^\}", recipe, re.M | re.S).group(0)]
extra = subprocess.run(["bash", "-c", "\n".join(pieces) + '\nextra_flags "$1"', "bash", unit], check=True, capture_output=True, text=True).stdout
flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function"] + extra.split()
asm = f"/tmp/{unit}.isa.s"
subprocess.run(["hipcc", *flags, "--cuda-device-only", "-S", os.path.join(root, unit + ".hip"), "-o", asm], check=True, stderr=subprocess.DEVNULL)
lines = open(asm).read().split("\n")
starts = [(i, l) for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and "kernel" in l]
for k, (i, l) in enumerate(starts):
    if needle not in l:
        continue
    end = starts[k + 1][0] if k + 1 < len(starts) else len(lines)
    body = [x.strip() for x in lines[i:end] if x.startswith("\t") and not x.strip().startswith((";", "."))]
    c = Counter(x.split()[0] for x in body)
    name = re.sub(r"^_Z(N12_GLOBAL__N_1)?\d+", "", l.split(":")[0])[:70]
    mfma = sum(v for kk, v in c.items() if kk.startswith("v_mfma"))
    branches = sum(v for kk, v in c.items() if kk.startswith("s_cbranch"))
    scratch = sum(v for kk, v in c.items() if kk.startswith("scratch_"))
    if table:
        used = {key: int(n) for key, n in re.findall(r"^; (NumVgprs|TotalNumSgprs|ScratchSize): (\d+)", "\n".join(lines[i:end]), re.M)}
        digest = hashlib.sha1(repr(sorted(c.items())).encode()).hexdigest()[:10]
        print(f"| `{name}` | {len(body)} | {branches} | {used['NumVgprs']} | {used['TotalNumSgprs']} | {used['ScratchSize']} | `{digest}` |")
        continue
    print(f"{name}\n    {len(body)} instructions, {mfma} matrix, {branches} branches ({c['s_cbranch_execnz']} execnz = waterfall / divergent loops), "
          f"{c['s_and_saveexec_b64']} saveexec, {c['v_readfirstlane_b32']} readfirstlane, {scratch} scratch accesses")
    waits = Counter(x for x in body if x.startswith("s_waitcnt"))
    print("    s_waitcnt:", ", ".join(f"{w.split(None, 1)[1]} x {n}" for w, n in waits.most_common(6)))
    prev, nxt, total = Counter(), Counter(), 0
    for j, x in enumerate(body):
        if x.startswith("s_nop"):
            n = int(x.split()[1]) + 1
            total += n
            prev[body[j - 1].split()[0]] += n
            if j + 1 < len(body):
                nxt[body[j + 1].split()[0]] += n
    print(f"    wait states: {total} cycles of s_nop; after {prev.most_common(4)}; before {nxt.most_common(4)}")
    print("    most frequent:", ", ".join(f"{op} x {n}" for op, n in c.most_common(14)))
    if dump:
        out = f"/tmp/{unit}.{k}.s"
        open(out, "w").write("\n".join(lines[i:end]))
        print("    assembly:", out)
