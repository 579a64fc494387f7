#!/usr/bin/env python3
"""Where do a kernel's full-width integer multiplies sit?  Disassembles code objects (default: minipath_amd/csrc/kernels*.gfx950.co,
make code-objects), finds the natural loops of the kernel whose mangled name contains KERNEL_SUBSTRING (backward branches, as
tools/scratch_in_loops.py does), and prints every 32 x 32 -> 32 / 64 bit multiply (v_mul_lo_u32, v_mul_hi_*32, v_mad_*64_*32: quarter
rate on the vector unit; s_mul_i32, s_mul_hi_*32 on the scalar unit) with the number of loops around it, then the totals per depth.
The pass loop of a packet kernel is taken to be the innermost loop that holds the RNG's seeding (its 16 v_mul_lo_u32); the totals
inside it are printed last (the seeding has 24 vector multiplies, the shading record's address 2).  usage: mul_in_loops.py KERNEL_SUBSTRING [CODE_OBJECT...]"""
import collections
import glob
import os
import re
import subprocess
import sys

MUL = re.compile(r"^(v_mul_lo_u32|v_mul_hi_[iu]32|v_mad_[iu]64_[iu]32|s_mul_i32|s_mul_hi_[iu]32)")


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    cos = sys.argv[2:] or sorted(glob.glob(os.path.join(here, "..", "minipath_amd", "csrc", "kernels*.gfx950.co")))
    txt = "\n".join(subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout for co in cos)
    fn, ins = None, []
    for line in txt.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:", line)
        if m:
            if ins:
                break
            fn = m.group(2) if sys.argv[1] in m.group(2) else None
            continue
        if fn:
            m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
            if m:
                ins.append((int(m.group(3), 16), m.group(1), m.group(2)))
    print(fn, len(ins), "instructions")
    loops = []
    for a, op, args in ins:
        if op.startswith("s_cbranch") or op == "s_branch":
            try:
                off = int(args.split()[0])
            except (ValueError, IndexError):
                continue
            if off >= 32768:
                off -= 65536
            tgt = a + 4 + off * 4
            if tgt <= a:
                loops.append((tgt, a))
    # one loop per header: the backward branches to one target (the loop's latch and its `continue`s) are one loop, up to the last
    ends = collections.defaultdict(int)
    for t, b in loops:
        ends[t] = max(ends[t], b)
    loops = sorted(ends.items())
    per_depth = collections.Counter()
    for a, op, args in ins:
        if MUL.match(op):
            depth = sum(1 for t, b in loops if t <= a <= b)
            per_depth[(depth, op.split("_e")[0])] += 1
            print(f"  {a:#x} {op:20s} loops around: {depth}")
    for (depth, op), n in sorted(per_depth.items()):
        print(f"depth {depth}: {n:3d} {op}")
    # the pass loop: the innermost loop that holds the 16 v_mul_lo_u32 of the RNG's seeding (eight 64-bit products by a constant)
    seeds = [(b - t, t, b) for t, b in loops if sum(1 for a, op, _ in ins if t <= a <= b and op.startswith("v_mul_lo_u32")) >= 16]
    if not seeds:
        print("no loop holds the RNG's seeding")
        return
    _, t, b = min(seeds)
    inside = collections.Counter(op.split("_e")[0] for a, op, _ in ins if t <= a <= b and MUL.match(op))
    print(f"pass loop {t:#x} .. {b:#x}:", ", ".join(f"{n} {op}" for op, n in sorted(inside.items())))
    print("vector multiplies inside the pass loop:", sum(n for op, n in inside.items() if op.startswith("v_")))
    print("scalar multiplies inside the pass loop:", sum(n for op, n in inside.items() if op.startswith("s_")))


if __name__ == "__main__":
    main()
