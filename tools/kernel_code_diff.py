#!/usr/bin/env python3
"""Is the machine code of two sets of gfx950 code objects the same, symbol by symbol?

usage: tools/kernel_code_diff.py OLD.co... -- NEW.co...

Disassembles every code object (llvm-objdump -d) and compares the instruction text of every function -- kernels and device functions
alike -- under its mangled name.  A symbol that occurs in several objects of one set (a device function every translation unit
emits for itself) must read the same in all of them.  Two things are not compared, because they depend on where a function sits in
its code object and not on what it does:
  * the immediates of the s_add_u32 / s_addc_u32 that directly follow an s_getpc_b64 and add to its register pair (the distance
    of a pc-relative call or address);
  * padding after a function's last instruction (up to the next function's alignment, or at the end of the code object).
Prints the symbols only one set has and the symbols that differ (with the first differing instruction); exit status 1 if any."""
import os
import re
import shutil
import subprocess
import sys

OBJDUMP = next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")) if p and os.path.exists(p)), None)
PADDING = ("s_code_end", "s_nop 0", "...")  # "...": a run of zero bytes


def functions(path):
    """{symbol: [instruction, ...]} of one code object, position-dependent text taken out"""
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", path], capture_output=True, text=True, check=True).stdout
    out, name = {}, None
    for line in text.split("\n"):
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.startswith("\t"):
            out[name].append(" ".join(line.split("//")[0].split()))  # (the comment holds the address, the bytes and branch targets)
    for body in out.values():
        while body and body[-1] in PADDING:
            body.pop()
        for i, ins in enumerate(body):
            m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]$", ins)
            if not m:
                continue
            # only the two instructions directly after it: the low half into the pair's first register, the carry into its second
            for k, (op, reg) in enumerate((("s_add_u32", "s" + m.group(1)), ("s_addc_u32", "s" + m.group(2))), start=i + 1):
                if k < len(body) and re.match(r"%s %s, %s, \S+$" % (op, reg, reg), body[k]):
                    body[k] = "%s %s, %s, <pc-relative>" % (op, reg, reg)
    return out


def union(paths, label):
    """the functions of a set of code objects; a symbol in several of them has to agree with itself"""
    out, where, clashes = {}, {}, []
    for p in paths:
        for name, body in functions(p).items():
            if name in out and out[name] != body:
                clashes.append("%s: %s differs between %s and %s" % (label, name, where[name], p))
            out.setdefault(name, body)
            where.setdefault(name, p)
    return out, clashes


def main(argv):
    if "--" not in argv or OBJDUMP is None:
        print(__doc__)
        return 2
    old_paths, new_paths = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    old, problems = union(old_paths, "old")
    new, more = union(new_paths, "new")
    problems += more
    problems += ["only in old: " + n for n in sorted(set(old) - set(new))]
    problems += ["only in new: " + n for n in sorted(set(new) - set(old))]
    for n in sorted(set(old) & set(new)):
        a, b = old[n], new[n]
        if a != b:
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            problems.append("differs: %s (%d / %d instructions; at %d: %r / %r)" % (n, len(a), len(b), k, a[k:k + 1], b[k:k + 1]))
    print("\n".join(problems))
    print("%d symbols in old, %d in new, %d in both, %d of them identical" % (len(old), len(new), len(set(old) & set(new)),
                                                                             sum(old[n] == new[n] for n in set(old) & set(new))))
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
