#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assembly files (hipcc --cuda-device-only -S).

    cmp_asm.py parent.s branch.s [--resources]

Input: the assembly after `c++filt`, with the removed template arguments already dropped from the
demangled names (the sed lines of README.md).  A kernel is its code from its symbol to its
.Lfunc_end label, its .amdhsa_kernel block and its metadata entry; comment lines are dropped, the
function index of the .LBB<fn>_<n> / .Lfunc_end<fn> labels is removed (a kernel that moves in the
object keeps its code but not that index) and __hip_cuid_* becomes a fixed token.  Prints the
kernels only one side has and the kernels that differ; --resources compares only next_free_vgpr,
next_free_sgpr, group_segment_fixed_size, private_segment_fixed_size and accum_offset."""
import re
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset")


def kernels(path):
    lines = [l.rstrip() for l in open(path) if not l.lstrip().startswith(";")]
    lines = [re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", l) for l in lines]
    lines = [re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end)\d+", r".\1", l) for l in lines]
    lines = [re.sub(r"\s*;.*$", "", l) for l in lines]
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel (.+)$", lines[i])
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
            out.setdefault(m.group(1), {})["desc"] = lines[i:j + 1]
            i = j
        i += 1
    for name in out:
        start = lines.index(name + ":")
        end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
        out[name]["code"] = lines[start:end]
    # metadata: one YAML list entry per kernel, from "  - .agpr_count" to the next one
    idx = [k for k, l in enumerate(lines) if l.startswith("  - .agpr_count")]
    stop = next(k for k, l in enumerate(lines) if l.startswith("amdhsa.target"))
    for a, b in zip(idx, idx[1:] + [stop]):
        ent = lines[a:b]
        name = next(l.split(".name:", 1)[1].strip().strip("'") for l in ent if l.lstrip().startswith(".name:"))
        out[name]["meta"] = ent
    return out


def main():
    res = "--resources" in sys.argv
    a, b = (kernels(p) for p in sys.argv[1:3])
    for n in sorted(set(a) - set(b)):
        print("only in parent:", n)
    for n in sorted(set(b) - set(a)):
        print("only in branch:", n)
    same = diff = 0
    for n in sorted(set(a) & set(b)):
        if res:
            pick = lambda k: [l.split()[-1] for r in RES for l in k["desc"] if ".amdhsa_" + r in l]  # noqa: E731
            ok = pick(a[n]) == pick(b[n])
            note = f"{pick(a[n])} -> {pick(b[n])}"
        else:
            ok = a[n] == b[n]
            note = ", ".join(f"{p}: {sum(x != y for x, y in zip(a[n][p], b[n][p])) + abs(len(a[n][p]) - len(b[n][p]))} lines"
                             for p in ("code", "desc", "meta") if a[n][p] != b[n][p])
        same += ok
        diff += not ok
        if not ok:
            print("DIFFERS:", n, note)
    print(f"kernels: parent {len(a)}, branch {len(b)}; compared {same + diff}: {same} identical, {diff} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
