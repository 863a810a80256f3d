#!/usr/bin/env python3
"""Did a change of source leave the kernels alone?  Compares every kernel present in both of two gfx950 assembly files
(python st-nerf_amd/build.py --asm SOURCE OUT): the instruction stream from the kernel's label to s_endpgm -- comments and blank
lines dropped, local labels (.LBB.., .Lpost_getpc.., any .L..) renamed by order of first appearance -- and the resource lines
TotalNumSgprs, TotalNumVgprs, ScratchSize, Occupancy, LDSByteSize (a kernel without one of them is an error, not a match), both as
tools/asm_listing.py's kernels() reads them.  One line per kernel; exit status 1 on any difference.

    python tools/isa_same.py OLD.s NEW.s"""
import re
import sys

import asm_listing

RESOURCES = ("TotalNumSgprs", "TotalNumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def kernels(path):
    out = {}
    for name, k in asm_listing.kernels(open(path).read()).items():
        labels = {}
        lines = []
        for line in k["body"].split("\n")[1:]:          # (behind the kernel's own label)
            line = line.split(";", 1)[0].strip()
            if line:
                lines.append(re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), line))
        missing = [r for r in RESOURCES if r not in k]
        if missing:
            sys.exit("%s: no '; %s:' line behind %s" % (path, missing[0], name))
        out[name] = (lines, tuple(str(k[r]) for r in RESOURCES))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    differ = 0
    for name in old:
        if name not in new:
            continue
        (lo, ro), (ln, rn) = old[name], new[name]
        what = []
        if lo != ln:
            at = next((i for i, (a, b) in enumerate(zip(lo, ln)) if a != b), min(len(lo), len(ln)))
            what.append("instructions differ (%d / %d lines, first at line %d)" % (len(lo), len(ln), at + 1))
        what += ["%s %s -> %s" % (k, a, b) for k, a, b in zip(RESOURCES, ro, rn) if a != b]
        differ += bool(what)
        print("%-9s %s  %s" % ("DIFFERENT" if what else "same", name, "; ".join(what) or "%d lines; %s" % (len(lo), " ".join("%s %s" % kv for kv in zip(RESOURCES, ro)))))
    for name in sorted(set(old) ^ set(new)):
        print("%-9s %s" % ("only old" if name in old else "only new", name))
    if not set(old) & set(new):
        sys.exit("no kernel in both files")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
