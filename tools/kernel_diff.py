#!/usr/bin/env python3
"""Compare the device assembly of two builds of one translation unit, symbol by symbol.

    hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only unit.hip -o unit.s    (once per tree; the same path, the same -o)
    python tools/kernel_diff.py old.s new.s

Each function (`name:` ... `.Lfunc_end<n>:`) and its `.amdhsa_kernel name` descriptor (registers, LDS, scratch) are keyed by
symbol and compared after normalising ONLY the function index of the local labels -- .LBB<n>_<m>, .Lfunc_begin<n>,
.Lfunc_end<n>, the "Header=BB<n>_<m>" loop comments that cite them, and the blanks that pad a label line's comment to its
column (their number follows the index's digit count) -- which moves when a function in front disappears.
Exit status 0: no remaining symbol changed and none is new.
"""
import re
import subprocess
import sys

LABEL = re.compile(r"(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end)\d+")
PAD = re.compile(r"^(\.LBBN_\d+:) +;")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")      # hipcc's hash of the unit's path and command line (the -o name included)


def symbols(text):
    names = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([^\s:]+):", line) or re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(PAD.sub(r"\1 ;", LABEL.sub(r"\1N", line)))
            if re.match(r"^(\.Lfunc_end\d+:|\s*\.end_amdhsa_kernel)", line):
                cur = None
    return out


def demangle(names):
    try:
        return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def main(old_path, new_path):
    a, b = open(old_path).read(), open(new_path).read()
    if a == b:
        print("byte-identical")
        return 0
    if CUID.sub("", a) == CUID.sub("", b):
        print("identical apart from the __hip_cuid symbol name (hipcc hashes the path and the command line into it)")
        return 0
    old, new = symbols(a), symbols(b)
    changed = sorted(n for n in old if n in new and old[n] != new[n])
    removed, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print(f"{len(old)} -> {len(new)} functions: {len(set(old) & set(new)) - len(changed)} identical, "
          f"{len(changed)} changed, {len(removed)} removed, {len(added)} new")
    for title, names in (("changed", changed), ("removed", removed), ("new", added)):
        for n in demangle(names):
            print(f"  {title}: {n}")
    return 1 if changed or added else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]) if len(sys.argv) == 3 else __doc__)
