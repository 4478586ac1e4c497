#!/usr/bin/env python3
"""Per-kernel register, scratch and occupancy figures from a hipcc -Rpass-analysis=kernel-resource-usage log, and the
difference between two such logs (a parent build and a new one): which kernels kept their figures, which changed,
which are new. No GPU needed.

    hipcc --offload-arch=gfx950 -O3 ... -Rpass-analysis=kernel-resource-usage ... 2> build.log
    python tools/kernel_resources.py new.log                 # a table of every kernel
    python tools/kernel_resources.py parent.log new.log      # unchanged / changed / new, as markdown
"""
from __future__ import annotations

import re
import subprocess
import sys

FIELDS = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("SGPRs Spill", "SGPR spill"), ("VGPRs Spill", "VGPR spill"),
          ("LDS Size [bytes/block]", "LDS"))


def parse(path: str) -> dict[str, dict[str, str]]:
    kernels: dict[str, dict[str, str]] = {}
    cur = None
    where = r"remark: (?:\S+:\d+:\d+: )?"  # (with debug locations the remark names the kernel's file, line and column first)
    for line in open(path, errors="replace"):
        m = re.search(where + r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(where + r"\s*([A-Za-z /\[\]]+?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return kernels


def demangle(names: list[str]) -> dict[str, str]:
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        out = names
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d)  # the argument list
        short[n] = d.replace("(bool)", "").replace("(int)", "")
    return short


def row(name: str, k: dict[str, str]) -> str:
    return "| `" + name + "` | " + " | ".join(k.get(f, "?") for f, _ in FIELDS) + " |"


def header() -> str:
    return "| kernel | " + " | ".join(h for _, h in FIELDS) + " |\n|---|" + "---|" * len(FIELDS)


def main(argv: list[str]) -> int:
    if len(argv) not in (2, 3):
        print(__doc__)
        return 2
    new = parse(argv[-1])
    names = demangle(sorted(new))
    if len(argv) == 2:
        print(header())
        for n in sorted(new, key=names.get):
            print(row(names[n], new[n]))
        return 0
    old = parse(argv[1])
    same = [n for n in old if n in new and old[n] == new[n]]
    changed = [n for n in old if n in new and old[n] != new[n]]
    gone = [n for n in old if n not in new]
    added = [n for n in new if n not in old]
    print(f"{len(old)} kernels before, {len(new)} after: {len(same)} with identical figures, {len(changed)} changed, "
          f"{len(gone)} gone, {len(added)} new\n")
    if changed:
        old_names = demangle(sorted(old))
        print("Changed (before, after):\n\n" + header())
        for n in changed:
            print(row(old_names[n], old[n]))
            print(row(names[n], new[n]))
        print()
    if gone:
        print("Gone: " + ", ".join(demangle(gone).values()) + "\n")
    if added:
        print("New:\n\n" + header())
    for n in sorted(added, key=names.get):
        print(row(names[n], new[n]))
    return 1 if changed or gone else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
