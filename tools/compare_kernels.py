#!/usr/bin/env python3
"""Say whether two builds of a translation unit hold the same device code, kernel by kernel.

    hipcc <the product flags> --cuda-device-only -S csrc/train_field.hip -o before/train_field.s     (and again after the change)
    python tools/compare_kernels.py before/train_field.s after/train_field.s
    python tools/compare_kernels.py before/ after/            # every *.s of the two directories, paired by file name

For every kernel (a symbol with an .amdhsa_kernel block) it compares
  * the instruction text from the kernel's label to its descriptor, with comments stripped and the function number taken
    out of local labels (.LBB<n>_<m> -> .LBB_<m>: <n> counts the functions of the file, so it changes when definitions move),
  * the .amdhsa_* directives of its descriptor (registers, LDS, scratch, ...),
and prints SAME or DIFF.  The exit status is non-zero when any kernel differs or the two sides do not hold the same kernels.
It only diffs: what the instructions are is not its business.  ("Moving device code": a refactor of a training
unit that promises unchanged speed shows this tool's output instead of a timing of every kernel.)
"""
from __future__ import annotations

import re
import sys
from pathlib import Path

_LOCAL_LABEL = re.compile(r"(\.L[A-Za-z_]+)\d+_")


def _clean(line: str) -> str:
    line = line.split(";", 1)[0].strip()
    return _LOCAL_LABEL.sub(r"\1_", line)


def kernels(path: Path) -> dict[str, tuple[list[str], list[str]]]:
    """{kernel symbol: (instruction lines, descriptor lines)} of one assembly file."""
    lines = path.read_text().splitlines()
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        desc = next(i for i in range(start, len(lines)) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", lines[i]))
        end = next(i for i in range(desc, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        text = [c for l in lines[start + 1:desc] if (c := _clean(l))]
        hsa = [c for l in lines[desc + 1:end] if (c := _clean(l))]
        out[name] = (text, hsa)
    return out


def compare(a: Path, b: Path) -> bool:
    ka, kb = kernels(a), kernels(b)
    ok = True
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"DIFF  {name}  (only in {b if name in kb else a})")
            ok = False
            continue
        (ta, ha), (tb, hb) = ka[name], kb[name]
        what = [w for w, same in (("instructions", ta == tb), ("descriptor", ha == hb)) if not same]
        if what:
            first = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), min(len(ta), len(tb)))
            print(f"DIFF  {name}  ({', '.join(what)}; {len(ta)} vs {len(tb)} lines, first differing line {first})")
            ok = False
        else:
            print(f"SAME  {name}  ({len(ta)} lines)")
    return ok


def main(argv: list[str]) -> int:
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = Path(argv[1]), Path(argv[2])
    if a.is_dir() != b.is_dir():
        print("give two files or two directories")
        return 2
    if not a.is_dir():
        return 0 if compare(a, b) else 1
    fa, fb = {p.name for p in a.glob("*.s")}, {p.name for p in b.glob("*.s")}
    ok = fa == fb
    for f in sorted(fa ^ fb):
        print(f"DIFF  {f}  (only in {b if f in fb else a})")
    for f in sorted(fa & fb):
        print(f"== {f}")
        ok = compare(a / f, b / f) and ok
    print("all kernels SAME" if ok else "DIFFERENCES found")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
