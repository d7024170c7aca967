#!/usr/bin/env python3
"""Compare one translation unit's gfx950 machine code between two trees, kernel by kernel.

    python tools/isa_diff.py [--new-ok | --by-code] OTHER_TREE [SOURCE.hip]   (default source: ea_ceva_decode.hip; this tree is the other side)

Both sides are compiled with build.py's flags plus `--cuda-device-only -S`.  A kernel's body is what lies between its label
and its `.Lfunc_end`, comments dropped, local `.L*` labels renumbered in order of appearance, its own symbol replaced.
Prints the kernels that exist on one side only and those whose bodies differ; exit status 0 only when there are none.
A kernel whose instructions are equal and whose descriptor (`.amdhsa_*`) alone differs -- a field appended to its parameter
block changes `.amdhsa_kernarg_size` and nothing else -- is listed as such, with the directives that differ, and with
`--new-ok` neither it nor a kernel that only this tree has counts against the exit status.
`--by-code` is for a change that renames kernels: it pairs them by body (instructions and descriptor) whatever their symbols,
prints the symbols left without a partner on either side, and exits 0 only when there are none.
No GPU needed.  A refactor that must not move device speed shows it this way."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(tree, source):
    pkg = os.path.join(tree, "efficient-attention_amd")
    spec = importlib.util.spec_from_file_location("ea_build", os.path.join(pkg, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run([b.HIPCC] + b.FLAGS + [b._cuid(source), "--cuda-device-only", "-S", os.path.join(b.CSRC, source), "-o", out],
                       check=True)
        text = open(out).read()
    found = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index(".Lfunc_end")]
        lines, labels = [], {}
        for line in body.splitlines()[2:]:
            line = line.split(";")[0].strip().replace(name, "KERNEL")
            if line:
                lines.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), line))
        found[name] = lines
    return found


def _split(lines):
    """-> (instructions, descriptor directives)"""
    return [x for x in lines if not x.startswith(".amdhsa_")], [x for x in lines if x.startswith(".amdhsa_")]


def by_code(a, b, source):
    pool = {}
    for k in sorted(b):
        pool.setdefault(tuple(b[k]), []).append(k)
    gone = []
    for k in sorted(a):
        twins = pool.get(tuple(a[k]))
        if twins:
            twins.pop()
        else:
            gone.append(k)
    new = sorted(k for twins in pool.values() for k in twins)
    for k in gone:
        print("other tree only:", k)
    for k in new:
        print("this tree only:", k)
    print("%s: %d / %d kernels, %d paired by code, %d / %d unmatched" % (source, len(a), len(b), len(a) - len(gone), len(gone), len(new)))
    return 1 if gone or new else 0


def main():
    args = [x for x in sys.argv[1:] if x not in ("--new-ok", "--by-code")]
    new_ok = "--new-ok" in sys.argv
    other, source = args[0], (args[1] if len(args) > 1 else "ea_ceva_decode.hip")
    a, b = kernels(other, source), kernels(ROOT, source)
    if "--by-code" in sys.argv:
        return by_code(a, b, source)
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if _split(a[k])[0] != _split(b[k])[0])
    descr = sorted(k for k in set(a) & set(b) if k not in differ and a[k] != b[k])
    for k in gone:
        print("other tree only:", k)
    for k in new:
        print("this tree only:", k)
    for k in differ:
        print("differs (%d / %d instructions): %s" % (len(_split(a[k])[0]), len(_split(b[k])[0]), k))
    for k in descr:
        da, db = _split(a[k])[1], _split(b[k])[1]
        print("same instructions, descriptor differs (%s): %s"
              % ("; ".join("%s -> %s" % (x, y) for x, y in zip(da, db) if x != y) or "directives added or dropped", k))
    print("%s: %d / %d kernels, %d identical, %d identical but for the descriptor"
          % (source, len(a), len(b), len(set(a) & set(b)) - len(differ) - len(descr), len(descr)))
    return 1 if gone or differ or (not new_ok and (new or descr)) else 0


if __name__ == "__main__":
    sys.exit(main())
