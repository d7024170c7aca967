#!/usr/bin/env python3
"""Compare one translation unit's gfx950 machine code between two trees, kernel by kernel.

    python tools/isa_diff.py OTHER_TREE [SOURCE.hip]          (default source: ea_ceva_decode.hip; this tree is the other side)

Both sides are compiled with build.py's flags plus `--cuda-device-only -S`.  A kernel's body is what lies between its label
and its `.Lfunc_end`, comments dropped, local `.L*` labels renumbered in order of appearance, its own symbol replaced.
Prints the kernels that exist on one side only and those whose bodies differ; exit status 0 only when there are none.
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


def main():
    other, source = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "ea_ceva_decode.hip")
    a, b = kernels(other, source), kernels(ROOT, source)
    only = sorted(set(a) ^ set(b))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for k in only:
        print("one side only:", k)
    for k in differ:
        print("differs (%d / %d instructions): %s" % (len(a[k]), len(b[k]), k))
    print("%s: %d / %d kernels, %d identical" % (source, len(a), len(b), len(set(a) & set(b)) - len(differ)))
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main())
