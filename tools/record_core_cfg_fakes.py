#!/usr/bin/env python
"""Writes tests/golden/core_cfg_fakes.json: the (shape, dtype) of every output of torch.ops.ea.{lara,eva,local}_{fwd,bwd} under
FakeTensorMode for the cases of tests/core_cfg_fakes.py.  No GPU needed (fake CUDA tensors; the library's host-side plan query).
Run ONCE, on the tree whose fakes are the reference (DESIGN.md 4h names the commit); tests/test_core_cfg_cpu.py holds every later
tree to the file.  Usage: python tools/record_core_cfg_fakes.py <commit the tree is at>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import core_cfg_fakes as cases  # noqa: E402


def main(commit):
    out = {}
    for case in cases.CASES:
        if case.startswith("lara/"):
            os.environ["EA_LARA_COMPOSITE"] = case.split("/")[2][-1]
        out[case] = cases.run(case)
    path = os.path.join(ROOT, "tests", "golden", "core_cfg_fakes.json")
    with open(path, "w") as f:
        json.dump({"recorded_on": commit, "cases": out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(out), path))


if __name__ == "__main__":
    main(sys.argv[1])
