"""One LARA and one EVA module step at [2, 14, 14, 192], 3 heads (tests/module_rs192_cases.py), forward + backward, with the
192 -> 192 products on the register-resident kernel (EA_LIN_RS192=1, the default: ea_linear_rs192) and on lin_kernel
(EA_LIN_RS192=0): the output, dx and every parameter gradient must be bit-identical.  The switch is read once per process, so
the two settings run in two fresh child processes, each under its own time limit; the tests below only compare."""
import os
import subprocess
import sys

import pytest

import module_rs192_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "efficient-attention_amd")
CHILD_LIMIT_S = 240


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    """{setting: {attn: results}} from one child process per setting of EA_LIN_RS192."""
    import torch
    td = tmp_path_factory.mktemp("module_rs192")
    procs = {}
    for on in (1, 0):
        out = str(td / ("rs192_%d.pt" % on))
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(ROOT, "tests", "module_rs192_cases.py"), PKG, out]
        procs[on] = (out, subprocess.Popen(cmd, env=dict(os.environ, EA_LIN_RS192=str(on)), stdout=subprocess.PIPE,
                                           stderr=subprocess.STDOUT, text=True))
    logs = {on: p.communicate()[0] for on, (_, p) in procs.items()}
    res = {}
    for on, (out, p) in procs.items():
        assert p.returncode == 0, "EA_LIN_RS192=%d: exit %s\n%s" % (on, p.returncode, logs[on][-2000:])
        res[on] = torch.load(out)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("attn", list(mc.ATTN_ARGS))
def test_module_step_is_bit_identical_with_and_without_the_register_resident_kernel(steps, attn):
    import torch
    new, old = steps[1][attn], steps[0][attn]
    # LARA: the forward's output projection rides the combine pass, only the backward runs the new kernel; EVA: both
    assert new["calls"].count("ea_linear_rs192") == (1 if attn == "lara" else 2), new["calls"]
    assert "ea_linear_w192_prepare_rs" in new["calls"]
    assert "ea_linear_rs192" not in old["calls"] and "ea_linear_w192_prepare_rs" not in old["calls"], old["calls"]
    assert [c for c in new["calls"] if not c.startswith("ea_linear")] == [c for c in old["calls"] if not c.startswith("ea_linear")]
    names = sorted(k for k in new if k != "calls")
    assert names == sorted(k for k in old if k != "calls")
    assert {"y", "dx", "grad.qkv.weight", "grad.proj.weight", "grad.proj.bias"} <= set(names), names
    bad = []
    for k in names:
        a, b = new[k], old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and bool(torch.isfinite(a.float()).all()), k
        if not torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)):
            bad.append("%s: %d elements differ" % (k, int((a != b).sum())))
    assert not bad, "\n".join(bad)
