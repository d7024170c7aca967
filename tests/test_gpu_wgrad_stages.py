"""ea_wgrad / ea_wgrad_pair with two token stages of global loads in flight (EA_WGRAD_STAGES=2, the default) at the slice
lengths where the stage pipeline can go wrong -- its first two and its last two stages: slices of 1, 2, 3, 5 (and 4, 6, 7)
stages whose last stage holds 1, 63 or 64 rows (tests/wgrad_stage_cases.py), for [192 x 192], [576 x 192] and the pair
[576 x 192] + [192 x 192], bf16 and fp16, with and without the bias gradient.  Every case must be

  * within the model-relative bound of the same-operand core tests (tests/window_reference.py bound_report, DESIGN 4b:
    a(HIP) <= 4 a(M) + 2^-20 for fp32 results, and the same for max / max and rms / rms) of R = the fp64 product of the same
    16-bit operands, with M = the same product in fp32, and
  * bit-identical to the one-stage loop (EA_WGRAD_STAGES=1).

The library reads the switch once per process, so the two settings run in two child processes, each started fresh under its own
time limit; both run every case once and the tests below only compare."""
import os
import subprocess
import sys

import pytest

import wgrad_stage_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "efficient-attention_amd")
CHILD_LIMIT_S = 300


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """{stages: {case key: [(dW, db | None)]}} from one child process per setting of EA_WGRAD_STAGES."""
    import torch
    td = tmp_path_factory.mktemp("wgrad_stages")
    procs = {}
    for stages in (1, 2):
        out = str(td / ("stages%d.pt" % stages))
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(ROOT, "tests", "wgrad_stage_cases.py"), PKG, out]
        procs[stages] = (out, subprocess.Popen(cmd, env=dict(os.environ, EA_WGRAD_STAGES=str(stages)), stdout=subprocess.PIPE,
                                               stderr=subprocess.STDOUT, text=True))
    res = {}
    logs = {stages: p.communicate()[0] for stages, (_, p) in procs.items()}
    for stages, (out, p) in procs.items():
        assert p.returncode == 0, "EA_WGRAD_STAGES=%d: exit %s\n%s" % (stages, p.returncode, logs[stages][-2000:])
        res[stages] = torch.load(out)
    return res


def test_cases_cover_the_stage_counts_and_fills():
    stages = {(n + 63) // 64 for n in wc.ROWS_PER_SLICE}
    assert {1, 2, 3, 5} <= stages
    for s in (1, 2, 3, 5):
        assert {(n - 1) % 64 + 1 for n in wc.ROWS_PER_SLICE if (n + 63) // 64 == s} >= {1, 63, 64}, s
    assert 1 in wc.ROWS_PER_SLICE and 65 in wc.ROWS_PER_SLICE


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(wc.OPS))
def test_row_counts_give_slices_of_the_wanted_length(op):
    for n in wc.ROWS_PER_SLICE:
        rows, S = wc.rows_for(op, n)
        assert S >= 8 and rows == S * n and wc.slice_query(op)(rows) == S and (rows + S - 1) // S == n, (op, n, rows, S)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", wc.DTYPES)
@pytest.mark.parametrize("op", list(wc.OPS))
def test_two_stages_match_fp64_and_the_one_stage_loop(staged, op, dtype, bias):
    import torch
    import window_reference as wr
    io = torch.bfloat16 if dtype == "bf16" else torch.float16
    lines, bad = [], []
    for n in wc.ROWS_PER_SLICE:
        k = wc.key(op, n, dtype, bias)
        two, one = staged[2][k], staged[1][k]
        for i, (dy, x) in enumerate(wc.operands(op, n, dtype)):
            named = [("dW%d" % i, two[i][0], one[i][0], dy.double().t() @ x.double(), dy.float().t() @ x.float())]
            if bias:
                named.append(("db%d" % i, two[i][1], one[i][1], dy.double().sum(0), dy.float().sum(0)))
            else:
                assert two[i][1] is None and one[i][1] is None
            for name, got, old, R, M in named:
                ok, txt, _ = wr.bound_report(name, got, M.cpu(), R.cpu(), io)
                differ = int((got.view(torch.int32) != old.view(torch.int32)).sum())
                lines.append("%-22s %s  differing from one stage: %d" % (k, txt, differ))
                if not ok or differ:
                    bad.append(lines[-1])
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)
