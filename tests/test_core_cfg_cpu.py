"""-m "not gpu": the EVA / LARA core configurations as records (_ops.EvaCfg, _ops.LaraCfg).

  1. lists() -- the ONE encoder of the int[] / float[] arguments of torch.ops.ea.{eva,lara}_{fwd,bwd} -- writes exactly what the
     callers wrote by hand before the records existed; from_lists() takes every case back, and holds the only reading of the
     optional trailing keep-for-backward entry (absent = keep).
  2. The fake-tensor implementations of the lara / eva / local ops answer every case of tests/core_cfg_fakes.py with the output
     shapes and dtypes recorded from the tree before the records (tests/golden/core_cfg_fakes.json).  Fake CUDA tensors: no GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import core_cfg_fakes as fakes  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "core_cfg_fakes.json")))["cases"]


@pytest.fixture(scope="module")
def ops():
    from efficient_attention import _native, _ops
    if not os.path.exists(os.path.join(ROOT, "efficient-attention_amd", "lib", "libea_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    _native.lib()
    fakes.run(fakes.CASES[-1])          # (the first fake-tensor call of a process pays about a second of one-time set-up)
    return _ops


EVA = [    # (fields, need_grad, icfg, fcfg)
    ((True, (56, 56), 7, 0, 8, 49, "default"), True, [1, 56, 56, 7, 0, 8, 49, 0, 1], [0.5, 1.0]),
    ((True, (56, 56), 7, 0, 8, 49, "default"), False, [1, 56, 56, 7, 0, 8, 49, 0, 0], [0.5, 1.0]),
    ((False, (512,), 16, 16, 8, 64, "no-ln", 2, 1.0, 1.25), True, [0, 512, 0, 16, 16, 8, 64, 2, 1], [1.0, 1.25]),
    ((False, (512,), 16, 16, 8, 64, "default", 1, 1.0, 1.0), False, [0, 512, 0, 16, 16, 8, 64, 1, 0], [1.0, 1.0]),
]
LARA = [
    ((56, 56, 8, True, True, 0, 0, 2.0, 0.125), True, [56, 56, 8, 1, 1, 0, 0, 1], [2.0, 0.125]),
    ((56, 56, 8, True, True, 0, 0, 2.0, 0.125), False, [56, 56, 8, 1, 1, 0, 0, 0], [2.0, 0.125]),
    ((14, 14, 2, False, False, 2, 1, 1.0, 0.125), True, [14, 14, 2, 0, 0, 2, 1, 1], [1.0, 0.125]),
]


def _same_types(a, b):
    return [type(v) for v in a] == [type(v) for v in b]


@pytest.mark.parametrize("fields,need,icfg,fcfg", EVA)
def test_eva_lists_are_the_hand_written_encoding_and_round_trip(ops, fields, need, icfg, fcfg):
    cfg = ops.EvaCfg(*fields)
    got = cfg.lists(need)
    assert got == (icfg, fcfg) and _same_types(got[0], icfg) and _same_types(got[1], fcfg)
    back, back_need = ops.EvaCfg.from_lists(*got, cfg.adaptive_proj)
    assert back == cfg and back_need is need
    assert hash(back) == hash(cfg)
    assert ops.EvaCfg.from_lists(icfg[:8], fcfg, cfg.adaptive_proj) == (cfg, True)          # entry absent: keep for backward
    assert ops.EvaCfg.from_lists(icfg[:8] + [0], fcfg, cfg.adaptive_proj) == (cfg, False)


def test_eva_defaults_are_the_non_causal_core(ops):
    cfg = ops.EvaCfg(True, (56, 56), 7, 0, 8, 49, "default")
    assert (cfg.causal, cfg.mu_scale, cfg.keep_scale) == (0, 0.5, 1.0)
    assert ops.EvaExtras() == (None, None, None) and ops.EvaExtras._fields == ("keep", "table_bias", "pooled")


@pytest.mark.parametrize("fields,need,icfg,fcfg", LARA)
def test_lara_lists_are_the_hand_written_encoding_and_round_trip(ops, fields, need, icfg, fcfg):
    cfg = ops.LaraCfg(*fields)
    got = cfg.lists(need)
    assert got == (icfg, fcfg) and _same_types(got[0], icfg) and _same_types(got[1], fcfg)
    back, back_need = ops.LaraCfg.from_lists(*got)
    assert back == cfg and back_need is need
    assert hash(back) == hash(cfg)
    assert ops.LaraCfg.from_lists(icfg[:7], fcfg) == (cfg, True)
    assert ops.LaraCfg.from_lists(icfg[:7] + [0], fcfg) == (cfg, False)
    assert cfg.L == (cfg.H // cfg.r) * (cfg.W // cfg.r) and cfg.C == cfg.L * (2 if cfg.dup else 1)


def test_golden_file_and_case_list_agree():
    assert sorted(GOLDEN) == sorted(fakes.CASES)


@pytest.mark.parametrize("case", fakes.CASES)
def test_fake_outputs_equal_the_recorded_ones(ops, monkeypatch, case):
    if case.startswith("lara/"):
        monkeypatch.setenv("EA_LARA_COMPOSITE", case.split("/")[2][-1])
    assert fakes.run(case) == GOLDEN[case]
