"""-m "not gpu": the interface of per-sequence token counts in causal softmax decoding: the five _seq entry points (additions to
C ABI 38) are declared and bound with one argument more than their twins and refuse before any launch; the Python surface."""
import ctypes

import pytest
import torch

import efficient_attention as ea
from efficient_attention import _native as nv
from test_cabi import declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
from test_softmax_decode_cpu import BADARG, UNSUPPORTED, _step

TWINS = ["ea_softmax_sdecode_" + n for n in ("append", "attn_split", "merge", "attn_mm", "advance")]


def test_the_seq_entries_are_declared_and_bound_with_ntok(lib):  # noqa: F811
    for name in TWINS:
        assert name + "_seq" in declared_symbols() and hasattr(lib, name + "_seq")
        assert nv.SIGNATURES[name + "_seq"] == nv.SIGNATURES[name][:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert nv.lib().ea_abi_version() == 38


@pytest.mark.parametrize("change,ntok_ok,code", [({}, False, BADARG), (dict(D=48), True, UNSUPPORTED), (dict(T=0), True, BADARG)],
                         ids=["ntok", "D48", "T0"])
def test_the_seq_entries_refuse_before_any_launch(lib, change, ntok_ok, code):  # noqa: F811
    geom, v, p, ws, keep = _step(**change)
    g = ctypes.byref(geom)
    for ntok in [ctypes.c_void_p(keep[0].data_ptr() + 8)] if ntok_ok else [None, ctypes.c_void_p(keep[0].data_ptr() + 2)]:
        assert lib.ea_softmax_sdecode_append_seq(g, p, None, v, v, p, ntok, None) == code
        assert lib.ea_softmax_sdecode_attn_split_seq(g, v, v, v, p, v, 2, ws, ntok, None) == code
        assert lib.ea_softmax_sdecode_merge_seq(g, v, 2, ws, ntok, None) == code
        assert lib.ea_softmax_sdecode_attn_mm_seq(g, v, v, v, p, v, ntok, None) == code
        assert lib.ea_softmax_sdecode_advance_seq(g, ntok, None) == code


def test_the_python_surface_takes_per_sequence():
    from ea_harness.sequence import DecoderStack
    m = ea.CausalSoftmaxAttention(64, 2).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # (accepted: refused for the device, behind it)
        m.init_kv_cache({}, 1, 8, torch.bfloat16, "cpu", per_sequence=True)
    with pytest.raises(TypeError, match="per_sequence must be a bool"):
        m.init_kv_cache({}, 1, 8, torch.bfloat16, "cpu", per_sequence="yes")
    with pytest.raises(TypeError):                                            # keyword-only
        m.init_kv_cache({}, 1, 8, torch.bfloat16, "cpu", 0, False, True)
    soft = DecoderStack(50, 64, 128, 2, 1, attn_name="softmax").eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        soft.init_kv_decoding(1, 8, torch.bfloat16, "cpu", per_sequence=True)
    # a shared-count state (its buffers, on the host: the refusal reads no device) takes all rows or none
    st = {m._incremental_state_id + ".kv_state": {"kv": torch.zeros(2, 2, 2, 4, 32), "pos": torch.zeros(1), "status": torch.zeros(1)}}
    with pytest.raises(NotImplementedError, match=r"per-sequence.*per_sequence=True"):
        m.reset_decoding_rows(st, [1])
