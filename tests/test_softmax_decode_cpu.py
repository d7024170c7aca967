"""-m "not gpu": the interface of KV-cache decoding of causal softmax attention (csrc/ea_softmax_decode.hip): the six entry points
(additions to C ABI 38) are declared, bound and exported and refuse before any launch; the planner's rule; the Python surface."""
import ctypes
import inspect

import pytest
import torch

import efficient_attention as ea
from efficient_attention import _native as nv
from test_cabi import declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
from test_causal_softmax_cpu import ATTN

ENTRIES = ["ea_softmax_sdecode_" + n for n in ("append", "attn_split", "merge", "attn_mm", "advance", "parts")]
BADARG, UNSUPPORTED = -1, -2


def test_the_entry_points_are_declared_bound_and_exported(lib):  # noqa: F811
    for name in ENTRIES:
        assert name in declared_symbols() and hasattr(lib, name) and name in nv.SIGNATURES
    assert nv.lib().ea_abi_version() == 38 == nv.ABI_VERSION              # additions only: no signature changed


def _step(D=64, dtype=nv.EA_BF16, T=4, cap=64, B=1, H=2):
    """A step's arguments on host memory: every call below is refused before anything is launched or read."""
    keep = [torch.zeros(64, dtype=torch.int32), torch.zeros(2 * 2 * 64 * 128, dtype=torch.bfloat16),
            torch.zeros(4096, dtype=torch.float32)]
    geom = nv.ea_softmax_sdec_geom(B, H, D, dtype, T, cap, keep[0].data_ptr(), keep[0].data_ptr() + 4)
    view = nv.ea_t4(keep[1].data_ptr(), 2 * 64 * 128, 64 * 128, 128)
    return geom, ctypes.byref(view), ctypes.c_void_p(keep[1].data_ptr()), ctypes.c_void_p(keep[2].data_ptr()), keep + [view]


@pytest.mark.parametrize("change,code", [(dict(D=48), UNSUPPORTED), (dict(dtype=nv.EA_F32), BADARG), (dict(T=0), BADARG),
                                         (dict(cap=0), BADARG), (dict(B=0), BADARG), (dict(H=-1), BADARG)],
                         ids=["D48", "fp32", "T0", "cap0", "B0", "H-1"])
def test_every_entry_refuses_a_bad_geometry(lib, change, code):  # noqa: F811
    geom, v, p, ws, _keep = _step(**change)
    g = ctypes.byref(geom)
    assert lib.ea_softmax_sdecode_append(g, p, None, v, v, p, None) == code
    assert lib.ea_softmax_sdecode_attn_split(g, v, v, v, p, v, 2, ws, None) == code
    assert lib.ea_softmax_sdecode_merge(g, v, 2, ws, None) == code
    assert lib.ea_softmax_sdecode_attn_mm(g, v, v, v, p, v, None) == code
    assert lib.ea_softmax_sdecode_advance(g, None) == code


def test_null_views_parts_and_long_split_steps_are_refused(lib):  # noqa: F811
    geom, v, p, ws, _keep = _step()
    g = ctypes.byref(geom)
    assert lib.ea_softmax_sdecode_append(None, p, None, v, v, p, None) == BADARG
    assert lib.ea_softmax_sdecode_append(g, None, None, v, v, p, None) == BADARG
    assert lib.ea_softmax_sdecode_append(g, p, None, None, v, p, None) == BADARG
    assert lib.ea_softmax_sdecode_append(g, p, None, v, v, None, None) == BADARG
    assert lib.ea_softmax_sdecode_attn_mm(g, v, None, v, p, v, None) == BADARG
    assert lib.ea_softmax_sdecode_attn_mm(g, v, v, v, None, v, None) == BADARG
    assert lib.ea_softmax_sdecode_attn_mm(g, v, v, v, p, None, None) == BADARG
    assert lib.ea_softmax_sdecode_attn_split(g, None, v, v, p, v, 1, None, None) == BADARG
    for parts in (0, 65):
        assert lib.ea_softmax_sdecode_attn_split(g, v, v, v, p, v, parts, ws, None) == BADARG
    assert lib.ea_softmax_sdecode_attn_split(g, v, v, v, p, v, 2, None, None) == BADARG            # parts > 1 needs ws
    assert lib.ea_softmax_sdecode_merge(g, v, 1, ws, None) == BADARG
    assert lib.ea_softmax_sdecode_merge(g, None, 2, ws, None) == BADARG
    long_step, v9, p9, ws9, _keep9 = _step(T=9)
    assert lib.ea_softmax_sdecode_attn_split(ctypes.byref(long_step), v9, v9, v9, p9, v9, 2, ws9, None) == BADARG
    unaligned = nv.ea_softmax_sdec_geom(1, 2, 64, nv.EA_BF16, 4, 64, geom.pos + 2, geom.status)
    assert lib.ea_softmax_sdecode_advance(ctypes.byref(unaligned), None) == BADARG
    assert lib.ea_softmax_sdecode_advance(None, None) == BADARG


# the smallest P with B H P >= 2 cus, clamped to [1, min(64, ceil(cap / 64))], at cus = 256:
#   (1, 8): 512 / 8 = 64 parts wanted; cap 32768 has 512 tiles -> 64; cap 512 has 8 -> 8; cap 100 has 2 -> 2; cap 64 has 1 -> 1
#   (8, 8): 512 / 64 = 8;  (1, 2): 256 wanted -> the ceiling 64;  (3, 7): ceil(512 / 21) = 25;  (64, 16): 1024 >= 512 -> 1
@pytest.mark.parametrize("B,H,cap,want", [(1, 8, 32768, 64), (1, 8, 512, 8), (1, 8, 100, 2), (1, 8, 64, 1), (8, 8, 32768, 8),
                                          (1, 2, 32768, 64), (3, 7, 4096, 25), (64, 16, 4096, 1)])
def test_the_planner_follows_its_rule(lib, B, H, cap, want):  # noqa: F811
    assert lib.ea_softmax_sdecode_parts(B, H, cap, 256) == want
    assert lib.ea_softmax_sdecode_parts(B, H, 0, 256) == BADARG and lib.ea_softmax_sdecode_parts(B, H, cap, -1) == BADARG


def test_the_python_surface():
    from ea_harness.sequence import DecoderStack
    names = lambda f: list(inspect.signature(f).parameters)               # noqa: E731
    assert names(ea.CausalSoftmaxAttention.init_kv_cache) == ["self", "incremental_state", "batch_size", "max_tokens", "dtype",
                                                              "device", "kv_splits", "hold_projections"]
    sig = inspect.signature(DecoderStack.init_kv_decoding)
    assert list(sig.parameters) == ["self", "batch_size", "max_tokens", "dtype", "device", "hold_weights", "kv_splits", "hold_vocab"]
    assert sig.parameters["hold_vocab"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["kv_splits"].default == 0
    for name in ("refresh_decoding_weights", "reorder_incremental_state", "reset_decoding_rows", "decoding_state_nbytes",
                 "static_decoding_overflowed", "decoding_positions", "decoding_positions_tensor", "_check_hold_projections"):
        assert callable(getattr(ea.CausalSoftmaxAttention, name))
    with pytest.raises(NotImplementedError, match="init_decoding"):
        DecoderStack(50, 64, 128, 2, 1, ATTN).init_kv_decoding(1, 8, torch.bfloat16, "cpu")
    soft = DecoderStack(50, 64, 128, 2, 1, attn_name="softmax")
    with pytest.raises(NotImplementedError, match="softmax decoding is not built.*init_kv_decoding"):
        soft.init_decoding(1, 8, None, "cpu")
    m = ea.CausalSoftmaxAttention(64, 2).eval()
    x = torch.zeros(1, 1, 64)
    with pytest.raises(NotImplementedError, match="incremental.*init_kv_cache"):
        m(x, x, x, incremental_state={})
    with pytest.raises(NotImplementedError, match="fp32 decoding"):
        m.init_kv_cache({}, 1, 8, torch.float32, "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.init_kv_cache({}, 1, 8, torch.bfloat16, "cpu")
    with pytest.raises(NotImplementedError, match="training mode"):
        ea.CausalSoftmaxAttention(64, 2).init_kv_cache({}, 1, 8, torch.bfloat16, "cuda")
    with pytest.raises(NotImplementedError, match="head dim 16"):
        ea.CausalSoftmaxAttention(64, 4).eval().init_kv_cache({}, 1, 8, torch.bfloat16, "cuda")
