"""-m "not gpu": the causal softmax core's C ABI (ea_softmax_causal_fwd / _bwd / _tiles, additions to ABI 38), its planner rule,
what the entries refuse before any launch (no pointer is dereferenced, no device is needed), and the interfaces around it:
CausalSoftmaxAttention's keys are fairseq's, DecoderLayer / the default DecoderStack are what they were."""
import ctypes
import inspect
import json
import os

import pytest

from test_cabi import declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)

_BADARG = -1
NEW = ("ea_softmax_causal_fwd", "ea_softmax_causal_bwd", "ea_softmax_causal_tiles")
ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)


def test_symbols_are_exported_declared_and_bound(lib):
    from efficient_attention import _native
    for name in NEW:
        assert hasattr(lib, name) and name in declared_symbols() and name in _native.SIGNATURES, name
    assert len(_native.SIGNATURES["ea_softmax_causal_fwd"]) == len(_native.SIGNATURES["ea_softmax_attn_fwd"])
    assert len(_native.SIGNATURES["ea_softmax_causal_bwd"]) == len(_native.SIGNATURES["ea_softmax_attn_bwd"])
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert lib.ea_abi_version() == 38


# (which, B, H, N, D, has_keep) -> tiles at 256 compute units: the largest t allowed with B H (ceil(N / 64 t) + 1) >= 4 * 256
@pytest.mark.parametrize("args,want", [
    ((0, 18, 8, 512, 128, 0), 1), ((0, 18, 8, 512, 64, 0), 1), ((0, 8, 8, 4096, 64, 0), 4), ((0, 8, 8, 4096, 64, 1), 2),
    ((1, 8, 8, 4096, 64, 0), 2), ((1, 8, 8, 4096, 128, 0), 1), ((0, 4, 8, 2048, 128, 0), 1), ((0, 64, 8, 512, 64, 0), 4),
    ((0, 64, 8, 512, 128, 0), 2), ((1, 18, 8, 512, 64, 1), 1)])
def test_planner_rule(lib, args, want):
    assert lib.ea_softmax_causal_tiles(*args, 256) == want


@pytest.mark.parametrize("args", [(2, 1, 1, 64, 64, 0, 256), (0, 0, 1, 64, 64, 0, 256), (0, 1, 1, 0, 64, 0, 256),
                                  (0, 1, 1, 64, 48, 0, 256), (0, 1, 1, 64, 64, 0, -1)])
def test_tiles_refusals(lib, args):
    assert lib.ea_softmax_causal_tiles(*args) == _BADARG


@pytest.mark.parametrize("B,H,N,D,dtype,keep,tiles", [
    (0, 2, 64, 64, 0, None, 0), (2, 0, 64, 64, 0, None, 0), (2, 2, 0, 64, 0, None, 0), (2, 2, 64, 96, 0, None, 0),
    (2, 2, 64, 64, 2, None, 0), (2, 2, 64, 64, 0, None, 3), (2, 2, 64, 64, 0, None, -1), (2, 2, 64, 128, 0, None, 4),
    (2, 2, 64, 64, 0, 1, 4)])
def test_forward_refuses_before_any_launch(lib, B, H, N, D, dtype, keep, tiles):
    """Null views everywhere: a refusal for B / H / N / D / dtype / tiles comes back before anything is read or launched."""
    from efficient_attention import _native as nv
    null = ctypes.byref(nv.ea_t4())
    keep_p = None if keep is None else ctypes.c_void_p(16)           # (only compared with NULL)
    rc = lib.ea_softmax_causal_fwd(B, H, N, D, dtype, ctypes.c_float(0.125), null, null, null, None, null, None, keep_p,
                                   ctypes.c_float(1.0), tiles, None)
    assert rc == _BADARG


def test_module_keys_are_fairseqs():
    import efficient_attention as ea
    m = ea.CausalSoftmaxAttention(64, 2)
    want = {"%s.%s" % (p, w) for p in ("q_proj", "k_proj", "v_proj", "out_proj") for w in ("weight", "bias")}
    assert set(m.state_dict()) == want
    assert list(inspect.signature(m.forward).parameters) == ["query", "key", "value", "key_padding_mask", "incremental_state",
                                                              "need_weights", "attn_mask"]
    assert "CausalSoftmaxAttention" in ea.__all__ and "softmax_causal" not in ea.AttentionFactory.attn_dict


def test_decoder_interfaces_are_unchanged_and_softmax_stack_builds():
    from ea_harness import sequence as sq
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    assert names(sq.DecoderLayer.__init__) == ["self", "embed_dim", "ffn_dim", "num_heads", "attn_args", "dropout",
                                               "attention_dropout", "activation_dropout", "normalize_before"]
    assert names(sq.DecoderStack.__init__)[-1] == "attn_name"
    assert inspect.signature(sq.DecoderStack.__init__).parameters["attn_name"].default == "causal_eva"
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_layer_keys.json")))
    default = sq.DecoderStack(50, 64, 128, 2, 1, ATTN)
    keys = set(default.state_dict())
    assert {"layers.0.self_attn." + k for k in golden["self_attn"]} <= keys
    soft = sq.DecoderStack(50, 64, 128, 2, 1, ATTN, attn_name="softmax")
    attn = {k for k in soft.state_dict() if ".self_attn." in k}
    assert attn == {"layers.0.self_attn.%s.%s" % (p, w) for p in ("q_proj", "k_proj", "v_proj", "out_proj") for w in ("weight", "bias")}
    assert {k for k in keys if ".self_attn." not in k} == set(soft.state_dict()) - attn
    with pytest.raises(NotImplementedError, match="softmax decoding is not built"):
        soft.init_decoding(1, 8, None, "cpu")
    with pytest.raises(ValueError):
        sq.DecoderStack(50, 64, 128, 2, 1, ATTN, attn_name="performer")
