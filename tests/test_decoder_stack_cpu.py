"""-m "not gpu": the causal-EVA decoder of ea_harness/sequence.py (DecoderLayer, DecoderStack) and the fused few-row linear
behind the feed-forward of its held decoding step (ea_ceva_sdecode_linear_fused, C ABI 24): the interface, the parameter
names, what the entry point refuses before any launch, and the refusals of `init_decoding` / `decode` that need no device.
Numerics: tests/test_gpu_decoder_stack.py.

tests/golden/decoder_layer_keys.json holds names only.  The reference layer lives inside fairseq, which this project neither
ships nor depends on, so the fixture was WRITTEN FROM THE REFERENCE'S SOURCE, not recorded from an instance: "layer" from the members
of fairseq/modules/transformer_layer.py:236-284 that a layer without encoder attention and without the scale_* options has
(self_attn_layer_norm, fc1, fc2, final_layer_norm), "absent" from those it has not, "self_attn" from the parameters
efficient_attention/causal_eva.py:339-395 registers for adaptive_proj 'qk' with the T5 bias, "stack" / "stack_final_norm" from
fairseq's TransformerDecoderBase (embed_tokens tied to the output projection, layers, layer_norm)."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

from test_cabi import HEADER, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_layer_keys.json")
ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)


def _stack(**kw):
    from ea_harness.sequence import DecoderStack
    return DecoderStack(50, 128, 256, 2, 2, ATTN, **kw)


# ---- C ABI 24 -------------------------------------------------------------------------------------------------------------------
def test_abi_24_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() >= 24 and _native.ABI_VERSION == _native.lib().ea_abi_version()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int ea_ceva_sdecode_linear_fused\(([^)]*)\);", text).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["int32_t M", "int32_t K", "int32_t N", "const void* x", "int32_t x_dtype", "int64_t ldx",
                    "const float* ln_gamma", "const float* ln_beta", "float ln_eps", "const void* w", "int32_t w_dtype",
                    "const void* bias", "int32_t act", "const void* res", "int32_t res_dtype", "int64_t ldr", "void* y",
                    "int32_t y_dtype", "int64_t ldy", "void* stream"]
    I, L, P, F = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert _native.SIGNATURES["ea_ceva_sdecode_linear_fused"] == [I, I, I, P, I, L, P, P, F, P, I, P, I, P, I, L, P, I, L, P]
    # (the plain entry point keeps its signature)
    assert _native.SIGNATURES["ea_ceva_sdecode_linear"] == [I, I, I, P, I, L, P, I, P, P, I, L, P]
    assert hasattr(lib, "ea_ceva_sdecode_linear_fused")
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]


_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
_INF, _NAN = float("inf"), float("nan")
# (what is wrong, expected return).  Pointers are offsets from a 16-byte aligned base (or None).  Only refused calls: an
# accepted one launches.  The first block is the table of ea_ceva_sdecode_linear (tests/test_ceva_held_decode_cpu.py).
_FUSED_REFUSED = (
    [({p: off}, _BADARG) for p in ("x", "w", "y") for off in (None, 2, 4, 8, 24)]        # null, or not 16-byte aligned
    + [({"bias": off}, _BADARG) for off in (2, 8, 40)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, -256)]                                   # ldx < K
    + [({"ldy": n}, _BADARG) for n in (767, 0, -768)]                                   # ldy < N
    + [({"ldx": 260}, _BADARG), ({"ldx": 257}, _BADARG), ({"ldx": 258, "x_dtype": _F32}, _BADARG)]
    + [({"ldy": 772}, _BADARG), ({"ldy": 770, "y_dtype": _F32}, _BADARG)]
    + [({"M": n}, _BADARG) for n in (0, -1, -64)]
    + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)] + [({"N": n}, _BADARG) for n in (0, -16)]
    + [({"w_dtype": t, "x_dtype": t, "y_dtype": t, "res_dtype": t}, _BADARG) for t in (_F32, 3, -1)]
    + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _BF16, "y_dtype": _F16}, _BADARG),
       ({"x_dtype": 3}, _BADARG)]
    + [({"w_dtype": _BF16, "y_dtype": _F16}, _BADARG), ({"y_dtype": 3}, _BADARG)]
    + [({"M": n}, _UNSUPPORTED) for n in (65, 128, 1 << 20)]
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]
    + [({"N": n, "ldy": 1024, "ldr": 1024}, _UNSUPPORTED) for n in (8, 24, 776)]
    # the prologue: exactly one of gamma / beta; alignment; eps (read only with LayerNorm on)
    + [({"gamma": None}, _BADARG), ({"beta": None}, _BADARG)]
    + [({p: off}, _BADARG) for p in ("gamma", "beta") for off in (4, 8, 68)]
    + [({"eps": e}, _BADARG) for e in (0.0, -1e-5, _INF, -_INF, _NAN)]
    # the epilogue: the residual's alignment, type and stride; the activation
    + [({"res": off}, _BADARG) for off in (2, 4, 8, 120)]
    + [({"res_dtype": t}, _BADARG) for t in (_F16, 3, -1)]
    + [({"w_dtype": _F16, "x_dtype": _F16, "y_dtype": _F16, "res_dtype": _BF16}, _BADARG)]
    + [({"ldr": n}, _BADARG) for n in (767, 0, -768, 772)] + [({"ldr": 770, "res_dtype": _F32}, _BADARG)]
    + [({"act": a}, _UNSUPPORTED) for a in (2, -1, 7)]
    # x may not be y (res may: not refused, so not in this table)
    + [({"y": 0}, _BADARG), ({"x": 112, "y": 112}, _BADARG)]
    # a bad argument is decided before the geometry and before the activation
    + [(dict(bad, M=65), _BADARG) for bad in ({"x": None}, {"gamma": None}, {"eps": 0.0}, {"res": 8}, {"res_dtype": 3},
                                              {"ldr": 767}, {"y": 0})]
    + [(dict(bad, act=2), _BADARG) for bad in ({"beta": None}, {"eps": _NAN}, {"ldr": 0}, {"y": 0}, {"bias": 2})]
    + [({"M": 65, "act": 2}, _UNSUPPORTED)]
)
# ... and what is NOT read: eps without LayerNorm, res_dtype / ldr without a residual.  These calls get past every check but
# the last one made here (act), which stands in for the launch.
_FUSED_NOT_READ = [{"gamma": None, "beta": None, "eps": e} for e in (0.0, _NAN, -1.0)] \
    + [{"res": None, "res_dtype": 3}, {"res": None, "ldr": 0}, {"res": None, "ldr": 771}]


def _refused_fused(nv, bad):
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    arg = dict(M=8, K=256, N=768, x=0, x_dtype=_BF16, ldx=256, gamma=64, beta=80, eps=1e-5, w=16, w_dtype=_BF16, bias=32,
               act=1, res=96, res_dtype=_BF16, ldr=768, y=48, y_dtype=_BF16, ldy=768)
    arg.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    return nv.lib().ea_ceva_sdecode_linear_fused(
        arg["M"], arg["K"], arg["N"], p(arg["x"]), arg["x_dtype"], arg["ldx"], p(arg["gamma"]), p(arg["beta"]), arg["eps"],
        p(arg["w"]), arg["w_dtype"], p(arg["bias"]), arg["act"], p(arg["res"]), arg["res_dtype"], arg["ldr"], p(arg["y"]),
        arg["y_dtype"], arg["ldy"], None)


def test_fused_linear_entry_point_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _refused_fused(_native, bad)) for bad, want in _FUSED_REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 90 and not wrong, wrong
    unread = [(bad, _refused_fused(_native, dict(bad, act=2))) for bad in _FUSED_NOT_READ]
    assert all(rc == _UNSUPPORTED for _, rc in unread), unread


# ---- the modules ----------------------------------------------------------------------------------------------------------------
def test_decoder_layer_and_stack_parameter_names():
    from ea_harness.sequence import DecoderLayer
    import efficient_attention as ea
    want = json.load(open(GOLDEN))
    layer_keys = sorted(want["layer"] + ["self_attn." + k for k in want["self_attn"]])
    for pre_norm in (True, False):
        layer = DecoderLayer(128, 256, 2, ATTN, normalize_before=pre_norm)
        assert sorted(layer.state_dict()) == layer_keys
        assert type(layer.self_attn) is ea.CausalEVAttention and layer.self_attn.self_attention
        assert not [n for n in want["absent"] if hasattr(layer, n)]
        assert tuple(layer.fc1.weight.shape) == (256, 128) and tuple(layer.fc2.weight.shape) == (128, 256)
    for final_norm in (False, True):
        stack = _stack(final_norm=final_norm)
        keys = want["stack"] + ["layers.%d.%s" % (i, k) for i in range(2) for k in layer_keys]
        assert sorted(stack.state_dict()) == sorted(keys + (want["stack_final_norm"] if final_norm else []))


def test_interface():
    from ea_harness import sequence as sq
    import efficient_attention as ea
    names = lambda f: list(inspect.signature(f).parameters)             # noqa: E731
    assert names(sq.DecoderLayer.__init__) == ["self", "embed_dim", "ffn_dim", "num_heads", "attn_args", "dropout",
                                               "attention_dropout", "activation_dropout", "normalize_before"]
    assert inspect.signature(sq.DecoderLayer.__init__).parameters["normalize_before"].default is True
    assert names(sq.DecoderStack.__init__)[:7] == ["self", "vocab", "embed_dim", "ffn_dim", "num_heads", "layers", "attn_args"]
    assert inspect.signature(sq.DecoderStack.__init__).parameters["final_norm"].default is False
    init = inspect.signature(sq.DecoderStack.init_decoding).parameters
    assert list(init) == ["self", "batch_size", "max_tokens", "dtype", "device", "rolling", "hold_weights", "per_sequence",
                          "landmark_splits", "compact_landmarks", "max_step_tokens"]
    assert [init[k].default for k in list(init)[5:]] == [True, True, False, 1, False, None]
    assert names(sq.DecoderStack.decode) == ["self", "tokens", "state", "key_padding_mask"]
    assert names(sq.DecoderStack.generate)[:5] == ["self", "prompt", "n_new", "state", "graph"]
    for name, args in (("refresh_decoding_weights", ["self", "state"]), ("reorder_decoding_state", ["self", "state", "new_order"]),
                       ("reset_decoding_rows", ["self", "state", "rows"]), ("decoding_state_nbytes", ["self", "state"])):
        assert names(getattr(sq.DecoderStack, name)) == args
    assert names(ea.CausalEVAttention.decoding_positions_tensor) == ["self", "incremental_state"]
    doc = " ".join(sq.DecoderStack.__doc__.split())
    assert "adaptive input and adaptive softmax" in doc and "out of scope" in doc
    m = sq.wikitext103_decoder.__doc__
    assert "1024 / 4096 / 8 heads / 16 layers" in m


def test_wikitext103_decoder_geometry(monkeypatch):
    """(Two layers stand in for sixteen: the builder is patched to count what it is asked for.)"""
    from ea_harness import sequence as sq
    seen = {}

    class Probe:
        def __init__(self, *a, **kw):
            seen["a"], seen["kw"] = a, kw
    monkeypatch.setattr(sq, "DecoderStack", Probe)
    sq.wikitext103_decoder(vocab=77)
    assert seen["a"][:5] == (77, 1024, 4096, 8, 16) and seen["kw"] == dict(normalize_before=True, final_norm=False)
    assert seen["a"][5]["window_size"] == 128 and seen["a"][5]["chunk_size"] == 8 and seen["a"][5]["causal"]


def test_positions_tensor_raises_on_a_dynamic_state():
    stack = _stack().eval()
    attn = stack.layers[0].self_attn
    for what in (attn.decoding_positions_tensor, attn.decoding_positions):
        with pytest.raises(RuntimeError, match="needs a static or rolling decoding state"):
            what({})


def test_init_decoding_refuses_fp32_with_hold_weights():
    stack = _stack().eval()
    for rolling in (True, False):
        with pytest.raises(ValueError, match="holds 16-bit projection weights"):
            stack.init_decoding(2, 16, torch.float32, "cpu", rolling=rolling)          # hold_weights defaults to True
        with pytest.raises(ValueError, match="holds 16-bit projection weights"):
            stack.init_decoding(2, 16, torch.float32, "cpu", rolling=rolling, hold_weights=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                       # a 16-bit one goes on to the device check
        stack.init_decoding(2, 16, torch.bfloat16, "cpu")
    with pytest.raises(ValueError, match="max_positions"):
        stack.init_decoding(2, 5000, torch.bfloat16, "cpu")


def test_decode_and_generate_in_training_mode_raise():
    stack = _stack()
    assert stack.training
    tokens = torch.zeros(1, 2, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="incremental decoding in training mode"):
        stack.decode(tokens, None)
    with pytest.raises(NotImplementedError, match="incremental decoding in training mode"):
        stack.generate(tokens.t(), 4)
    stack.eval()
    assert all(not layer.dropout_module.training for layer in stack.layers)
