"""-m "not gpu": `hold_projections` of static / rolling incremental decoding (init_*_decoding(hold_projections=True): the
state holds 16-bit copies of the module's two projections, and a step of at most 64 rows runs them on
ea_ceva_sdecode_linear): the interface, that the option's two refusals come behind those of the plain state and before
anything is allocated, what the state holds, and what the entry point refuses before any launch (ABI 22).
Its numerics are tests/test_gpu_ceva_held_decode.py."""
import ctypes
import inspect
import re

import pytest
import torch

import efficient_attention as ea
from test_api_parity import _causal_eva
from test_cabi import HEADER, LIB, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
from test_ceva_split_decode_cpu import _no_device

_INITS = ("init_static_decoding", "init_rolling_decoding")
_STATIC_ARGS = ["self", "incremental_state", "batch_size", "max_tokens", "dtype", "device"]


def test_hold_projections_is_a_keyword_only_option_that_defaults_to_off():
    for which in _INITS:
        extra = ["max_step_tokens"] if "rolling" in which else []
        method = getattr(ea.CausalEVAttention, which)
        assert list(inspect.signature(method).parameters) == _STATIC_ARGS + extra       # the lists the other tests pin
        assert "hold_projections" in method.__doc__
        for by_position in ([True, 4, True], [True, 1, False], [True]):    # behind the other two, or in their place
            with pytest.raises(TypeError):
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", *([None] * len(extra)), *by_position)
        with pytest.raises(TypeError):                                   # an unknown keyword stays one
            getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", hold_projection=True)
        for kw in (dict(hold_projections=True), dict(hold_projections=False), {},
                   dict(hold_projections=True, per_sequence=True, landmark_splits=4)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):   # by keyword: the call goes on to the device check
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                getattr(_causal_eva().eval(), which)(incremental_state={}, batch_size=2, max_tokens=16, dtype=torch.bfloat16,
                                                     device="cpu", **kw)
    for name, args in (("refresh_decoding_weights", ["self", "incremental_state"]),
                       ("reset_decoding_rows", ["self", "incremental_state", "rows"]),
                       ("decoding_positions", ["self", "incremental_state"]),
                       ("decoding_state_nbytes", ["self", "incremental_state"]),
                       ("static_decoding_overflowed", ["self", "incremental_state"]),
                       ("static_decoding_overflowed_rows", ["self", "incremental_state"])):
        assert list(inspect.signature(getattr(ea.CausalEVAttention, name)).parameters) == args


def test_docstrings_say_that_a_capture_fixes_the_weights():
    for name in _INITS + ("refresh_decoding_weights",):
        doc = " ".join(getattr(ea.CausalEVAttention, name).__doc__.split())
        assert "a capture fixes the weights" in doc.lower(), name
    assert "data_ptr()" in ea.CausalEVAttention.refresh_decoding_weights.__doc__


def test_the_refusals_of_the_plain_state_come_first(monkeypatch):
    """The option does not hide what the state refuses anyway: same exception, same message with and without it -- also where
    the option itself would be refused (an fp32 cache, a module with only some biases)."""
    from efficient_attention import _f32

    def some_biases():
        m = _causal_eva().eval()
        m.k_proj.bias = None
        return m
    cases = [(NotImplementedError, lambda: _causal_eva(self_attention=False).eval(), {}),
             (NotImplementedError, lambda: _causal_eva(attn_args=dict(causal=False)).eval(), {}),
             (NotImplementedError, lambda: _causal_eva().train(), {}),
             (NotImplementedError, lambda: _causal_eva(attn_args=dict(adaptive_proj="default")).eval(), {}),
             (NotImplementedError, lambda: _causal_eva(attn_args=dict(chunk_size=None, num_chunks=4)).eval(), {}),
             (ValueError, lambda: _causal_eva().eval(), dict(dtype=torch.float64)),
             (RuntimeError, lambda: _causal_eva().eval(), dict(device="cpu")),
             (RuntimeError, some_biases, dict(device="cpu"))]
    for exc, m_fn, kw in cases:
        msgs = set()
        for which in _INITS:
            for opt in ({}, dict(hold_projections=False), dict(hold_projections=True),
                        dict(hold_projections=True, per_sequence=True, landmark_splits=4)):
                args = dict(dict(batch_size=2, max_tokens=16, dtype=torch.bfloat16, device="cpu"), **kw)
                st = {}
                with pytest.raises(exc) as got:
                    getattr(m_fn(), which)(st, **args, **opt)
                assert st == {}
                msgs.add(str(got.value))
        assert len(msgs) == 1 and "hold_projections" not in msgs.pop(), (exc, msgs)
    _no_device(monkeypatch, allocate=False)
    for B, T in ((0, 16), (2, 0)):                                       # the sizes, behind the device check
        with pytest.raises(ValueError, match="batch_size > 0 and max_tokens > 0"):
            _causal_eva().eval().init_static_decoding({}, B, T, torch.float32, "cpu", hold_projections=True)
    with pytest.raises(ValueError, match="max_step_tokens"):             # a rolling state's own
        _causal_eva().eval().init_rolling_decoding({}, 2, 16, torch.float32, "cpu", max_step_tokens=0, hold_projections=True)
    for which in _INITS:                                                 # ... and the other option's
        with pytest.raises(ValueError, match="landmark_splits"):
            getattr(_causal_eva().eval(), which)({}, 2, 16, torch.float32, "cpu", landmark_splits=0, hold_projections=True)
    monkeypatch.setattr(_f32, "ENABLED", False)
    with pytest.raises(ValueError, match="fp32 cores"):
        _causal_eva().eval().init_static_decoding({}, 2, 16, torch.float32, "cpu", hold_projections=True)


@pytest.mark.parametrize("which", _INITS)
@pytest.mark.parametrize("opt", [{}, dict(per_sequence=True, landmark_splits=4)], ids=["alone", "with_the_others"])
def test_the_two_refusals_of_the_option_come_before_any_allocation(which, opt, monkeypatch):
    from efficient_attention import _f32
    monkeypatch.setattr(_f32, "ENABLED", True)
    _no_device(monkeypatch, allocate=False)
    st = {}
    with pytest.raises(ValueError, match="hold_projections") as got:
        getattr(_causal_eva().eval(), which)(st, 2, 16, torch.float32, "cpu", hold_projections=True, **opt)
    assert st == {} and "fp32" in str(got.value)
    for gone in ("q_proj", "k_proj", "v_proj"):
        m = _causal_eva().eval()
        getattr(m, gone).bias = None
        with pytest.raises(ValueError, match="hold_projections") as got:
            getattr(m, which)(st, 2, 16, torch.bfloat16, "cpu", hold_projections=True, **opt)
        assert st == {} and "bias" in str(got.value)
        with pytest.raises(pytest.fail.Exception, match="allocated before refusing"):         # without the option: on to the allocation
            getattr(m, which)({}, 2, 16, torch.bfloat16, "cpu", **opt)


@pytest.mark.parametrize("which", _INITS)
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_seq"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
def test_a_held_state_is_the_plain_state_and_its_projections(which, per, bias, monkeypatch):
    """Off by default; hold_projections=False and no option: the same keys, shapes, host entries and bytes; True: the five
    entries, 16-bit, rows of w_qkv in the order q, k, v, the values rounded to nearest even."""
    torch.manual_seed(5)
    m = _causal_eva(bias=bias).eval()
    _no_device(monkeypatch, allocate=True)
    B, C = 3, m.embed_dim
    made = {}
    for name, kw in (("none", {}), ("off", dict(hold_projections=False)), ("held", dict(hold_projections=True))):
        st = {}
        getattr(m, which)(st, B, 40, torch.bfloat16, "cpu", per_sequence=per, **kw)
        made[name] = (m._get_input_buffer(st), dict(m.get_incremental_state(st, "attn_static")), m.decoding_state_nbytes(st), st)
    shapes = {n: {k: (tuple(v.shape), v.dtype) for k, v in buf.items() if torch.is_tensor(v)} for n, (buf, _, _, _) in made.items()}
    assert shapes["none"] == shapes["off"] and set(made["none"][0]) == set(made["off"][0])
    assert made["none"][1] == made["off"][1] and "hold_projections" not in made["off"][1]
    assert made["none"][2] == made["off"][2]
    assert made["held"][1] == dict(made["off"][1], hold_projections=True)
    buf = made["held"][0]
    assert set(buf) == set(made["off"][0]) | {"w_qkv", "b_qkv", "w_out", "b_out", "proj_rows"}
    want = {"w_qkv": (3 * C, C), "w_out": (C, C), "proj_rows": (64, 3 * C)}
    if bias:
        want.update(b_qkv=(3 * C,), b_out=(C,))
    else:
        assert buf["b_qkv"] is None and buf["b_out"] is None
    for k, shape in want.items():
        assert shapes["held"].pop(k) == (shape, torch.bfloat16), k
    assert shapes["held"] == shapes["off"]
    n = 3 * C * C + C * C + 64 * 3 * C + (4 * C if bias else 0)
    assert made["held"][2] == made["off"][2] + 2 * n
    for i, lin in enumerate((m.q_proj, m.k_proj, m.v_proj)):
        assert torch.equal(buf["w_qkv"][i * C:(i + 1) * C], lin.weight.detach().to(torch.bfloat16))
        if bias:
            assert torch.equal(buf["b_qkv"][i * C:(i + 1) * C], lin.bias.detach().to(torch.bfloat16))
    assert torch.equal(buf["w_out"], m.out_proj.weight.detach().to(torch.bfloat16))
    assert not any(t.requires_grad for t in buf.values() if torch.is_tensor(t))
    # refresh_decoding_weights: in place, every pointer kept; a plain state refreshes what it holds and gains nothing
    ptrs = {k: buf[k].data_ptr() for k in want}
    with torch.no_grad():
        m.q_proj.weight.mul_(3.0)
        m.out_proj.weight.add_(1.0)
    assert not torch.equal(buf["w_qkv"][:C], m.q_proj.weight.detach().to(torch.bfloat16))
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("a refresh allocates no state"))
    assert m.refresh_decoding_weights(made["held"][3]) is made["held"][3]
    assert torch.equal(buf["w_qkv"][:C], m.q_proj.weight.detach().to(torch.bfloat16))
    assert torch.equal(buf["w_qkv"][C:2 * C], m.k_proj.weight.detach().to(torch.bfloat16))
    assert torch.equal(buf["w_out"], m.out_proj.weight.detach().to(torch.bfloat16))
    assert {k: buf[k].data_ptr() for k in want} == ptrs
    keys = set(made["off"][0])
    m.refresh_decoding_weights(made["off"][3])
    assert set(made["off"][0]) == keys
    with pytest.raises(RuntimeError, match="needs a static or rolling decoding state"):
        m.refresh_decoding_weights({})


# ---- C ABI 22: ea_ceva_sdecode_linear ---------------------------------------------------------------------------------------
def test_abi_22_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() >= 22 and _native.ABI_VERSION == _native.lib().ea_abi_version()
    raw = open(HEADER).read()
    assert re.search(r"#define\s+EA_CEVA_LINEAR_MAX_ROWS\s+64\b", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.search(r"int ea_ceva_sdecode_linear\(([^)]*)\);", text).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["int32_t M", "int32_t K", "int32_t N", "const void* x", "int32_t x_dtype", "int64_t ldx", "const void* w",
                    "int32_t w_dtype", "const void* bias", "void* y", "int32_t y_dtype", "int64_t ldy", "void* stream"]
    I, L, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _native.SIGNATURES["ea_ceva_sdecode_linear"] == [I, I, I, P, I, L, P, I, P, P, I, L, P]
    assert hasattr(lib, "ea_ceva_sdecode_linear")
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]


_BADARG, _UNSUPPORTED = -1, -2
_BF16, _F16, _F32 = 0, 1, 2
# (what is wrong, expected return).  x, w, bias and y are offsets from a 16-byte aligned base (or None).  Only refused calls:
# an accepted one launches.
_LINEAR_REFUSED = (
    [({p: off}, _BADARG) for p in ("x", "w", "y") for off in (None, 2, 4, 8, 24)]        # null, or not 16-byte aligned
    + [({"bias": off}, _BADARG) for off in (2, 8, 40)]
    + [({"ldx": n}, _BADARG) for n in (255, 0, -256)]                                   # ldx < K
    + [({"ldy": n}, _BADARG) for n in (767, 0, -768)]                                   # ldy < N
    + [({"ldx": 260}, _BADARG), ({"ldx": 257}, _BADARG), ({"ldx": 258, "x_dtype": _F32}, _BADARG)]    # 520, 514, 1032 bytes
    + [({"ldy": 772}, _BADARG), ({"ldy": 770, "y_dtype": _F32}, _BADARG)]               # 1544, 3080 bytes
    + [({"M": n}, _BADARG) for n in (0, -1, -64)]
    + [({"K": n, "ldx": 256}, _BADARG) for n in (0, -32)] + [({"N": n}, _BADARG) for n in (0, -16)]
    + [({"w_dtype": t, "x_dtype": t, "y_dtype": t}, _BADARG) for t in (_F32, 3, -1)]    # not a 16-bit type
    + [({"w_dtype": _BF16, "x_dtype": _F16}, _BADARG), ({"w_dtype": _F16, "x_dtype": _BF16, "y_dtype": _F16}, _BADARG),
       ({"x_dtype": 3}, _BADARG)]                                                       # x neither fp32 nor w's type
    + [({"w_dtype": _BF16, "y_dtype": _F16}, _BADARG), ({"y_dtype": 3}, _BADARG)]       # y neither fp32 nor w's type
    + [({"M": n}, _UNSUPPORTED) for n in (65, 128, 1 << 20)]
    + [({"K": n, "ldx": 1024}, _UNSUPPORTED) for n in (16, 48, 264, 1000)]              # K % 32 (strides stay aligned)
    + [({"N": n, "ldy": 1024}, _UNSUPPORTED) for n in (8, 24, 776)]                     # N % 16
    # a bad argument is decided before the geometry
    + [(dict(bad, M=65), _BADARG) for bad in ({"x": None}, {"w": 8}, {"ldx": 255}, {"ldy": 772}, {"w_dtype": _F32},
                                              {"x_dtype": 3}, {"bias": 2})]
    + [(dict(bad, K=48, ldx=1024), _BADARG) for bad in ({"y": None}, {"M": 0}, {"y_dtype": 3})]
)


def _refused_linear(nv, bad):
    buf = ctypes.create_string_buffer(128)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    arg = dict(M=8, K=256, N=768, x=0, x_dtype=_BF16, ldx=256, w=16, w_dtype=_BF16, bias=32, y=48, y_dtype=_BF16, ldy=768)
    arg.update(bad)

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)
    return nv.lib().ea_ceva_sdecode_linear(arg["M"], arg["K"], arg["N"], p(arg["x"]), arg["x_dtype"], arg["ldx"], p(arg["w"]),
                                           arg["w_dtype"], p(arg["bias"]), p(arg["y"]), arg["y_dtype"], arg["ldy"], None)


def test_linear_entry_point_refuses_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(bad, want, _refused_linear(_native, bad)) for bad, want in _LINEAR_REFUSED]
    wrong = [row for row in got if row[1] != row[2]]
    assert len(got) >= 60 and not wrong, wrong
