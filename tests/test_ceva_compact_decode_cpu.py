"""-m "not gpu": `compact_landmarks` of static / rolling incremental decoding (init_*_decoding(compact_landmarks=True): a bf16
or fp16 state keeps rf_k_bar and beta in its own dtype, and its steps run ea_ceva_sdecode_close_l16, _attn_l16 and
_attn_split_l16): the interface, that the option's refusal comes behind those of the plain state and before anything is
allocated, what the state holds, and what the three entry points refuse before any launch (ABI 23).
Its numerics are tests/test_gpu_ceva_compact_decode.py."""
import ctypes
import inspect
import re

import pytest
import torch

import efficient_attention as ea
from test_api_parity import _causal_eva
from test_cabi import _CEVA_REFUSED, HEADER, LIB, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)
from test_ceva_split_decode_cpu import _SPLIT_REFUSED, _no_device

_INITS = ("init_static_decoding", "init_rolling_decoding")
_STATIC_ARGS = ["self", "incremental_state", "batch_size", "max_tokens", "dtype", "device"]
_OTHERS = dict(per_sequence=True, landmark_splits=4, hold_projections=True)


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_compact_landmarks_is_a_keyword_only_option_that_defaults_to_off():
    for which in _INITS:
        extra = ["max_step_tokens"] if "rolling" in which else []
        method = getattr(ea.CausalEVAttention, which)
        assert list(inspect.signature(method).parameters) == _STATIC_ARGS + extra       # the lists the other tests pin
        assert "compact_landmarks" in method.__doc__
        for by_position in ([True, 4, True, True], [True, 1, False, True], [True]):     # behind the other three, or in their place
            with pytest.raises(TypeError):
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", *([None] * len(extra)), *by_position)
        for misspelt in ("compact_landmark", "compact", "compact_landmarks_"):
            with pytest.raises(TypeError):                               # an unknown keyword stays one
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", **{misspelt: True})
        for kw in (dict(compact_landmarks=True), dict(compact_landmarks=False), {}, dict(_OTHERS, compact_landmarks=True)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):   # by keyword: the call goes on to the device check
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                getattr(_causal_eva().eval(), which)(incremental_state={}, batch_size=2, max_tokens=16, dtype=torch.bfloat16,
                                                     device="cpu", **kw)


def test_docstrings_list_the_state_of_a_compact_option():
    for which in _INITS:
        doc = " ".join(getattr(ea.CausalEVAttention, which).__doc__.split())
        assert "compact_landmarks=True" in doc and "rounded" in doc and "_l16" in doc, which
    doc = " ".join(ea.CausalEVAttention.init_static_decoding.__doc__.split())
    for other in ("reorder_incremental_state", "reset_decoding_rows", "decoding_state_nbytes", "refresh_decoding_weights",
                  "decoding_positions"):                                 # each checked, and said so where the tensors are listed
        assert other in doc[doc.index("compact_landmarks=True"):], other


def test_the_refusals_of_the_plain_state_come_first(monkeypatch):
    """The option does not hide what the state refuses anyway: same exception, same message with and without it -- also where
    the option itself would be refused."""
    from efficient_attention import _f32
    cases = [(NotImplementedError, lambda: _causal_eva(self_attention=False).eval(), {}),
             (NotImplementedError, lambda: _causal_eva(attn_args=dict(causal=False)).eval(), {}),
             (NotImplementedError, lambda: _causal_eva().train(), {}),
             (NotImplementedError, lambda: _causal_eva(attn_args=dict(adaptive_proj="default")).eval(), {}),
             (NotImplementedError, lambda: _causal_eva(attn_args=dict(chunk_size=None, num_chunks=4)).eval(), {}),
             (ValueError, lambda: _causal_eva().eval(), dict(dtype=torch.float64)),
             (RuntimeError, lambda: _causal_eva().eval(), dict(device="cpu"))]
    for exc, m_fn, kw in cases:
        msgs = set()
        for which in _INITS:
            for opt in ({}, dict(compact_landmarks=False), dict(compact_landmarks=True), dict(_OTHERS, compact_landmarks=True)):
                args = dict(dict(batch_size=2, max_tokens=16, dtype=torch.bfloat16, device="cpu"), **kw)
                st = {}
                with pytest.raises(exc) as got:
                    getattr(m_fn(), which)(st, **args, **opt)
                assert st == {}
                msgs.add(str(got.value))
        assert len(msgs) == 1 and "compact_landmarks" not in msgs.pop(), (exc, msgs)
    _no_device(monkeypatch, allocate=False)
    for B, T in ((0, 16), (2, 0)):                                       # the sizes, behind the device check
        with pytest.raises(ValueError, match="batch_size > 0 and max_tokens > 0"):
            _causal_eva().eval().init_static_decoding({}, B, T, torch.float32, "cpu", compact_landmarks=True)
    with pytest.raises(ValueError, match="max_step_tokens"):             # a rolling state's own
        _causal_eva().eval().init_rolling_decoding({}, 2, 16, torch.float32, "cpu", max_step_tokens=0, compact_landmarks=True)
    for which in _INITS:                                                 # ... and the other options'
        with pytest.raises(ValueError, match="landmark_splits"):
            getattr(_causal_eva().eval(), which)({}, 2, 16, torch.float32, "cpu", landmark_splits=0, compact_landmarks=True)
        with pytest.raises(ValueError, match="hold_projections"):
            getattr(_causal_eva().eval(), which)({}, 2, 16, torch.float32, "cpu", hold_projections=True, compact_landmarks=True)
    monkeypatch.setattr(_f32, "ENABLED", False)
    with pytest.raises(ValueError, match="fp32 cores"):
        _causal_eva().eval().init_static_decoding({}, 2, 16, torch.float32, "cpu", compact_landmarks=True)


@pytest.mark.parametrize("which", _INITS)
@pytest.mark.parametrize("opt", [{}, dict(per_sequence=True, landmark_splits=4)], ids=["alone", "with_the_others"])
def test_an_fp32_state_has_nothing_to_compact(which, opt, monkeypatch):
    """The option's own refusal: a ValueError that names it and says why, before anything is allocated; without the option
    the same call goes on to the allocation."""
    from efficient_attention import _f32
    monkeypatch.setattr(_f32, "ENABLED", True)
    _no_device(monkeypatch, allocate=False)
    st = {}
    with pytest.raises(ValueError, match="compact_landmarks") as got:
        getattr(_causal_eva().eval(), which)(st, 2, 16, torch.float32, "cpu", compact_landmarks=True, **opt)
    assert st == {} and "fp32" in str(got.value) and "fidelity path" in str(got.value) and "nothing to compact" in str(got.value)
    for kw in ({}, dict(compact_landmarks=False)):
        with pytest.raises(pytest.fail.Exception, match="allocated before refusing"):
            getattr(_causal_eva().eval(), which)({}, 2, 16, torch.float32, "cpu", **kw, **opt)
    with pytest.raises(pytest.fail.Exception, match="allocated before refusing"):          # a 16-bit state: accepted
        getattr(_causal_eva().eval(), which)({}, 2, 16, torch.float16, "cpu", compact_landmarks=True, **opt)


@pytest.mark.parametrize("which", _INITS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("opt", [{}, _OTHERS], ids=["alone", "with_the_others"])
def test_a_compact_state_is_the_plain_state_with_16_bit_landmark_rows(which, dtype, opt, monkeypatch):
    """Off by default; compact_landmarks=False and no option: the same keys, shapes, dtypes, host entries and bytes; True: the
    same keys and shapes, rf_k_bar and beta in the state's dtype and nothing else changed, the bytes less by those of the two
    tensors halved, and the host dict notes the option."""
    m = _causal_eva().eval()
    _no_device(monkeypatch, allocate=True)
    B, h, d, r, w = 3, m.num_heads, m.head_dim, m.chunk_size, m.window_size
    made = {}
    for name, kw in (("none", {}), ("off", dict(compact_landmarks=False)), ("compact", dict(compact_landmarks=True))):
        st = {}
        getattr(m, which)(st, B, 40, dtype, "cpu", **opt, **kw)
        made[name] = (m._get_input_buffer(st), dict(m.get_incremental_state(st, "attn_static")), m.decoding_state_nbytes(st))
    shapes = {n: {k: (tuple(v.shape), v.dtype) for k, v in buf.items() if torch.is_tensor(v)} for n, (buf, _, _) in made.items()}
    assert shapes["none"] == shapes["off"] and set(made["none"][0]) == set(made["off"][0])
    assert made["none"][1] == made["off"][1] and "compact_landmarks" not in made["off"][1]
    assert made["none"][2] == made["off"][2]
    assert made["compact"][1] == dict(made["off"][1], compact_landmarks=True)
    assert set(made["compact"][0]) == set(made["off"][0])
    cap = -(-40 // w) * w
    for k in ("rf_k_bar", "beta"):
        assert shapes["off"].pop(k) == ((B, h, cap // r, d), torch.float32)
        assert shapes["compact"].pop(k) == ((B, h, cap // r, d), dtype)
        assert made["compact"][0][k].data_ptr() % 16 == 0 and made["compact"][0][k].stride(2) % 8 == 0
    assert shapes["compact"] == shapes["off"]
    assert made["off"][2] - made["compact"][2] == 2 * B * h * (cap // r) * d * 2


# ---- C ABI 23: ea_ceva_sdecode_close_l16, _attn_l16, _attn_split_l16 ---------------------------------------------------------
_TWINS = (("ea_ceva_sdecode_close_l16", "ea_ceva_sdecode_close", 9), ("ea_ceva_sdecode_attn_l16", "ea_ceva_sdecode_attn", 10),
          ("ea_ceva_sdecode_attn_split_l16", "ea_ceva_sdecode_attn_split", 12))


def test_abi_23_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() >= 23 and _native.ABI_VERSION == _native.lib().ea_abi_version()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} ea_ceva_sdec_geom;", text).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == ["B", "H", "D", "dtype", "window", "ext", "chunk", "T_new", "cap", "adaptive", "has_bias", "ring", "pos",
                      "status", "ntok"]                                  # unchanged
    assert fields == [n for n, _ in _native.ea_ceva_sdec_geom._fields_]
    for name, twin, nargs in _TWINS:
        decl, tdecl = [re.search(r"int %s\(([^)]*)\);" % n, text).group(1) for n in (name, twin)]
        args, targs = [[" ".join(a.split()) for a in d_.split(",")] for d_ in (decl, tdecl)]
        assert args == targs and len(args) == nargs                      # the twin's signature, name for name
        assert _native.SIGNATURES[name] == _native.SIGNATURES[twin] and len(_native.SIGNATURES[name]) == nargs
        assert hasattr(lib, name) and name in declared_symbols()
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]


_BADARG, _UNSUPPORTED = -1, -2
_F32 = 2
_CLOSE, _ATTN, _SPLIT = "sdecode_close_l16", "sdecode_attn_l16", "sdecode_attn_split_l16"
_ALL = (_CLOSE, _ATTN, _SPLIT)
# (entry point, what is wrong, expected return), in the manner of test_cabi._CEVA_REFUSED.  Only refused calls: an accepted
# one launches.
_L16_REFUSED = (
    # the twins' rows, with the twins' codes and their "which fault decides" order ...
    [(_CLOSE, bad, want) for e, bad, want in _CEVA_REFUSED if e == "sdecode_close"]
    + [(_ATTN, bad, want) for e, bad, want in _CEVA_REFUSED if e == "sdecode_attn"]
    # ... attn_split's are those of attn (test_ceva_split_decode_cpu pins that for the twin) and the split's own: parts, ws,
    # T_new > 8, decided first
    + [(_SPLIT, bad, want) for e, bad, want in _CEVA_REFUSED if e == "sdecode_attn"]
    + [(_SPLIT, {"g": None} if bad is None else bad, want) for e, bad, want in _SPLIT_REFUSED if e == "sdecode_attn_split"]
    # what a compact state adds.  An fp32 geometry: a fault of the dtype, decided where {"dtype": 3} is -- before the head dim
    + [(e, {"dtype": _F32}, _BADARG) for e in _ALL]
    + [(e, {"dtype": _F32, "D": 48}, _BADARG) for e in _ALL]
    + [(e, {"dtype": _F32, "ntok": 32}, _BADARG) for e in _ALL]
    # landmark strides that are no multiple of 8 elements (4 and 68: multiples of 4, which is what an fp32 row needs; 68
    # also holds a row of D = 64)
    + [(e, {t + "." + f: n}, _BADARG) for e in _ALL for t in ("lk", "lv") for f, n in (("sn", 4), ("sn", 68), ("sh", 68), ("sb", 2052))]
    # a landmark pointer that is not 16-byte aligned
    + [(e, {t + ".ptr": off}, _BADARG) for e in _ALL for t in ("lk", "lv") for off in (8, 4, 2)]
    # ... all of them behind the head dim, like the token rows ("D": 48, "q.ptr": 2 of the twins)
    + [(e, dict(bad, D=48), _UNSUPPORTED) for e in _ALL for bad in ({"lk.sn": 68}, {"lv.ptr": 8})]
    # ... and behind what the split adds
    + [(_SPLIT, dict(bad, **first), _BADARG) for bad in ({"dtype": _F32}, {"lv.sn": 4}, {"lk.ptr": 8})
       for first in ({"parts": 1}, {"ws": None}, {"T_new": 9})]
)


def _refused_call(nv, entry, bad):
    """test_cabi._ceva_refused_call and test_ceva_split_decode_cpu._refused_call for the three entry points of a compact
    state: the same valid base (B 2, H 2, D 64, bf16, window 8, ext 8, chunk 4, T_new 2, cap 64, ring 0), the same overrides.
    pos, status, ntok and ws are offsets 0, 16, 32 (or None) and 48 from a 16-byte aligned host address."""
    buf = ctypes.create_string_buffer(96)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    geo = dict(B=2, H=2, D=64, dtype=nv.EA_BF16, window=8, ext=8, chunk=4, T_new=2, adaptive=1, has_bias=1, cap=64, ring=0,
               pos=0, status=16, ntok=None)
    arg = {n: {"ptr": 0, "sb": 2048, "sh": 64, "sn": 128} for n in ("q", "k", "v", "lk", "lv", "out")}
    arg.update(g=1, pad=0, bias=0, mu=[0] * 8, parts=4, ws=48)
    for key, val in bad.items():
        name, _, field = key.partition(".")
        if key in geo:
            geo[key] = val
        elif name == "mu" and field:
            arg["mu"][int(field)] = val
        elif field:
            arg[name][field] = val
        else:
            arg[key] = val

    def p(off):
        return None if off is None else ctypes.c_void_p(base + off)

    def t(name):
        v = arg[name]
        return None if v is None else ctypes.byref(nv.ea_t4(None if v["ptr"] is None else base + v["ptr"], v["sb"], v["sh"], v["sn"]))
    for key in ("pos", "status", "ntok"):
        geo[key] = None if geo[key] is None else base + geo[key]
    g = None if arg["g"] is None else ctypes.byref(nv.ea_ceva_sdec_geom(**geo))
    mu = None if arg["mu"] is None else (ctypes.c_void_p * 8)(*[None if m is None else base + m for m in arg["mu"]])
    fn = getattr(nv.lib(), "ea_ceva_" + entry)
    if entry == _CLOSE:
        return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), mu, t("lk"), t("lv"), None)
    if entry == _ATTN:
        return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), p(arg["bias"]), t("lk"), t("lv"), t("out"), None)
    return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), p(arg["bias"]), t("lk"), t("lv"), t("out"), arg["parts"], p(arg["ws"]), None)


def test_l16_entry_points_refuse_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    for e in ("sdecode_close", "sdecode_attn"):                          # the tables this one is built from hold what it takes
        assert len([1 for x, _, _ in _CEVA_REFUSED if x == e]) >= 35
    assert len([1 for x, bad, _ in _SPLIT_REFUSED if x == "sdecode_attn_split" and bad and set(bad) & {"parts", "ws", "T_new"}]) >= 15
    got = [(entry, bad, want, _refused_call(_native, entry, bad)) for entry, bad, want in _L16_REFUSED]
    wrong = [row for row in got if row[2] != row[3]]
    assert len(got) >= 250 and not wrong, wrong
