"""-m "not gpu": per-sequence token counts of static / rolling incremental decoding (init_*_decoding(per_sequence=True)):
the interface, that the option refuses what the shared-count state refuses -- message for message, before anything is
allocated -- and what the ea_ceva_sdecode_* entry points refuse once `ntok` is set, before any launch (ABI 20).
Its numerics are tests/test_gpu_ceva_perseq_decode.py."""
import ctypes
import inspect
import re

import pytest
import torch

import efficient_attention as ea
from test_api_parity import _causal_eva
from test_cabi import HEADER, LIB, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)

_INITS = ("init_static_decoding", "init_rolling_decoding")


def _init(m, which, per_sequence, st=None, device="cpu", dtype=torch.bfloat16, B=2, T=16, **kw):
    if per_sequence is not None:
        kw["per_sequence"] = per_sequence
    return getattr(m, which)({} if st is None else st, B, T, dtype, device, **kw)


def _same_refusal(exc, m_fn, **kw):
    """Shared count and per-sequence, static and rolling: one exception type, one message."""
    msgs = []
    for which in _INITS:
        for per in (None, False, True):
            st = {}
            with pytest.raises(exc) as got:
                _init(m_fn(), which, per, st=st, **kw)
            assert st == {}
            msgs.append((type(got.value), str(got.value)))
    assert len(set(msgs)) == 1, msgs
    return msgs[0][1]


def test_per_sequence_is_a_keyword_only_option_that_defaults_to_off():
    """By behaviour: the positional parameter lists of the two methods are pinned as they were by the tests of the static
    and the rolling state, so the option is not among them; it is accepted by keyword, refused by position, and off by
    default (test_gpu_ceva_perseq_decode.py: a state made without it is the shared-count state)."""
    for which in _INITS:
        extra = [None] if "rolling" in which else []
        assert "per_sequence" in getattr(ea.CausalEVAttention, which).__doc__
        with pytest.raises(TypeError):                                   # not accepted by position
            getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", *extra, True)
        with pytest.raises(TypeError):                                   # nor is any other keyword
            getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", per_row=True)
        for per in (False, True):                                        # by keyword: accepted, the call goes on to the device check
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", per_sequence=per)
            with pytest.raises(RuntimeError, match="no CPU fallback"):   # ... and every other argument by keyword still binds
                getattr(_causal_eva().eval(), which)(incremental_state={}, batch_size=2, max_tokens=16, dtype=torch.bfloat16,
                                                     device="cpu", per_sequence=per)
    for name, args in (("reset_decoding_rows", ["self", "incremental_state", "rows"]),
                       ("decoding_positions", ["self", "incremental_state"]),
                       ("static_decoding_overflowed", ["self", "incremental_state"]),
                       ("static_decoding_overflowed_rows", ["self", "incremental_state"])):
        assert list(inspect.signature(getattr(ea.CausalEVAttention, name)).parameters) == args
    for name in ("decoding_positions", "static_decoding_overflowed", "static_decoding_overflowed_rows"):
        assert "back" in getattr(ea.CausalEVAttention, name).__doc__    # they read device memory back, and say so


@pytest.mark.parametrize("case", ["encoder_decoder", "not_causal", "training", "adaptive_default"])
def test_per_sequence_refuses_what_the_shared_count_refuses(case):
    m_fn = {"encoder_decoder": lambda: _causal_eva(self_attention=False).eval(),
            "not_causal": lambda: _causal_eva(attn_args=dict(causal=False)).eval(),
            "training": lambda: _causal_eva().train(),
            "adaptive_default": lambda: _causal_eva(attn_args=dict(adaptive_proj="default")).eval()}[case]
    msg = _same_refusal(NotImplementedError, m_fn)
    assert "incremental decoding" in msg or "adaptive projection" in msg


def test_per_sequence_needs_a_chunk_size():
    assert "needs --chunk-size" in _same_refusal(
        NotImplementedError, lambda: _causal_eva(attn_args=dict(chunk_size=None, num_chunks=4)).eval())


@pytest.mark.parametrize("device", ["cpu", torch.device("cpu")], ids=["str", "device"])
def test_per_sequence_has_no_cpu_fallback(device):
    assert "no CPU fallback" in _same_refusal(RuntimeError, lambda: _causal_eva().eval(), device=device)


def test_per_sequence_cache_dtypes(monkeypatch):
    from efficient_attention import _f32
    assert "bf16, fp16 or fp32" in _same_refusal(ValueError, lambda: _causal_eva().eval(), dtype=torch.float64)
    monkeypatch.setattr(_f32, "ENABLED", False)
    assert "fp32 cores" in _same_refusal(ValueError, lambda: _causal_eva().eval(), dtype=torch.float32)


@pytest.mark.parametrize("B,T", [(0, 16), (2, 0)])
def test_per_sequence_sizes(B, T, monkeypatch):
    """(The size check comes after the device check, which is stubbed so that it is reached without a GPU.)"""
    from efficient_attention import _native
    monkeypatch.setattr(_native, "require_cuda", lambda *a, **k: None)
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("allocated before refusing"))
    assert "batch_size > 0 and max_tokens > 0" in _same_refusal(ValueError, lambda: _causal_eva().eval(), B=B, T=T)


@pytest.mark.parametrize("S", [0, -5])
def test_per_sequence_rolling_refuses_a_non_positive_step_bound(S, monkeypatch):
    from efficient_attention import _native
    monkeypatch.setattr(_native, "require_cuda", lambda *a, **k: None)
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("allocated before refusing"))
    msgs = []
    for per in (False, True):
        st = {}
        with pytest.raises(ValueError, match="max_step_tokens") as got:
            _init(_causal_eva().eval(), "init_rolling_decoding", per, st=st, max_step_tokens=S)
        assert st == {}
        msgs.append(str(got.value))
    assert msgs[0] == msgs[1]


@pytest.mark.parametrize("state", [None, {}], ids=["none", "empty"])
def test_row_helpers_need_a_static_state(state):
    m = _causal_eva().eval()
    m.init_incremental_state()
    for call in (lambda: m.reset_decoding_rows(state, [0]), lambda: m.decoding_positions(state),
                 lambda: m.static_decoding_overflowed_rows(state)):
        with pytest.raises(RuntimeError, match="needs a static or rolling decoding state"):
            call()


# ---- C ABI 20: ea_ceva_sdec_geom.ntok ------------------------------------------------------------------------------------
def test_abi_20_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() >= 20 and _native.ABI_VERSION == _native.lib().ea_abi_version()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} ea_ceva_sdec_geom;", text).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [n for n, _ in _native.ea_ceva_sdec_geom._fields_]
    assert fields[-3:] == ["pos", "status", "ntok"]                      # appended: the fields before it keep their offsets
    assert _native.ea_ceva_sdec_geom.ntok.offset == _native.ea_ceva_sdec_geom.status.offset + 8
    assert _native.ea_ceva_sdec_geom().ntok is None                      # ctypes zero-initialises: old callers pass NULL
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]


_BADARG = -1
_STATIC = ("sdecode_close", "sdecode_attn")
# (entry point, what is wrong, expected return), in the manner of test_cabi._CEVA_REFUSED.  ntok is an offset from the
# 16-byte aligned base like pos (0) and status (16); a valid one would be 32.  Only refused calls: an accepted one launches.
_NTOK_REFUSED = (
    [(e, {"ntok": 34}, _BADARG) for e in _STATIC + ("sdecode_append", "sdecode_advance")]                 # misaligned
    + [(e, {"ntok": 33}, _BADARG) for e in _STATIC + ("sdecode_append", "sdecode_advance")]
    + [(e, {"ntok": 32, "pos": None}, _BADARG) for e in _STATIC + ("sdecode_append", "sdecode_advance")]
    + [(e, {"ntok": 32, "status": None}, _BADARG) for e in _STATIC + ("sdecode_append",)]
    + [(e, {"ntok": 32, "pos": 2}, _BADARG) for e in _STATIC + ("sdecode_append", "sdecode_advance")]
    + [(e, {"ntok": 32, "pad": None}, _BADARG) for e in _STATIC + ("sdecode_append",)]
    # where it meets D = 48: a static-state fault is decided before the head dim, so BADARG, not UNSUPPORTED
    + [(e, {"D": 48, "ntok": 34}, _BADARG) for e in _STATIC + ("sdecode_append",)]
    + [(e, {"D": 48, "ntok": 32, "pos": None}, _BADARG) for e in _STATIC + ("sdecode_append",)]
    + [(e, {"D": 48, "ntok": 32, "status": None}, _BADARG) for e in _STATIC + ("sdecode_append",)]
    + [(e, {"D": 48, "ntok": 32, "cap": 60}, _BADARG) for e in _STATIC]
    + [(e, {"D": 48, "ntok": 32, "ring": 16}, _BADARG) for e in _STATIC + ("sdecode_append",)]
    # ... and an aligned ntok does not hide the head dim, nor any other fault of the shared-count table
    + [(e, {"D": 48, "ntok": 32}, -2) for e in _STATIC + ("sdecode_append",)]
    + [(e, dict(bad, ntok=32), _BADARG) for e in _STATIC for bad in (
        {"B": 0}, {"T_new": 0}, {"chunk": 3}, {"ring": 20}, {"q": None}, {"lv.sn": 2}, {"dtype": 3})]
    + [("sdecode_attn", {"ntok": 32, "out": None}, _BADARG), ("sdecode_close", {"ntok": 32, "mu": None}, _BADARG),
       ("sdecode_append", {"ntok": 32, "qkv": 4}, _BADARG), ("sdecode_advance", {"ntok": 32, "T_new": 0}, _BADARG),
       ("sdecode_advance", {"ntok": 32, "B": 0}, _BADARG)]
)


def _refused_call(nv, entry, bad):
    """test_cabi._ceva_refused_call for the static family, with the geometry's `ntok`."""
    buf = ctypes.create_string_buffer(96)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    geo = dict(B=2, H=2, D=64, dtype=nv.EA_BF16, window=8, ext=8, chunk=4, T_new=2, adaptive=1, has_bias=1, cap=64, ring=0,
               pos=0, status=16, ntok=None)
    arg = {n: {"ptr": 0, "sb": 2048, "sh": 64, "sn": 128} for n in ("q", "k", "v", "lk", "lv", "out")}
    arg.update(pad=0, bias=0, qkv_new=0, qkv=0, mu=[0] * 8)
    for key, val in bad.items():
        name, _, field = key.partition(".")
        if key in geo:
            geo[key] = val
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
    g = ctypes.byref(nv.ea_ceva_sdec_geom(**geo))
    mu = None if arg["mu"] is None else (ctypes.c_void_p * 8)(*[base + m for m in arg["mu"]])
    fn = getattr(nv.lib(), "ea_ceva_" + entry)
    if entry.endswith("close"):
        return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), mu, t("lk"), t("lv"), None)
    if entry.endswith("attn"):
        return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), p(arg["bias"]), t("lk"), t("lv"), t("out"), None)
    if entry.endswith("append"):
        return fn(g, p(arg["qkv_new"]), None, p(arg["qkv"]), p(arg["pad"]), None)
    return fn(g, None)


def test_sdecode_entry_points_refuse_a_bad_ntok_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(entry, bad, want, _refused_call(_native, entry, bad)) for entry, bad, want in _NTOK_REFUSED]
    wrong = [row for row in got if row[2] != row[3]]
    assert len(got) >= 50 and not wrong, wrong
