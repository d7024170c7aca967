"""-m "not gpu": `landmark_splits` of static / rolling incremental decoding (init_*_decoding(landmark_splits=P): a step of at
most 8 tokens runs attn as ea_ceva_sdecode_attn_split + ea_ceva_sdecode_merge, P workgroups per window block sharing the
landmark rows): the interface, that the option's own refusal comes behind those of init_static_decoding, what the state
holds, and what the two entry points refuse before any launch (ABI 21).
Its numerics are tests/test_gpu_ceva_split_decode.py."""
import ctypes
import inspect
import re

import pytest
import torch

import efficient_attention as ea
from test_api_parity import _causal_eva
from test_cabi import HEADER, LIB, declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)

_INITS = ("init_static_decoding", "init_rolling_decoding")
_STATIC_ARGS = ["self", "incremental_state", "batch_size", "max_tokens", "dtype", "device"]


def _no_device(monkeypatch, allocate):
    """The device check stubbed, so that what comes behind it is reached without a GPU.  allocate: False -- any allocation
    fails the test; True -- the state's tensors are made on the CPU, the bias table and the mu copies left out."""
    from efficient_attention import _native
    monkeypatch.setattr(_native, "require_cuda", lambda *a, **k: None)
    if not allocate:
        monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("allocated before refusing"))
        return
    zeros = torch.zeros
    monkeypatch.setattr(torch, "zeros", lambda shape, dtype=None, device=None: zeros(shape, dtype=dtype))
    monkeypatch.setattr(ea.CausalEVAttention, "_decode_bias_table", lambda self, device: None)
    monkeypatch.setattr(ea.CausalEVAttention, "_decode_mu_f32", lambda self: [])


def test_landmark_splits_is_a_keyword_only_option():
    for which in _INITS:
        extra = ["max_step_tokens"] if "rolling" in which else []
        method = getattr(ea.CausalEVAttention, which)
        assert list(inspect.signature(method).parameters) == _STATIC_ARGS + extra       # the lists the other tests pin
        assert "landmark_splits" in method.__doc__ and "256 / (B h)" in method.__doc__  # ... and how to choose it
        for by_position in ([True, 4], [4]):                             # behind per_sequence, or in its place
            with pytest.raises(TypeError):
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", *([None] * len(extra)), *by_position)
        for kw in (dict(landmark_splits=4), dict(landmark_splits=4, per_sequence=True), dict(landmark_splits=1), {}):
            with pytest.raises(RuntimeError, match="no CPU fallback"):   # by keyword: the call goes on to the device check
                getattr(_causal_eva().eval(), which)({}, 2, 16, torch.bfloat16, "cpu", **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                getattr(_causal_eva().eval(), which)(incremental_state={}, batch_size=2, max_tokens=16, dtype=torch.bfloat16,
                                                     device="cpu", **kw)


@pytest.mark.parametrize("P", [0, -1, 65, 2.5, True, "4", None])
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_seq"])
def test_landmark_splits_out_of_range_is_a_value_error_that_names_it(P, per, monkeypatch):
    _no_device(monkeypatch, allocate=False)
    for which in _INITS:
        st = {}
        with pytest.raises(ValueError, match="landmark_splits") as got:
            getattr(_causal_eva().eval(), which)(st, 2, 16, torch.bfloat16, "cpu", per_sequence=per, landmark_splits=P)
        assert st == {} and repr(P) in str(got.value)


def test_the_refusals_of_init_static_decoding_come_first(monkeypatch):
    """A bad option does not hide what the state refuses anyway: same exception, same message as without the option."""
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
            for opt in ({}, dict(landmark_splits=4), dict(landmark_splits=0), dict(landmark_splits=2.5, per_sequence=True)):
                args = dict(dict(batch_size=2, max_tokens=16, dtype=torch.bfloat16, device="cpu"), **kw)
                st = {}
                with pytest.raises(exc) as got:
                    getattr(m_fn(), which)(st, **args, **opt)
                assert st == {}
                msgs.add(str(got.value))
        assert len(msgs) == 1 and "landmark_splits" not in msgs.pop(), (exc, msgs)
    _no_device(monkeypatch, allocate=False)
    for B, T in ((0, 16), (2, 0)):                                       # the sizes, behind the device check
        with pytest.raises(ValueError, match="batch_size > 0 and max_tokens > 0"):
            _causal_eva().eval().init_static_decoding({}, B, T, torch.bfloat16, "cpu", landmark_splits=0)
    with pytest.raises(ValueError, match="max_step_tokens"):             # a rolling state's own
        _causal_eva().eval().init_rolling_decoding({}, 2, 16, torch.bfloat16, "cpu", max_step_tokens=0, landmark_splits=0)
    monkeypatch.setattr(_f32, "ENABLED", False)
    with pytest.raises(ValueError, match="fp32 cores"):
        _causal_eva().eval().init_static_decoding({}, 2, 16, torch.float32, "cpu", landmark_splits=0)


@pytest.mark.parametrize("which", _INITS)
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_seq"])
def test_the_state_of_a_split_is_the_plain_state_and_one_workspace(which, per, monkeypatch):
    """Default 1; P = 1 and no option: the same keys and shapes; P > 1: one more tensor, fp32 [B, h, 8, P, d + 4], counted by
    decoding_state_nbytes; the host dict records P."""
    m = _causal_eva().eval()
    _no_device(monkeypatch, allocate=True)
    B, h, d = 3, m.num_heads, m.head_dim
    made = {}
    for name, kw in (("none", {}), ("one", dict(landmark_splits=1)), ("six", dict(landmark_splits=6))):
        st = {}
        getattr(m, which)(st, B, 40, torch.bfloat16, "cpu", per_sequence=per, **kw)
        made[name] = (m._get_input_buffer(st), dict(m.get_incremental_state(st, "attn_static")), m.decoding_state_nbytes(st))
    shapes = {n: {k: (tuple(v.shape), v.dtype) for k, v in buf.items() if torch.is_tensor(v)} for n, (buf, _, _) in made.items()}
    assert shapes["none"] == shapes["one"] and "split_ws" not in shapes["one"]
    assert made["none"][1] == made["one"][1] and made["one"][1]["landmark_splits"] == 1
    assert made["none"][2] == made["one"][2]
    assert made["six"][1] == dict(made["one"][1], landmark_splits=6)
    assert shapes["six"].pop("split_ws") == ((B, h, 8, 6, d + 4), torch.float32)
    assert shapes["six"] == shapes["one"]
    assert made["six"][2] == made["one"][2] + B * h * 8 * 6 * (d + 4) * 4


# ---- C ABI 21: ea_ceva_sdecode_attn_split, ea_ceva_sdecode_merge -----------------------------------------------------------
def test_abi_21_header_binding_and_exports_agree(lib):  # noqa: F811
    from efficient_attention import _native
    assert _native.lib().ea_abi_version() >= 21 and _native.ABI_VERSION == _native.lib().ea_abi_version()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} ea_ceva_sdec_geom;", text).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [n for n, _ in _native.ea_ceva_sdec_geom._fields_] and fields[-3:] == ["pos", "status", "ntok"]   # unchanged
    for name, nargs in (("ea_ceva_sdecode_attn_split", 12), ("ea_ceva_sdecode_merge", 5)):
        decl = re.search(r"int %s\(([^)]*)\);" % name, text).group(1)
        assert len(decl.split(",")) == nargs == len(_native.SIGNATURES[name])
        assert "const ea_ceva_sdec_geom* g" in decl and "int32_t parts" in decl and "ws" in decl and "void* stream" in decl
        assert hasattr(lib, name)
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert not [s for s in declared_symbols() if not hasattr(lib, s)]


_BADARG, _UNSUPPORTED = -1, -2
_BOTH = ("sdecode_attn_split", "sdecode_merge")
_SPLIT = ("sdecode_attn_split",)
# (entry point, what is wrong, expected return), in the manner of test_ceva_perseq_decode_cpu._NTOK_REFUSED.  pos, status,
# ntok and ws are offsets from a 16-byte aligned base: 0, 16, 32 (or None) and 48.  Only refused calls: an accepted one launches.
_SPLIT_REFUSED = (
    [(e, {"parts": n}, _BADARG) for e in _BOTH for n in (1, 0, -1, 65, 1 << 20)]
    + [(e, {"ws": off}, _BADARG) for e in _BOTH for off in (None, 52, 56, 49)]
    + [(e, {"T_new": n}, _BADARG) for e in _BOTH for n in (9, 16, 0, -1)]
    + [(e, {"pos": off}, _BADARG) for e in _BOTH for off in (None, 2)]
    + [(e, {"status": off}, _BADARG) for e in _BOTH for off in (None, 18)]
    + [(e, {"ntok": 34}, _BADARG) for e in _BOTH]
    + [(e, {"D": D}, _UNSUPPORTED) for e in _BOTH for D in (48, 256)]
    + [(e, {"D": 48, "ntok": 32}, _UNSUPPORTED) for e in _BOTH]
    # what the split adds is a fault of the static state: decided before the head dim, like the others
    + [(e, dict(bad, D=48), _BADARG) for e in _BOTH for bad in (
        {"parts": 1}, {"parts": 65}, {"ws": None}, {"ws": 52}, {"T_new": 9}, {"pos": None}, {"status": None}, {"cap": 60},
        {"ring": 16}, {"ntok": 34})]
    # ... and the rest of the shared-count and per-sequence tables
    + [(e, dict(bad, ntok=nt), _BADARG) for e in _BOTH for nt in (None, 32) for bad in (
        {"B": 0}, {"H": 0}, {"chunk": 3}, {"chunk": 0}, {"window": 0}, {"ext": -1}, {"cap": 60}, {"ring": 20}, {"ring": 8},
        {"dtype": 3}, {"out": None}, {"out.ptr": 8}, {"out.sn": 2})]
    + [(e, dict(bad, ntok=nt), _BADARG) for e in _SPLIT for nt in (None, 32) for bad in (
        {"pad": None}, {"q": None}, {"k.ptr": 4}, {"v.sh": 3}, {"lk": None}, {"lv.sn": 2}, {"bias": None})]
    + [(e, None, _BADARG) for e in _BOTH]                                # no geometry at all
)


def _refused_call(nv, entry, bad):
    """test_ceva_perseq_decode_cpu._refused_call for the two entry points of a split step."""
    buf = ctypes.create_string_buffer(96)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    geo = dict(B=2, H=2, D=64, dtype=nv.EA_BF16, window=8, ext=8, chunk=4, T_new=2, adaptive=1, has_bias=1, cap=64, ring=0,
               pos=0, status=16, ntok=None)
    arg = {n: {"ptr": 0, "sb": 2048, "sh": 64, "sn": 128} for n in ("q", "k", "v", "lk", "lv", "out")}
    arg.update(pad=0, bias=0, parts=4, ws=48)
    for key, val in (bad or {}).items():
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
    g = None if bad is None else ctypes.byref(nv.ea_ceva_sdec_geom(**geo))
    fn = getattr(nv.lib(), "ea_ceva_" + entry)
    if entry.endswith("attn_split"):
        return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), p(arg["bias"]), t("lk"), t("lv"), t("out"), arg["parts"],
                  p(arg["ws"]), None)
    return fn(g, t("out"), arg["parts"], p(arg["ws"]), None)


def test_split_entry_points_refuse_before_any_launch(lib):  # noqa: F811
    from efficient_attention import _native
    got = [(entry, bad, want, _refused_call(_native, entry, bad)) for entry, bad, want in _SPLIT_REFUSED]
    wrong = [row for row in got if row[2] != row[3]]
    assert len(got) >= 100 and not wrong, wrong
