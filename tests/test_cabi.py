"""-m "not gpu": the C-ABI library loads and exports every symbol include/ea_hip.h declares, and
the ctypes binding table covers exactly that set (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ea_hip.h")
LIB = os.path.join(ROOT, "efficient-attention_amd", "lib", "libea_hip.so")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ea_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert len(syms) >= 25, syms
    for must in ("ea_window_attn_fwd", "ea_window_attn_bwd", "ea_lara_stats_fwd", "ea_lara_out_fwd",
                 "ea_softmax_attn_fwd", "ea_performer_out", "ea_eva_beta_fwd", "ea_version"):
        assert must in syms


def test_library_exports_every_declared_symbol(lib):
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_binding_table_matches_header():
    from efficient_attention import _native
    bound = set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"}
    assert bound == set(declared_symbols())


def test_binding_table_argument_counts_match_header():
    """Every ctypes signature has as many arguments as the header's declaration (round 6: a binding that lagged one argument
    behind its declaration passed the name-only check and failed on the GPU box)."""
    from efficient_attention import _native
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counts = {}
    for m in re.finditer(r"\b(ea_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        counts[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    bad = {n: (len(sig), counts.get(n)) for n, sig in _native.SIGNATURES.items() if counts.get(n) != len(sig)}
    assert not bad, bad


def test_version_and_argument_validation(lib):
    from efficient_attention import _native
    assert _native.version().startswith("ea_hip") and "gfx950" in _native.version()
    assert _native.lib().ea_abi_version() >= 1
    # NULL / inconsistent geometry is rejected on the host, before any launch
    g = _native.make_geom(2, 3, 196, 64, 0, True, (14, 14), 7, 0, 2, 49)
    assert _native.lib().ea_window_bias_ld(ctypes.byref(g)) == 64
    assert _native.lib().ea_window_bwd_parts(ctypes.byref(g)) >= 1
    bad = _native.make_geom(2, 3, 196, 64, 0, True, (14, 13), 7, 0, 2, 49)
    assert _native.lib().ea_window_bias_ld(ctypes.byref(bad)) < 0
    rc = _native.lib().ea_window_attn_fwd(ctypes.byref(g), None, None, None, None, None, None, None, None, None, None, 1.0, None)
    assert rc == -1
    odd = _native.make_geom(2, 3, 196, 48, 0, True, (14, 14), 7, 0, 2, 49)     # head dim not built
    assert _native.lib().ea_window_bias_ld(ctypes.byref(odd)) < 0


def test_composite_layer_entry_points_report_their_workspaces(lib):
    """ea_lara_layer_plan / _fwd / _bwd (one call per direction for the whole LARA core): sizes on the host, argument
    validation before any launch.  The numerical check of the composite path is every LARA test of the GPU suite (the
    module goes through it) plus tests/test_gpu_primitives.py::test_lara_composite_equals_step_by_step; the layout itself is
    pinned by tests/test_layer_plan_cpu.py."""
    from efficient_attention import _native
    L = _native.lib()
    cfg = _native.ea_lara_layer(128, 3, 64, 0, 28, 28, 4, 1, 1, 0, 0, 2.0, 0.125)      # cfg3: 49 landmarks, mis-opt, pool-mixed
    n = _native.ea_lara_layer_sizes()
    assert L.ea_lara_layer_plan(ctypes.byref(cfg), ctypes.byref(n)) == 0
    BH, C, Lm, D, N = 384, 49, 49, 64, 784
    assert n.n_saved >= 3 * BH * C * D + 2 * BH * Lm * D + 2 * BH * N and n.n_fwd_tmp >= BH * C * D and n.n_bwd_tmp >= 9 * BH * C * D
    assert L.ea_lara_layer_plan(ctypes.byref(cfg), None) == -1
    bad = _native.ea_lara_layer(128, 3, 64, 0, 28, 27, 4, 1, 1, 0, 0, 2.0, 0.125)      # grid not divisible by the pooling side
    assert L.ea_lara_layer_plan(ctypes.byref(bad), ctypes.byref(n)) == -1
    big = _native.ea_lara_layer(2, 3, 64, 0, 28, 28, 2, 0, 0, 0, 0, 2.0, 0.125)        # 196 landmarks: step-by-step path
    assert L.ea_lara_layer_plan(ctypes.byref(big), ctypes.byref(n)) == -2
    rc = L.ea_lara_layer_fwd(ctypes.byref(cfg), None, None, None, None, None, None, None, None, None, 1, None)
    assert rc == -1
    assert L.ea_lara_layer_bwd(ctypes.byref(cfg), None, None, None, None, None, None, None, None, None, None, None, None, None,
                               0, None) == -1


def test_eva_composite_entry_points_report_their_workspaces(lib):
    """ea_eva_layer_plan / _fwd / _bwd (one call per direction for the 2-D EVA core): host-side sizes and argument validation.
    Numerics: tests/test_gpu_primitives.py::test_eva_composite_equals_step_by_step and every EVA test of the GPU suite."""
    from efficient_attention import _native
    L = _native.lib()
    cfg = _native.ea_eva_layer(128, 3, 64, 0, 28, 28, 7, 4, 1, 0.125)              # cfg3: 7 x 7 windows, 49 chunks of 4 x 4
    n = _native.ea_eva_layer_sizes()
    assert L.ea_eva_layer_plan(ctypes.byref(cfg), ctypes.byref(n)) == 0
    BH, Lm, D, N = 384, 49, 64, 784
    assert n.n_saved >= BH * N + 5 * BH * Lm * D and n.n_bwd_tmp >= 5 * BH * Lm * D + BH * (2 * D * D + 6 * D)
    assert 0 <= n.saved_lse < n.saved_qmean < n.saved_kmean < n.n_saved and 0 <= n.bwd_dW < n.bwd_dvec < n.n_bwd_tmp and n.bias_ld >= 49
    geom = _native.make_geom(128, 3, N, 64, 0, True, (28, 28), 7, 0, 4, 49)
    assert n.bias_ld == L.ea_window_bias_ld(ctypes.byref(geom))
    # bias-gradient partials in the scratch
    assert 0 <= n.bwd_dbias_part < n.n_bwd_tmp and n.dbias_part_rows >= 128
    assert n.bwd_dbias_part + n.dbias_part_rows * 3 * 49 * n.bias_ld <= n.n_bwd_tmp
    assert 0 <= n.n_bwd_tmp and 0 <= n.bwd_dqmean < n.bwd_dkmean < n.n_bwd_tmp                        # d(chunk means) (ABI 10)
    assert L.ea_eva_layer_plan(ctypes.byref(cfg), None) == -1
    bad = _native.ea_eva_layer(128, 3, 64, 0, 28, 28, 8, 4, 1, 0.125)              # grid not divisible by the window side
    assert L.ea_eva_layer_plan(ctypes.byref(bad), ctypes.byref(n)) == -1
    big = _native.ea_eva_layer(2, 3, 64, 0, 28, 28, 7, 2, 0, 0.125)                # 196 landmarks: step-by-step path
    assert L.ea_eva_layer_plan(ctypes.byref(big), ctypes.byref(n)) == -2
    odd = _native.ea_eva_layer(2, 3, 48, 0, 28, 28, 7, 4, 0, 0.125)                # head dim not built
    assert L.ea_eva_layer_plan(ctypes.byref(odd), ctypes.byref(n)) == -2
    assert L.ea_eva_layer_fwd(ctypes.byref(cfg), None, None, None, None, None, None, None, None, 1, None) == -1
    assert L.ea_eva_layer_bwd(ctypes.byref(cfg), None, None, None, None, None, None, None, None, None, None, None, None, None,
                              None, None, 0, None) == -1


# ---- causal EVA decoding: what the six ea_ceva_* entry points refuse, before any HIP call --------------------------------
# (entry point, what is wrong, expected return).  Geometry fields are overridden by name; a pointer is None (null) or an
# offset from a 16-byte aligned host address; "q.sn" is a field of the ea_t4 `q`, "mu.3" the fourth mu parameter.  The valid
# base: B 2, H 2, D 64, bf16, window 8, ext 8, chunk 4, T_new 2; dynamic t0 6, chunk 1 closing, cap 16; static cap 64, ring 0.
# The expected codes are those of the library as it was BEFORE the entry points were folded onto one validation (this table
# run against a build of that commit); where two faults meet, the rows pin which one decides.  (A ring behind
# ea_ceva_decode_* cannot be written down here: ea_ceva_dec_geom has no such field, the refusal lives behind the C ABI.)
_BADARG, _UNSUPPORTED = -1, -2
_CEVA_DYNAMIC = ("decode_close", "decode_attn")
_CEVA_STATIC = ("sdecode_close", "sdecode_attn")
_CEVA_REFUSED = (
    [(e, {"g": None}, _BADARG) for e in _CEVA_DYNAMIC + _CEVA_STATIC + ("sdecode_append", "sdecode_advance")]
    # both families: the geometry dec_fill checks, the rows, the landmark rows, the pad flags
    + [(e, bad, _BADARG) for e in _CEVA_DYNAMIC + _CEVA_STATIC for bad in (
        {"B": 0}, {"H": 0}, {"window": 0}, {"chunk": 0}, {"ext": -1}, {"T_new": 0}, {"dtype": 3}, {"dtype": -1},
        {"q": None}, {"k.ptr": None}, {"v.ptr": 2}, {"q.sn": 32}, {"k.sb": 4}, {"v.sh": 12}, {"lk": None}, {"lv.ptr": 8},
        {"lv.sn": 2}, {"pad": None}, {"D": 48, "dtype": 3}, {"D": 48, "T_new": 0})]
    + [(e, {"D": 48}, _UNSUPPORTED) for e in _CEVA_DYNAMIC + _CEVA_STATIC]
    + [(e, {"D": 96}, _UNSUPPORTED) for e in _CEVA_DYNAMIC + _CEVA_STATIC]
    + [(e, {"D": 48, "q.ptr": 2}, _UNSUPPORTED) for e in _CEVA_DYNAMIC + _CEVA_STATIC]       # D is decided before the rows
    # dynamic: the step inside the cache, the chunks inside the step
    + [(e, bad, _BADARG) for e in _CEVA_DYNAMIC for bad in ({"t0": -1}, {"cap": 7}, {"t0": 15})]
    + [("decode_close", bad, _BADARG) for bad in (
        {"mu": None}, {"mu.0": None}, {"mu.7": None}, {"mu.3": 4}, {"c_first": -1}, {"c_first": 2}, {"c_last": 2},
        {"adaptive": 0, "mu.3": None})]
    + [("decode_close", {"D": 48, "mu": None}, _UNSUPPORTED), ("decode_close", {"D": 48, "c_last": 0}, _UNSUPPORTED)]
    # static: the counters, the capacity in whole windows, the ring -- all decided before D
    + [(e, bad, _BADARG) for e in _CEVA_STATIC for bad in (
        {"pos": None}, {"status": None}, {"pos": 2}, {"status": 18}, {"cap": 60}, {"chunk": 3}, {"ring": 20}, {"ring": 16},
        {"ring": -8}, {"cap": 0}, {"D": 48, "pos": None}, {"D": 48, "cap": 60}, {"D": 48, "ring": 16}, {"D": 48, "pad": None})]
    + [("sdecode_close", bad, _BADARG) for bad in ({"mu": None}, {"mu.4": None}, {"mu.1": 8})]
    + [("sdecode_close", {"D": 48, "mu": None}, _UNSUPPORTED)]
    # attn, both families: the output rows and the bias
    + [(e, bad, _BADARG) for e in ("decode_attn", "sdecode_attn") for bad in (
        {"out": None}, {"out.ptr": 4}, {"out.sn": 8}, {"bias": None})]
    + [(e, {"D": 48, "bias": None}, _UNSUPPORTED) for e in ("decode_attn", "sdecode_attn")]
    # append: its own subset, D last
    + [("sdecode_append", bad, _BADARG) for bad in (
        {"pos": None}, {"status": None}, {"pos": 2}, {"status": 18}, {"pad": None}, {"qkv_new": None}, {"qkv": None},
        {"qkv_new": 8}, {"qkv": 4}, {"B": 0}, {"H": 0}, {"T_new": 0}, {"cap": 1}, {"dtype": 3}, {"ring": 20}, {"ring": 16},
        {"D": 48, "pos": None}, {"D": 48, "dtype": 3}, {"D": 48, "qkv": 4}, {"D": 48, "ring": 16})]
    + [("sdecode_append", {"D": 48}, _UNSUPPORTED)]
    + [("sdecode_advance", bad, _BADARG) for bad in ({"pos": None}, {"pos": 2}, {"T_new": 0}, {"cap": 1})]
)


def _ceva_refused_call(nv, entry, bad):
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: a refused call returns before any HIP call
    static = entry.startswith("sdecode")
    geo = dict(B=2, H=2, D=64, dtype=nv.EA_BF16, window=8, ext=8, chunk=4, T_new=2, adaptive=1, has_bias=1)
    geo.update(dict(cap=64, ring=0, pos=0, status=16) if static else dict(cap=16, t0=6, c_first=1, c_last=1, has_mask=1))
    arg = {n: {"ptr": 0, "sb": 2048, "sh": 64, "sn": 128} for n in ("q", "k", "v", "lk", "lv", "out")}
    arg.update(g=1, pad=0, bias=0, qkv_new=0, qkv=0, mu=[0] * 8)
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
    for key in ("pos", "status"):
        if key in geo:
            geo[key] = None if geo[key] is None else base + geo[key]
    geom = (nv.ea_ceva_sdec_geom if static else nv.ea_ceva_dec_geom)(**geo)
    g = None if arg["g"] is None else ctypes.byref(geom)
    mu = None if arg["mu"] is None else (ctypes.c_void_p * 8)(*[None if m is None else base + m for m in arg["mu"]])
    fn = getattr(nv.lib(), "ea_ceva_" + entry)
    if entry.endswith("close"):
        return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), mu, t("lk"), t("lv"), None)
    if entry.endswith("attn"):
        return fn(g, t("q"), t("k"), t("v"), p(arg["pad"]), p(arg["bias"]), t("lk"), t("lv"), t("out"), None)
    if entry.endswith("append"):
        return fn(g, p(arg["qkv_new"]), None, p(arg["qkv"]), p(arg["pad"]), None)
    return fn(g, None)


def test_ceva_decoding_entry_points_refuse_before_any_launch(lib):
    """Every refused argument combination of ea_ceva_decode_* / ea_ceva_sdecode_* keeps its return code, and where two faults
    meet, the one that decided before still decides (_CEVA_REFUSED).  Only refused calls: an accepted one would launch."""
    from efficient_attention import _native
    got = [(entry, bad, want, _ceva_refused_call(_native, entry, bad)) for entry, bad, want in _CEVA_REFUSED]
    wrong = [row for row in got if row[2] != row[3]]
    assert len(got) >= 150 and not wrong, wrong
