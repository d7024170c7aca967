"""-m "not gpu": C ABI 29 -- the LARA forward combine with the output projection inside (ea_lara_out_proj_fwd_merge,
ea_lara_layer_fwd_proj) is bound with the header's argument counts, and the composite refuses out-of-scope geometry and bad
arguments on the host, before any HIP call (only refused calls here: an accepted one would launch)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ea_hip.h")
NEW = ("ea_lara_out_proj_fwd_merge", "ea_lara_layer_fwd_proj")
_BADARG, _UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def nv():
    from efficient_attention import _native
    if not os.path.exists(os.path.join(ROOT, "efficient-attention_amd", "lib", "libea_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    _native.lib()
    return _native


def _header_counts():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counts = {}
    for m in re.finditer(r"\b(ea_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        counts[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return counts


def test_abi_29_symbols_are_bound_with_the_headers_argument_counts(nv):
    assert nv.lib().ea_abi_version() == nv.ABI_VERSION >= 29
    counts = _header_counts()
    for name in NEW:
        assert hasattr(nv.lib(), name)
        assert counts[name] == len(nv.SIGNATURES[name]), name
    # the fused entries are their unfused counterparts plus (w_proj16, bias, y, ldy)
    assert len(nv.SIGNATURES["ea_lara_out_proj_fwd_merge"]) == len(nv.SIGNATURES["ea_lara_out_fwd_merge"]) + 4
    assert len(nv.SIGNATURES["ea_lara_layer_fwd_proj"]) == len(nv.SIGNATURES["ea_lara_layer_fwd"]) + 4
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in NEW) and "ABI 29" in doc


def _layer(nv, B=128, H=3, D=64, gh=28, gw=28, r=4, dup=0, mis=0):
    return nv.ea_lara_layer(B, H, D, 0, gh, gw, r, 1, 1, mis, dup, 2.0, D ** -0.5)


def _call_layer(nv, cfg, **over):
    """ea_lara_layer_fwd_proj on never-dereferenced host addresses (a refused call returns before any HIP call)."""
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    t = nv.ea_t4(base, 784 * 576, 64, 576)
    a = dict(q=ctypes.byref(t), out=ctypes.byref(t), saved=ctypes.c_void_p(base), tmp=ctypes.c_void_p(base),
             w=ctypes.c_void_p(base), bias=ctypes.c_void_p(base), y=ctypes.c_void_p(base), ldy=192,
             params=(ctypes.c_void_p * 8)(*[base] * 8))
    a.update(over)
    return nv.lib().ea_lara_layer_fwd_proj(ctypes.byref(cfg), a["q"], a["q"], a["q"], None, None, a["params"], a["out"], a["saved"],
                                           a["tmp"], 1, a["w"], a["bias"], a["y"], a["ldy"], None), base


def test_composite_refuses_out_of_scope_geometry_before_any_launch(nv):
    # C > 64 (antithetic sampling at 49 landmarks), heads != 3, d != 64, S_fwd > 4 (a small batch of long sequences)
    for cfg in (_layer(nv, B=2, gh=14, gw=14, r=2, dup=1), _layer(nv, H=2), _layer(nv, H=6, D=32), _layer(nv, H=4),
                _layer(nv, B=1)):
        assert _call_layer(nv, cfg)[0] == _UNSUPPORTED
        # ... decided before the pointers are looked at
        assert _call_layer(nv, cfg, w=None, y=None, q=None)[0] == _UNSUPPORTED
    assert nv.lib().ea_lara_layer_fwd_proj(None, *([None] * 9), 1, None, None, None, 192, None) == _BADARG
    bad_grid = _layer(nv, gw=27)
    assert _call_layer(nv, bad_grid)[0] == _BADARG


def test_composite_refuses_bad_projection_operands(nv):
    cfg = _layer(nv)                                                     # in scope: the benchmark's geometry
    base = _call_layer(nv, _layer(nv, H=2))[1]
    for over in (dict(w=None), dict(y=None), dict(ldy=191), dict(ldy=190), dict(ldy=194), dict(q=None), dict(out=None),
                 dict(saved=None), dict(tmp=None), dict(params=None)):
        assert _call_layer(nv, cfg, **over)[0] == _BADARG, over
    buf = ctypes.create_string_buffer(256)
    b16 = (ctypes.addressof(buf) + 15) & ~15
    for over in (dict(w=ctypes.c_void_p(b16 + 8)), dict(y=ctypes.c_void_p(b16 + 4)), dict(bias=ctypes.c_void_p(b16 + 2))):
        assert _call_layer(nv, cfg, **over)[0] == _BADARG, over
    assert base


def test_step_entry_refuses_out_of_scope_geometry(nv):
    fn = nv.lib().ea_lara_out_proj_fwd_merge
    nul = [None] * 3
    for B, H, D, C, S, want in ((2, 2, 64, 49, 2, _UNSUPPORTED), (2, 6, 32, 49, 2, _UNSUPPORTED), (2, 3, 64, 98, 2, _UNSUPPORTED),
                                (2, 3, 64, 49, 5, _UNSUPPORTED), (2, 3, 64, 49, 2, _BADARG), (2, 3, 48, 49, 2, _BADARG)):
        g = nv.ea_lara_geom(B, H, 196, D, 0, C, 0, 2.0, 0.125)
        rc = fn(ctypes.byref(g), None, *nul, S, *([None] * 7), None, None, None, None, None, None, 192, None)
        assert rc == want, (B, H, D, C, S, rc)
