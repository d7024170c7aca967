"""-m "not gpu": the one rule every strided [B,H,N,D] view (ea_t4) must meet, pinned through one entry point per view family.

The rule: the view and its base pointer are not null, the base is 16-byte aligned, every stride is a multiple of the 16-byte
granule (8 elements of a 16-bit type, 4 of fp32) and the token stride covers the head dim (sn >= D).  Each case hands an
entry point an accepted geometry, non-null dummy host buffers for every pointer and views that are valid but for ONE defect
in ONE view.  A refusal is decided before any launch, so nothing here touches a device, and no case is a fully valid call.

The expected codes were recorded from the library as it was when the rule was still written out once per family (t4_ok,
pf_t4_ok, f32_t4_ok, dec_t4_ok in ea_capi.hip): every one of the 259 cases answered EA_E_BADARG there, on a machine without
a GPU too -- no geometry step of these eight entry points asks the device anything."""
import ctypes

import pytest

_BADARG = -1
_D = 64


def _geoms(nv):
    return {
        # causal: the one window geometry that takes a keep mask (without it a non-null `keep` is EA_E_UNSUPPORTED first)
        "window": nv.make_geom(2, 3, 192, _D, 0, False, None, 16, 16, 4, 48, causal=1),
        "lara": nv.ea_lara_geom(2, 3, 196, _D, 0, 49, 0, 0.0, 0.125),
        "perf16": nv.ea_perf_geom(2, 3, 196, _D, 0, 64),
        "perf_bf16": nv.ea_perf_geom(2, 3, 196, _D, 0, 64),
        "perf_f32": nv.ea_perf_geom(2, 3, 196, _D, 2, 64),
        "kz_bf16": nv.ea_kz_geom(2, 3, 196, _D, 0, 0, 64, 64, 0, 0),
        "kz_f32": nv.ea_kz_geom(2, 3, 196, _D, 2, 2, 64, 128, 0, 0),
        "sb": nv.ea_sb_geom(2, 3, 196, _D, 0, 64, 0, 1, 196, 14),
        "ga": nv.ea_f32_attn(B=2, H=3, Nq=196, Nk=196, D=_D, G=4, Wq=49, Wk=49, L=4, bias_ld=49, keep_ld=53,
                             keep_scale=1.0, scale=0.125),
        "dec_bf16": nv.ea_ceva_dec_geom(B=2, H=2, D=_D, dtype=0, window=8, ext=8, chunk=4, t0=6, T_new=2, c_first=1,
                                        c_last=1, cap=16, adaptive=1, has_bias=1, has_mask=1),
        "dec_f32": nv.ea_ceva_dec_geom(B=2, H=2, D=_D, dtype=2, window=8, ext=8, chunk=4, t0=6, T_new=2, c_first=1,
                                       c_last=1, cap=16, adaptive=1, has_bias=1, has_mask=1),
    }


# (case id, entry point, geometry, arguments after the geometry): "p" a non-null pointer, a float as itself, None the
# stream, (name, granule) a view whose strides come in multiples of `granule` elements
_V8 = lambda name: (name, 8)          # noqa: E731
_V4 = lambda name: (name, 4)          # noqa: E731
_ENTRIES = (
    ("window", "ea_window_attn_fwd", "window",
     (_V8("q"), _V8("k"), _V8("v"), "p", "p", "p", "p", _V8("out"), "p", "p", 1.0, None)),
    ("lara", "ea_lara_stats_fwd", "lara", (_V8("q"), _V8("k"), _V8("v"), "p", "p", "p", "p", "p", None)),
    ("performer16", "ea_performer_kv", "perf16", (_V8("k"), _V8("v"), "p", "p", "p", "p", "p", None)),
    ("performer_f32-bf16", "ea_performer_f32_kv", "perf_bf16", (_V8("k"), _V8("v"), "p", "p", "p", "p", "p", None)),
    ("performer_f32-f32", "ea_performer_f32_kv", "perf_f32", (_V4("k"), _V4("v"), "p", "p", "p", "p", "p", None)),
    ("kernelized-bf16", "ea_kernelized_kv", "kz_bf16", (_V8("k"), _V8("v"), "p", "p", "p", "p", "p", None)),
    ("kernelized-f32", "ea_kernelized_kv", "kz_f32", (_V4("k"), _V4("v"), "p", "p", "p", "p", "p", None)),
    ("scatter", "ea_scatter_kv", "sb", (_V8("k"), _V8("v"), "p", "p", "p", "p", "p", None)),
    ("f32_attn", "ea_f32_attn_fwd", "ga",
     (_V4("q"), _V4("k"), _V4("v"), _V4("ek"), _V4("ev"), "p", "p", "p", "p", "p", "p", _V4("out"), "p", "p", None)),
    ("ceva_decode-bf16", "ea_ceva_decode_attn", "dec_bf16",
     (_V8("q"), _V8("k"), _V8("v"), "p", "p", _V4("lk"), _V4("lv"), _V8("out"), None)),
    ("ceva_decode-f32", "ea_ceva_decode_attn", "dec_f32",
     (_V4("q"), _V4("k"), _V4("v"), "p", "p", _V4("lk"), _V4("lv"), _V4("out"), None)),
)
_DEFECTS = ("null view", "null ptr", "ptr % 16 == 8", "sb", "sh", "sn", "sn < D")
_CASES = [(cid, fn, geom, args, view, defect) for cid, fn, geom, args in _ENTRIES
          for view in (a[0] for a in args if isinstance(a, tuple)) for defect in _DEFECTS]
# the code each case got from the library before the four statements of the rule became one; all of them EA_E_BADARG
_RECORDED = {(c[0], c[4], c[5]): _BADARG for c in _CASES}


def _refused_call(nv, fn, geom, args, view, defect):
    buf = ctypes.create_string_buffer(4096 + 16)          # never dereferenced: a refused call returns before any HIP call
    base = (ctypes.addressof(buf) + 15) & ~15
    keep, call = [], [ctypes.byref(geom)]
    for a in args:
        if not isinstance(a, tuple):
            call.append(ctypes.c_void_p(base) if a == "p" else a)
            continue
        name, gran = a
        t = dict(ptr=base, sb=64 * 3 * 256, sh=256, sn=3 * 256)              # a [B, N, 3, h = 3, 64 (+ padding)] buffer
        if name == view:
            if defect == "null view":
                call.append(None)
                continue
            if defect == "null ptr":
                t["ptr"] = None
            elif defect == "ptr % 16 == 8":
                t["ptr"] = base + 8
            elif defect == "sn < D":
                t["sn"] = _D - gran
            else:
                t[defect] += gran // 2                    # an odd multiple of half the granule
                assert t[defect] % gran == gran // 2 and (t[defect] // (gran // 2)) % 2 == 1
        keep.append(nv.ea_t4(t["ptr"], t["sb"], t["sh"], t["sn"]))
        call.append(ctypes.byref(keep[-1]))
    return getattr(nv.lib(), fn)(*call)


def test_case_table_covers_every_family_and_defect():
    assert len(_CASES) == len(_RECORDED) == 7 * sum(sum(isinstance(a, tuple) for a in e[3]) for e in _ENTRIES) == 259
    assert {e[1] for e in _ENTRIES} == {"ea_window_attn_fwd", "ea_lara_stats_fwd", "ea_performer_kv", "ea_performer_f32_kv",
                                        "ea_kernelized_kv", "ea_scatter_kv", "ea_f32_attn_fwd", "ea_ceva_decode_attn"}


@pytest.mark.parametrize("cid,fn,geom,args", _ENTRIES, ids=[e[0] for e in _ENTRIES])
def test_one_defect_in_one_view_is_refused_with_the_recorded_code(cid, fn, geom, args):
    from efficient_attention import _native as nv
    g = _geoms(nv)[geom]
    got = {(c[0], c[4], c[5]): _refused_call(nv, fn, g, args, c[4], c[5]) for c in _CASES if c[0] == cid}
    wrong = {k: (v, _RECORDED[k]) for k, v in got.items() if v != _RECORDED[k]}
    assert got and not wrong, wrong
