"""-m "not gpu": ScatterBrain with overlapping windows -- which geometries the HIP feature half accepts, and what the
ea_scatter_ov_* entry points refuse on the host, before any launch (refused calls only: an accepted one would launch)."""
import ctypes

import pytest
import torch

_BADARG, _UNSUPPORTED = -1, -2


def _qkv(N, h=3, d=64):
    return torch.empty(1, N, 3, h, d, dtype=torch.bfloat16, device="meta")


def _proj(m, h=3, d=64):
    return torch.empty(h, m, d, device="meta")


@pytest.mark.parametrize("seq,w,two_d,m", [((28, 28), 7, True, 64), ((56, 56), 7, True, 32), ((32, 32), 8, True, 16),
                                           ((1024,), 16, False, 64), ((512,), 64, False, 32), ((200,), 8, False, 64)])
def test_scatter_supported_accepts_the_overlapping_geometries(seq, w, two_d, m):
    from efficient_attention import _ops
    N = seq[0] * (seq[1] if two_d else 1)
    assert _ops.scatter_supported(_qkv(N), _proj(m), two_d, list(seq), w, w // 2)
    assert _ops.scatter_supported(_qkv(N), _proj(m), two_d, list(seq), w)              # and without overlap, as before


def test_scatter_supported_refuses_what_the_kernels_do_not_cover():
    from efficient_attention import _ops
    assert not _ops.scatter_supported(_qkv(81 * 4), _proj(64), True, [18, 18], 9, 4)         # Wq = 81 > 64
    assert not _ops.scatter_supported(_qkv(256), _proj(64), False, [256], 128, 64)           # Wq = 128 > 64
    assert not _ops.scatter_supported(_qkv(784), _proj(96), True, [28, 28], 7, 3)            # m > 64
    assert not _ops.scatter_supported(_qkv(784, d=32), _proj(64, d=32), True, [28, 28], 7, 3)   # d != 64
    assert not _ops.scatter_supported(_qkv(784), _proj(64), True, [28, 28], 7, 8)            # patch beyond the adjacent windows


def _call(nv, entry, geom, ext, null=None):
    """One ea_scatter_ov_* call with valid-looking (never dereferenced) arguments; `null`: index of the argument after
    (geom, ext) that is passed as a null pointer."""
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    t = ctypes.byref(nv.ea_t4(base, 784 * 3 * 192, 64, 3 * 192))
    p = ctypes.c_void_p(base)
    g = None if geom is None else ctypes.byref(geom)
    if entry == "windows":
        return nv.lib().ea_scatter_ov_windows(g, ext)
    # (the key-padding mask is optional: its slot stays null)
    args = {"fwd": [t, t, t, None, p, p, p, p, t, p, t, p],
            "bwd_window": [t, t, t, None, p, p, p, p, t, p, p, t, t, t, p, p, p, p],
            "bwd_keys": [t, t, None, p, p, p, p, p, p, t, t]}[entry]
    if null is not None:
        args[null] = None
    return getattr(nv.lib(), "ea_scatter_ov_" + entry)(g, ext, *args, None)


_ENTRIES = ("fwd", "bwd_window", "bwd_keys")


def _geom(nv, **over):
    f = dict(B=2, H=3, N=784, D=64, dtype=nv.EA_BF16, M=64, attn_2d=1, gh=28, gw=28, window=7)
    f.update(over)
    return nv.ea_sb_geom(f["B"], f["H"], f["N"], f["D"], f["dtype"], f["M"], f["attn_2d"], f["gh"], f["gw"], f["window"])


def test_overlapping_entry_points_refuse_before_any_launch():
    from efficient_attention import _native as nv
    nv.lib()
    ok = _geom(nv)
    assert nv.lib().ea_scatter_ov_windows(ctypes.byref(ok), 3) == 16
    assert nv.lib().ea_scatter_ov_windows(ctypes.byref(_geom(nv, attn_2d=0, gh=1, gw=784, N=784, window=8)), 4) == 98
    assert nv.lib().ea_scatter_ov_windows(ctypes.byref(_geom(nv, dtype=nv.EA_F16)), 7) == 16
    got = []
    for entry in _ENTRIES + ("windows",):
        got += [
            (entry, "null geometry", _BADARG, _call(nv, entry, None, 3)),
            (entry, "ext < 0", _BADARG, _call(nv, entry, ok, -1)),
            (entry, "ext > w", _UNSUPPORTED, _call(nv, entry, ok, 8)),
            (entry, "grid not divisible by w", _BADARG, _call(nv, entry, _geom(nv, gh=27, N=27 * 28), 3)),
            (entry, "1-D length not divisible by w", _BADARG, _call(nv, entry, _geom(nv, attn_2d=0, gh=1, gw=100, N=100, window=8), 4)),
            (entry, "fp32 rows", _BADARG, _call(nv, entry, _geom(nv, dtype=2), 3)),
            (entry, "unknown dtype", _BADARG, _call(nv, entry, _geom(nv, dtype=7), 3)),
            (entry, "B = 0", _BADARG, _call(nv, entry, _geom(nv, B=0), 3)),
            (entry, "Wq > 64", _UNSUPPORTED, _call(nv, entry, _geom(nv, gh=27, gw=27, N=729, window=9), 4)),
            (entry, "m > 64", _UNSUPPORTED, _call(nv, entry, _geom(nv, M=96), 3)),
            (entry, "d != 64", _UNSUPPORTED, _call(nv, entry, _geom(nv, D=32), 3)),
        ]
    # every pointer but the optional mask is required
    n_args = {"fwd": 12, "bwd_window": 18, "bwd_keys": 11}
    mask_at = {"fwd": 3, "bwd_window": 3, "bwd_keys": 2}
    for entry in _ENTRIES:
        for i in range(n_args[entry]):
            if i != mask_at[entry]:
                got.append((entry, "null argument %d" % i, _BADARG, _call(nv, entry, ok, 3, null=i)))
    wrong = [row for row in got if row[2] != row[3]]
    assert len(got) >= 80 and not wrong, wrong
