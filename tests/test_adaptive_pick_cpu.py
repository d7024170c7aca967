"""-m "not gpu": the greedy pick from the adaptive head (csrc/ea_adaptive_pick.hip, C ABI 34: ea_adaptive_pick_ws,
ea_adaptive_pick; DecoderStack.init_adaptive_decoding): the header, the binding table and the version, the workspace query
against a host restatement of the documented layout, every argument error's code without a device, the fp64 host reference
(tests/adaptive_pick_reference.py) against the reference's arrays (tests/golden/adaptive_small.npz), and the stack's errors."""
import ctypes
import re

import numpy as np
import pytest
import torch

import adaptive_pick_reference as pref
from test_adaptive_cpu import ATTN, _small_state
from test_cabi import HEADER, declared_symbols

NEW = {"ea_adaptive_pick_ws": 4, "ea_adaptive_pick": 18}


def test_p0_header_binding_and_version():
    from efficient_attention import _native
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counts = {m.group(1): m.group(2).count(",") + 1
              for m in re.finditer(r"\b(ea_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    for name, n in NEW.items():
        assert name in declared_symbols() and counts[name] == n and len(_native.SIGNATURES[name]) == n, name
        assert hasattr(_native.lib(), name)
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 34
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert _native.lib().ea_adaptive_pick_ws.restype is ctypes.c_int64
    SPAN, MAX_K = pref.constants()
    assert SPAN % 128 == 0 and MAX_K % 32 == 0


def _ws(M, cutoffs, dims):
    from efficient_attention import _native as nv
    return nv.lib().ea_adaptive_pick_ws(M, len(dims), nv.host_array(ctypes.c_int64, cutoffs), nv.host_array(ctypes.c_int32, dims))


def test_p0_the_workspace_query_runs_on_the_cpu_and_equals_the_documented_layout():
    from efficient_attention import _native as nv
    SPAN, MAX_K = pref.constants()
    r16 = pref.r16
    cases = ((1, [96, 200, 333], [64, 32]), (64, [96, 200, 333], [64, 32]), (17, [37, 187, 257], [64, 32]),
             (64, [20000, 60000, 267744], [256, 64]), (33, [48, 48 + 3 * SPAN + 5], [256]),
             (64, [40, 100, 160, 300, 500], [64, 32, 32, MAX_K + 32]), (1, [1, 2], [32]))
    for M, cutoffs, dims in cases:
        lay = pref.ws_layout(M, cutoffs, dims)
        assert _ws(M, cutoffs, dims) == lay["total"], (M, cutoffs, dims)
        n, D = len(dims), sum(dims)
        sizes = [c - a for a, c in zip([0] + cutoffs[:-1], cutoffs)]
        parts = [-(-sizes[0] // 16)] + [-(-sizes[i + 1] // (SPAN if d <= MAX_K else 16)) for i, d in enumerate(dims)]
        assert lay["parts"] == parts
        formula = r16(4 * M * n) + r16(2 * M * D) + (n + 1) * (r16(8 * M) + 2 * r16(4 * M)) \
            + sum(r16(8 * M) for d in dims if d > MAX_K) + r16(8 * M) + r16(4 * M) \
            + sum(r16(8 * M * P) + r16(4 * M * P) for P in parts)
        assert lay["total"] == formula
    for cutoffs, dims in (c[1:] for c in cases[:5]):
        sizes = [_ws(M, cutoffs, dims) for M in (1, 2, 17, 64)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), "the workspace grows with M"
    good = ([96, 200, 333], [64, 32])
    assert _ws(0, *good) < 0 and _ws(65, *good) < 0                  # 1 <= M <= 64
    assert _ws(8, [96, 96, 333], [64, 32]) < 0                      # not increasing
    assert _ws(8, [0, 200, 333], [64, 32]) < 0                      # c0 < 1
    assert _ws(8, [96, 200, 333], [64, 0]) < 0                      # d_i < 1
    assert _ws(8, [96, 200, 2 ** 31], [64, 32]) < 0                 # V past the envelope
    assert _ws(8, [1, 2, 3, 4, 5, 6], [32] * 5) < 0                 # more tails than EA_ADAPTIVE_MAX_TAILS
    assert nv.lib().ea_adaptive_pick_ws(8, 0, nv.host_array(ctypes.c_int64, [5]), nv.host_array(ctypes.c_int32, [32])) < 0
    assert nv.lib().ea_adaptive_pick_ws(8, 2, None, None) < 0


def test_p0_argument_errors_are_decided_before_any_launch():
    """Every refusal has its code with no device present: a launch would fail differently."""
    from efficient_attention import _native as nv
    lib = nv.lib()
    BAD, UNS = -1, -2
    cut, dims = nv.host_array(ctypes.c_int64, [96, 200, 333]), nv.host_array(ctypes.c_int32, [64, 32])
    fake, big = ctypes.c_void_p(4096), 1 << 40                       # (aligned, never dereferenced: the call stops before)
    ptrs = nv.host_array(ctypes.c_void_p, [4096, 4096])

    def call(M=10, C=128, n=2, cut=cut, dims=dims, x=fake, x_dtype=2, ldx=128, targets=fake, head=fake, w_dtype=0, proj=ptrs,
             tables=ptrs, ws=fake, ws_bytes=big, token=fake, logp=fake):
        return lib.ea_adaptive_pick(M, C, n, cut, dims, x, x_dtype, ldx, targets, head, w_dtype, proj, tables, ws, ws_bytes,
                                    token, logp, None)
    assert nv.EA_F32 == 2 and nv.EA_BF16 == 0
    odd = ctypes.c_void_p(4096 + 4)
    for kw in (dict(cut=None), dict(dims=None), dict(proj=None), dict(tables=None), dict(x=None), dict(head=None),
               dict(ws=None), dict(token=None), dict(logp=None), dict(M=0), dict(C=0), dict(n=0), dict(ldx=64),
               dict(cut=nv.host_array(ctypes.c_int64, [96, 96, 333])), dict(cut=nv.host_array(ctypes.c_int64, [0, 200, 333])),
               dict(dims=nv.host_array(ctypes.c_int32, [64, 0])), dict(w_dtype=2), dict(x_dtype=1),
               dict(proj=nv.host_array(ctypes.c_void_p, [4096, None])), dict(tables=nv.host_array(ctypes.c_void_p, [4096 + 8, 4096])),
               dict(x=odd), dict(head=odd), dict(ws=odd), dict(targets=odd), dict(token=odd), dict(logp=ctypes.c_void_p(4098)),
               dict(x_dtype=0, ldx=132), dict(ws_bytes=64)):
        assert call(**kw) == BAD, kw
    for kw in (dict(M=65), dict(C=144, ldx=144), dict(dims=nv.host_array(ctypes.c_int32, [64, 40])),
               dict(n=5, cut=nv.host_array(ctypes.c_int64, [1, 2, 3, 4, 5, 6]), dims=nv.host_array(ctypes.c_int32, [32] * 5),
                    proj=nv.host_array(ctypes.c_void_p, [4096] * 5), tables=nv.host_array(ctypes.c_void_p, [4096] * 5)),
               dict(cut=nv.host_array(ctypes.c_int64, [96, 200, 2 ** 31]))):
        assert call(**kw) == UNS, kw
    assert call(targets=None, ws_bytes=64) == BAD                    # (targets are optional; the workspace is not)


def _golden_operands():
    d, sd = _small_state()
    head = torch.cat([sd["embed_tokens.embeddings.0.0.weight"], sd["adaptive_softmax.head.class_proj.weight"]]).numpy()
    projs = [sd["embed_tokens.embeddings.%d.1.weight" % i].numpy().T for i in (1, 2)]
    tabs = [sd["embed_tokens.embeddings.%d.0.weight" % i].numpy() for i in (1, 2)]
    return d, head, projs, tabs


def test_p0_the_host_reference_equals_the_references_arrays():
    d, head, projs, tabs = _golden_operands()
    cut = [96, 200, 333]
    x = d["x"].reshape(48, 128)
    full = d["logp_full"].reshape(48, 333)
    ref = pref.pick(x, head, projs, tabs, cut)
    assert ref["token"].dtype == np.int64 and ref["token"].tolist() == full.argmax(-1).tolist()
    np.testing.assert_allclose(ref["logp"], full.max(-1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ref["joint"], full, rtol=1e-5, atol=1e-6)
    t = d["targets"].reshape(-1)
    with_t = pref.pick(x, head, projs, tabs, cut, t)
    assert with_t["token"].tolist() == ref["token"].tolist()
    np.testing.assert_allclose(with_t["logp"], d["logp_targets"].reshape(-1), rtol=1e-5, atol=1e-6)
    bad = t.copy()
    bad[0], bad[5] = -1, 333
    got = pref.pick(x, head, projs, tabs, cut, bad)["logp"]
    assert np.isnan(got[0]) and np.isnan(got[5]) and np.isnan(got).sum() == 2
    # equal scores go to the lower token: a duplicated table row
    tabs2 = [tabs[0].copy(), tabs[1].copy()]
    tabs2[1][7] = tabs2[1][90]
    j = pref.pick(x, head, projs, tabs2, cut)["joint"]
    assert (j[:, 200 + 7] == j[:, 200 + 90]).all()
    token, gap, ok = pref.decided(ref["joint"], np.full(48, 1e-6))
    assert token.tolist() == ref["token"].tolist() and (gap >= 0).all() and ok.dtype == bool


def _state(dtype):
    """A decoding state's shell (the attention's own states need a device; nothing here reads them)."""
    from ea_harness import sequence as sq
    return sq.DecodingState({}, None, dict(batch_size=2, max_tokens=16, dtype=dtype, device="cpu"))


def test_p0_stack_errors():
    from ea_harness import sequence as sq
    plain = sq.DecoderStack(333, 128, 256, 2, 1, ATTN).eval()
    stack = sq.DecoderStack(333, 128, 256, 2, 1, ATTN, adaptive=dict(cutoff=[96, 200], factor=2)).eval()
    with pytest.raises(RuntimeError, match="adaptive=dict"):
        plain.init_adaptive_decoding(_state(torch.bfloat16))
    with pytest.raises(ValueError, match="16-bit tables"):
        stack.init_adaptive_decoding(_state(torch.float32))
    with pytest.raises(NotImplementedError, match="adaptive.*init_adaptive_decoding"):
        stack.init_decoding(2, 16, torch.bfloat16, "cpu", hold_vocab=True)
    state = _state(torch.bfloat16)
    assert state.adaptive is None
    with pytest.raises(ValueError, match="state's dtype"):
        stack.init_adaptive_decoding(state, stack.adaptive_tables(torch.float16, "cpu"))
    assert stack.init_adaptive_decoding(state) is state
    ad = state.adaptive
    assert isinstance(ad, sq.AdaptivePick) and isinstance(ad.tables, sq.AdaptiveTables) and ad.tables.dtype == torch.bfloat16
    assert ad.ws.numel() == pref.ws_layout(64, [96, 200, 333], [64, 32])["total"] and ad.ws.dtype == torch.uint8
    assert tuple(ad.logp.shape) == (2,) and ad.logp.dtype == torch.float32
    # the projections are the row blocks of one buffer: one launch forms every h_i
    tb = ad.tables
    assert tb.proj[1].data_ptr() == tb.proj[0].data_ptr() + 64 * 128 * 2 and all(p.is_contiguous() for p in tb.proj)
    assert tuple(tb.proj_all.shape) == (96, 128)
    assert torch.equal(tb.proj[1].float(), stack.adaptive_softmax.tail_projection(1).detach().to(torch.bfloat16).float())
    rows = torch.zeros(1, 2, 128)
    with pytest.raises(ValueError, match="return_logits"):
        stack.next_tokens(rows, state, return_logits=True)
    with pytest.raises(ValueError, match="return_lse"):
        stack.token_logprobs(rows, state, return_lse=True)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):                # (a missing device is an error, never a fall-back)
        stack.next_tokens(rows, state)
