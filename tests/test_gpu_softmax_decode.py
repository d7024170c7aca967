"""-m gpu: KV-cache decoding of causal softmax attention (csrc/ea_softmax_decode.hip).

The two attention kernels against an fp64 restatement on the same 16-bit operands, inside the bound DESIGN.md 4a derives (a CPU
model of the roundings must stay inside it first); the step protocol; the module against the fp64 module of
test_gpu_causal_softmax_module.py, captured steps and reorders; a softmax DecoderStack decoding, generating and searching."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

import test_gpu_causal_softmax_module as full       # noqa: E402

pytestmark = pytest.mark.gpu
DT16, IDS16 = [torch.bfloat16, torch.float16], ["bf16", "fp16"]
B = H = 2
# (d, t0, T, parts): one key, a part with no tile; exactly one tile, no merge; first key of a second tile; eight queries whose
# causal edge crosses the tile boundary at 256, parts that do not divide the tiles; more parts than tiles; several tiles per wave
SPLIT = [(64, 0, 1, 2), (128, 63, 1, 1), (128, 64, 1, 4), (32, 250, 8, 3), (128, 700, 3, 64), (64, 1100, 2, 2)]
# (d, t0, T): the smallest 16-token step from an empty cache; the smallest step routed here, ragged, offset % 16 != 0; d = 32 at a
# non-aligned offset; prefill with a ragged last block; two workgroups, diagonal tiles at a non-aligned offset
MM = [(64, 0, 16), (64, 130, 9), (32, 60, 37), (128, 0, 150), (128, 250, 70)]


def _operands(dtype, d, t0, T, extra=5):
    """A cache that already holds the step's rows, and the step's projection buffer: row 1 starts with three padded keys."""
    g = torch.Generator().manual_seed(3 * t0 + d + T)
    cap = t0 + T + extra                                           # (no multiple of the tile)
    kv = torch.randn(B, 2, H, cap, d, generator=g).to(dtype)
    rows = torch.randn(T, B, 3, H, d, generator=g).to(dtype)
    pad = torch.zeros(B, cap, dtype=torch.bool)
    pad[1, :3] = True
    return kv, rows, pad, cap


def _ref(rows, kv, pad, t0, T, dtype, round_p):
    """softmax(scale q k^T, -inf after the query and on padded keys) v in fp64 -> (ref, sum_j p_j |v_j|, the rounding model:
    P rounded to the dtype where the kernel rounds it, the output rounded once)."""
    n, d = t0 + T, kv.shape[-1]
    q = rows[:, :, 0].permute(1, 2, 0, 3).double()
    k, v = kv[:, 0, :, :n].double(), kv[:, 1, :, :n].double()
    dead = (torch.arange(n)[None, :] > t0 + torch.arange(T)[:, None])[None, None] | pad[:, None, None, :n]
    p = torch.softmax((d ** -0.5 * q @ k.transpose(-1, -2)).masked_fill(dead, float("-inf")), -1)
    model = ((p.to(dtype).double() if round_p else p) @ v).to(dtype).double()
    return p @ v, p @ v.abs(), model, v.abs().max().item()


def _geom(nv, dtype, d, T, cap, t0):
    pos, status = [torch.tensor([v], dtype=torch.int32, device="cuda") for v in (t0, 0)]
    io = nv.EA_BF16 if dtype == torch.bfloat16 else nv.EA_F16
    return nv.ea_softmax_sdec_geom(B, H, d, io, T, cap, pos.data_ptr(), status.data_ptr()), pos, status


def _attn(nv, geom, rows_d, kv_d, pad_d, out, T, parts):
    """The attention launches of a step, as the module issues them."""
    tq, tk, tv, to = [nv.t4(t) for t in (rows_d[:, :, 0].permute(1, 2, 0, 3), kv_d[:, 0], kv_d[:, 1], out[:, :, :T])]
    g, views = ctypes.byref(geom), [ctypes.byref(t) for t in (tq, tk, tv)] + [nv.ptr(pad_d), ctypes.byref(to)]
    if parts is None:
        return nv.call("ea_softmax_sdecode_attn_mm", g, *views, nv.stream())
    ws = torch.full((B, H, 8, parts, kv_d.shape[-1] + 4), float("nan"), device="cuda") if parts > 1 else None
    nv.call("ea_softmax_sdecode_attn_split", g, *views, parts, nv.ptr(ws), nv.stream())
    if parts > 1:
        nv.call("ea_softmax_sdecode_merge", g, views[4], parts, nv.ptr(ws), nv.stream())


def _check_kernel(dtype, d, t0, T, parts):
    from efficient_attention import _native as nv
    kv, rows, pad, cap = _operands(dtype, d, t0, T)
    ref, wabs, model, vmax = _ref(rows, kv, pad, t0, T, dtype, round_p=parts is None)
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    live = torch.isfinite(ref)                                     # (a query whose visible keys are all padded: NaN)
    bound = u * (ref.abs() + wabs) + 1e-6 * ref[live].abs().max() + ((t0 + T) * 2.0 ** -24 * vmax if dtype == torch.float16 else 0.0)
    use = ((model - ref).abs() / bound)[live].max().item()
    print((d, t0, T, parts), dtype, "rounding model uses %.3f of the bound" % use)
    assert use <= 1.0
    out = torch.full((B, H, T + 2, d), 7.0, dtype=dtype, device="cuda")          # two guard rows behind the step's
    geom, pos, status = _geom(nv, dtype, d, T, cap, t0)
    _attn(nv, geom, rows.cuda(), kv.cuda(), pad.to(torch.uint8).cuda(), out, T, parts)
    torch.cuda.synchronize()
    got = out.double().cpu()
    assert (got[:, :, T:] == 7.0).all() and (torch.isnan(got[:, :, :T]) == ~live).all()
    err = (got[:, :, :T] - ref).abs()
    print((d, t0, T, parts), dtype, "max |d| / bound %.3f" % (err / bound)[live].max().item())
    assert (err - bound)[live].max().item() <= 0


@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("case", SPLIT, ids=["d%d_t%d_T%d_P%d" % c for c in SPLIT])
def test_attn_split_kernel_against_fp64(dtype, case):
    _check_kernel(dtype, *case)


@pytest.mark.parametrize("dtype", DT16, ids=IDS16)
@pytest.mark.parametrize("case", MM, ids=["d%d_t%d_T%d" % c for c in MM])
def test_attn_mm_kernel_against_fp64(dtype, case):
    _check_kernel(dtype, *case, None)


@pytest.mark.parametrize("T,parts", [(3, 2), (20, None)], ids=["split", "mm"])
def test_step_protocol_fits_or_writes_nothing(T, parts):
    from efficient_attention import _native as nv
    dtype, d, t0 = torch.bfloat16, 64, 70
    kv, rows, pad, cap = _operands(dtype, d, t0, T)
    step_pad = torch.zeros(B, T, dtype=torch.uint8)
    step_pad[0, 1] = 1
    for room in (cap, t0 + T - 1):                                 # the step fits; it passes the capacity by one token
        kv_d, pad_d, rows_d = kv[:, :, :, :room].contiguous().cuda(), pad[:, :room].to(torch.uint8).cuda(), rows.cuda()
        before = (kv_d.clone(), pad_d.clone())
        out = torch.zeros((B, H, T, d), dtype=dtype, device="cuda")
        geom, pos, status = _geom(nv, dtype, d, T, room, t0)
        tk, tv = nv.t4(kv_d[:, 0]), nv.t4(kv_d[:, 1])
        nv.call("ea_softmax_sdecode_append", ctypes.byref(geom), nv.ptr(rows_d), nv.ptr(step_pad.cuda()), ctypes.byref(tk),
                ctypes.byref(tv), nv.ptr(pad_d), nv.stream())
        _attn(nv, geom, rows_d, kv_d, pad_d, out, T, parts)
        nv.call("ea_softmax_sdecode_advance", ctypes.byref(geom), nv.stream())
        if room == cap:
            want = rows_d[:, :, 1:].permute(1, 2, 3, 0, 4)          # [B, 2, h, T, d]
            assert torch.equal(kv_d[:, :, :, t0:t0 + T], want) and torch.equal(kv_d[:, :, :, :t0], before[0][:, :, :, :t0])
            assert torch.equal(pad_d[:, t0:t0 + T].cpu(), step_pad) and torch.equal(pad_d[:, :t0], before[1][:, :t0])
            assert pos.item() == t0 + T and status.item() == 0 and bool(torch.isfinite(out[0]).all())
        else:
            assert torch.equal(kv_d, before[0]) and torch.equal(pad_d, before[1])
            assert pos.item() == t0 and status.item() == 1 and bool(torch.isnan(out).all())


def _feed(m, x, pad, st, graph_from=None):
    """A prompt of 70 tokens, then single tokens, through the state -> rows [T, B, C]; graph_from: the single-token steps from
    that position on are one captured step replayed."""
    T = x.shape[0]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        xp = x[:70]
        ys = [m(xp, xp, xp, key_padding_mask=pad[:, :70], incremental_state=st)[0]]
        xin, pin, g = x[70:71].clone(), pad[:, 70:71].clone(), None
        for t in range(70, T):
            xin.copy_(x[t:t + 1])
            pin.copy_(pad[:, t:t + 1])
            if graph_from is not None and t == graph_from:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    y = m(xin, xin, xin, key_padding_mask=pin, incremental_state=st)[0]
            if g is not None:                                      # (a capture records the step and runs nothing)
                g.replay()
            else:
                y = m(xin, xin, xin, key_padding_mask=pin, incremental_state=st)[0]
            ys.append(y.clone())
    return torch.cat(ys, 0)


@pytest.mark.parametrize("C", [128, 256], ids=["d64", "d128"])
def test_module_decoding_matches_the_fp64_module(monkeypatch, C):
    import efficient_attention as ea
    T = 100
    monkeypatch.setattr(full, "T", T)
    torch.manual_seed(C)
    m = ea.CausalSoftmaxAttention(C, 2).cuda().eval()
    x = torch.randn(T, B, C, device="cuda")
    pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    pad[1, :4] = True                                              # left padding on one row
    ref = full._fp64_module(m, x, pad, 2)[0].detach()
    live = ~pad.t()                                                # [T, B]: a padded query of the left padding has no key
    rows = {}
    for splits, hold in [(1, False), (3, False), (3, True)]:
        st = {}
        m.init_kv_cache(st, B, T, torch.bfloat16, "cuda", kv_splits=splits, hold_projections=hold)
        got = rows[splits, hold] = _feed(m, x, pad, st)
        full._close(got[live], ref[live], "splits %d held %d" % (splits, hold))
        assert m.decoding_positions(st).tolist() == [T] * B and not m.static_decoding_overflowed(st)
        buf = m._get_input_buffer(st)
        assert m.decoding_state_nbytes(st) == sum(t.numel() * t.element_size() for t in buf.values() if t is not None)
    full._close(rows[3, True][live], rows[3, False][live].double(), "held against plain")
    # a captured step replayed: the outputs and the cache of the same steps run eagerly, bit for bit
    st2 = {}
    m.init_kv_cache(st2, B, T, torch.bfloat16, "cuda", kv_splits=3, hold_projections=True)
    again = _feed(m, x, pad, st2, graph_from=72)
    assert torch.equal(again[live], rows[3, True][live])
    assert all(torch.equal(m._get_input_buffer(st2)[k], buf[k]) for k in ("kv", "pad", "pos", "status"))


def test_reorder_permutes_later_outputs():
    import efficient_attention as ea
    torch.manual_seed(5)
    m = ea.CausalSoftmaxAttention(128, 2).cuda().eval()
    x = torch.randn(21, B, 128, device="cuda")
    sts = [{}, {}]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for st in sts:
            m.init_kv_cache(st, B, 32, torch.bfloat16, "cuda")
            m(x[:20], None, None, incremental_state=st)
        m.reorder_incremental_state(sts[1], torch.tensor([1, 0], device="cuda"))
        plain = m(x[20:], None, None, incremental_state=sts[0])[0]
        swapped = m(x[20:, [1, 0]], None, None, incremental_state=sts[1])[0]
    assert torch.equal(swapped, plain[:, [1, 0]])
    with pytest.raises(NotImplementedError, match="per-sequence"):
        m.reset_decoding_rows(sts[0], [1])
    m.reset_decoding_rows(sts[0], [0, 1])
    assert m.decoding_positions(sts[0]).tolist() == [0, 0]


def test_softmax_stack_decodes_generates_and_searches():
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(11)
    stack = DecoderStack(97, 128, 256, 2, 2, dropout=0.0, attn_name="softmax").cuda().eval()
    tokens = torch.randint(2, 97, (B, 41), device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = stack(tokens).double()
        state = stack.init_kv_decoding(B, 64, torch.bfloat16, "cuda", kv_splits=2)
        assert state.options["made_by"] == "init_kv_decoding"
        got = torch.cat([stack.decode(tokens[:, :40].t(), state), stack.decode(tokens[:, 40:].t(), state)], 0)
    full._close(got, ref, "decode against forward")
    held = [t for layer in state.ffn for t in layer]
    bufs = [t for layer in stack.layers for t in layer.self_attn._get_input_buffer(state.incremental).values() if t is not None]
    assert stack.decoding_state_nbytes(state) == sum(t.numel() * t.element_size() for t in held + bufs)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        eager = stack.generate(tokens[:, :9], 12, graph=False)
        assert torch.equal(stack.generate(tokens[:, :9], 12, graph=True), eager)
        beams = stack.init_kv_decoding(B * 3, 9 + 6, torch.bfloat16, "cuda", hold_vocab=True)
        hyps = stack.beam_search(tokens[:, :9], beams, beam_size=3, eos_idx=2, max_new=6)
    assert len(hyps) == B and all(sent and all(math.isfinite(h["score"]) for h in sent) for sent in hyps)
