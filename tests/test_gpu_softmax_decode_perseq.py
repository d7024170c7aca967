"""-m gpu: per-sequence token counts in causal softmax decoding (the _seq entries of csrc/ea_softmax_decode.hip): each row against
test_gpu_softmax_decode.py's fp64 restatement and bound with its own (t0_b, n_b), every live row compared, and bit for bit against
the row decoded alone on a shared-count B = 1 state; the step protocol with one overflowing row; the module; a softmax stack."""
import ctypes

import pytest
import torch

import test_gpu_softmax_decode as base

pytestmark = pytest.mark.gpu
B, H = 3, 2
# (d, T, t0[3], n[3], parts): an idle row beside working ones; n < T with the causal edge across a tile boundary; an empty cache
# beside several tiles (parts and waves without a tile of the short row); parts 1, not dividing the tiles, more than a row's tiles
SPLIT = [(64, 4, (62, 0, 300), (3, 0, 4), 1), (128, 1, (0, 700, 64), (1, 1, 0), 3), (32, 8, (250, 0, 130), (8, 1, 5), 5),
         (128, 2, (63, 127, 0), (2, 1, 2), 64)]
# (d, T, t0[3], n[3]): a second block for one row only, a row ending mid-wave, an idle row; 16 rows; d 32 / 128 at odd offsets
MM = [(64, 70, (0, 130, 5), (70, 9, 0)), (64, 16, (0, 63, 250), (16, 1, 16)), (32, 37, (61, 3, 77), (37, 20, 17)),
      (128, 66, (250, 1, 129), (65, 66, 33))]
ids = lambda cases: ["d%d_T%d_%s" % (c[0], c[1], "-".join(map(str, c[3]))) for c in cases]      # noqa: E731


def _launch(nv, dtype, rows_d, kv_d, pad_d, out, pos, ntok, parts, append=False, advance=False):
    """A step's launches: ntok None = the shared-count entries, else the _seq ones -> (pos, status, ntok) device tensors."""
    T, nb, d, cap = rows_d.shape[0], kv_d.shape[0], kv_d.shape[-1], kv_d.shape[3]
    pos_d, status = torch.tensor(pos, dtype=torch.int32, device="cuda"), torch.zeros(len(pos), dtype=torch.int32, device="cuda")
    ntok_d = None if ntok is None else torch.as_tensor(ntok, dtype=torch.int32).cuda()
    sfx, tail = ("", ()) if ntok is None else ("_seq", (nv.ptr(ntok_d),))
    io = nv.EA_BF16 if dtype == torch.bfloat16 else nv.EA_F16
    geom = nv.ea_softmax_sdec_geom(nb, H, d, io, T, cap, pos_d.data_ptr(), status.data_ptr())
    g, st = ctypes.byref(geom), nv.stream()
    tq, tk, tv, to = [nv.t4(t) for t in (rows_d[:, :, 0].permute(1, 2, 0, 3), kv_d[:, 0], kv_d[:, 1], out[:, :, :T])]
    views = [ctypes.byref(t) for t in (tq, tk, tv)] + [nv.ptr(pad_d), ctypes.byref(to)]
    if append is not False:
        nv.call("ea_softmax_sdecode_append" + sfx, g, nv.ptr(rows_d), nv.ptr(append), views[1], views[2], nv.ptr(pad_d), *tail, st)
    if parts is None:
        nv.call("ea_softmax_sdecode_attn_mm" + sfx, g, *views, *tail, st)
    else:
        ws = torch.full((nb, H, 8, parts, d + 4), float("nan"), device="cuda") if parts > 1 else None
        nv.call("ea_softmax_sdecode_attn_split" + sfx, g, *views, parts, nv.ptr(ws), *tail, st)
        if parts > 1:
            nv.call("ea_softmax_sdecode_merge" + sfx, g, views[4], parts, nv.ptr(ws), *tail, st)
    if advance:
        nv.call("ea_softmax_sdecode_advance" + sfx, g, *tail, st)
    torch.cuda.synchronize()
    return pos_d, status, ntok_d


def _check_rows(got, rows, kv, dtype, t0, n, parts, T):
    """out [B, H, T + 2, d] against fp64 row by row: live rows inside the bound, rows n_b .. T - 1 zero, guard rows untouched."""
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    nopad = torch.zeros(1, kv.shape[3], dtype=torch.bool)
    assert (got[:, :, T:] == 7.0).all()
    for b in range(B):
        assert (got[b, :, n[b]:T] == 0).all()
        if n[b]:
            ref, wabs, _, vmax = base._ref(rows[:n[b], b:b + 1], kv[b:b + 1], nopad, t0[b], n[b], dtype, parts is None)
            bound = u * (ref.abs() + wabs) + 1e-6 * ref.abs().max() + ((t0[b] + n[b]) * 2.0 ** -24 * vmax if dtype == torch.float16 else 0.0)
            err = (got[b:b + 1, :, :n[b]] - ref).abs()
            print((t0[b], n[b], parts), dtype, "row %d max |d| / bound %.3f" % (b, (err / bound).max().item()))
            assert bool(torch.isfinite(err).all()) and (err - bound).max().item() <= 0


def _operands(dtype, d, T, t0, extra=5):
    g = torch.Generator().manual_seed(d + T + sum(t0))
    cap = max(t0) + T + extra
    return torch.randn(B, 2, H, cap, d, generator=g).to(dtype), torch.randn(T, B, 3, H, d, generator=g).to(dtype), cap


@pytest.mark.parametrize("dtype", base.DT16, ids=base.IDS16)
@pytest.mark.parametrize("case", [c + (None,) for c in MM] + SPLIT, ids=ids(MM) + ids(SPLIT))
def test_seq_kernels_against_fp64_and_the_row_alone(dtype, case):
    from efficient_attention import _native as nv
    d, T, t0, n, parts = case
    kv, rows, cap = _operands(dtype, d, T, t0)
    kv_d, rows_d, pad_d = kv.cuda(), rows.cuda(), torch.zeros(B, cap, dtype=torch.uint8, device="cuda")
    out = torch.full((B, H, T + 2, d), 7.0, dtype=dtype, device="cuda")
    _launch(nv, dtype, rows_d, kv_d, pad_d, out, t0, n, parts)
    _check_rows(out.double().cpu(), rows, kv, dtype, t0, n, parts, T)
    if case in (MM[0] + (None,), SPLIT[2]) and dtype == torch.bfloat16:        # a row is what it is alone: B = 1, T = n_b
        for b in [b for b in range(B) if n[b]]:
            alone = torch.zeros((1, H, n[b], d), dtype=dtype, device="cuda")
            _launch(nv, dtype, rows_d[:n[b], b:b + 1].contiguous(), kv_d[b:b + 1], pad_d[b:b + 1], alone, [t0[b]], None, parts)
            assert torch.equal(out[b, :, :n[b]], alone[0])


@pytest.mark.parametrize("T,parts", [(3, 2), (20, None)], ids=["split", "mm"])
def test_seq_step_protocol_one_row_overflows(T, parts):
    from efficient_attention import _native as nv
    dtype, d, cap = torch.bfloat16, 64, 80
    t0, n = (5, cap - T + 1, 30), (2, T, 1)                        # row 1 alone passes cap, by one token
    kv, rows, _ = _operands(dtype, d, T, (cap - T - 5,) * 3)
    step_pad = torch.zeros(B, T, dtype=torch.uint8)
    step_pad[0, 2], step_pad[2, 1:] = 1, 1
    kv_d, rows_d, pad_d = kv.cuda(), rows.cuda(), torch.zeros(B, cap, dtype=torch.uint8, device="cuda")
    for b in range(B):
        pad_d[b, t0[b]:] = 1                                       # (stale flags behind the counts: append must clear its rows')
    want_kv, want_pad = kv_d.clone(), pad_d.clone()
    for b in (0, 2):
        want_kv[b, :, :, t0[b]:t0[b] + n[b]] = rows_d[:n[b], b, 1:].permute(1, 2, 0, 3)
        want_pad[b, t0[b]:t0[b] + n[b]] = 0
    out = torch.full((B, H, T + 2, d), 7.0, dtype=dtype, device="cuda")
    pos, status, ntok = _launch(nv, dtype, rows_d, kv_d, pad_d, out, t0, [9, 9, 9], parts, append=step_pad.cuda(), advance=True)
    assert torch.equal(kv_d, want_kv) and torch.equal(pad_d, want_pad)       # row 1: no byte; rows 0, 2: their n_b rows only
    assert status.tolist() == [0, 1, 0] and ntok.tolist() == list(n) and pos.tolist() == [t0[0] + n[0], t0[1], t0[2] + n[2]]
    got = out.double().cpu()
    assert bool(torch.isnan(got[1, :, :T]).all())
    got[1, :, :T] = 0
    _check_rows(got, rows, kv_d.cpu(), dtype, t0, (n[0], 0, n[2]), parts, T)


def _steps(m, st, x, flags, lens):
    pad = torch.arange(x.shape[0], device="cuda")[None, :] >= torch.tensor(lens, device="cuda")[:, None]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        y = m(x, x, x, key_padding_mask=pad if flags else None, incremental_state=st)[0]
    return [y[:n, b].clone() for b, n in enumerate(lens)]


def test_seq_module_rows_equal_the_rows_decoded_alone():
    import efficient_attention as ea
    torch.manual_seed(7)
    m = ea.CausalSoftmaxAttention(128, 2).cuda().eval()
    make = lambda nb, seq: m.init_kv_cache({}, nb, 64, torch.bfloat16, "cuda", kv_splits=3, hold_projections=True, per_sequence=seq)  # noqa: E731
    st, solo = make(B, True), [make(1, False) for _ in range(B)]
    # (T, the rows' token counts): a ragged prefill; single tokens with row 2 idle on some; after the reset, a new prompt on row 1
    plan = [(20, (20, 9, 13))] + [(1, (1, 1, i % 2)) for i in range(5)] + ["reset", (5, (1, 5, 1)), (1, (1, 1, 1)), "reorder", (1, (1, 1, 1))]
    xin, pin, graph, want = torch.zeros(1, B, 128, device="cuda"), torch.zeros(B, 1, dtype=torch.bool, device="cuda"), None, [0] * B
    _steps(m, make(B, True), xin, False, [1] * B)                  # (the single-token launches once before they are captured)
    for item in plan:
        if item == "reset":
            m.reset_decoding_rows(st, [1])
            m.reset_decoding_rows(solo[1], [0])
            want[1] = 0
            continue
        if item == "reorder":
            order = [2, 0, 1]
            m.reorder_incremental_state(st, torch.tensor(order, device="cuda"))
            solo, want = [solo[i] for i in order], [want[i] for i in order]
            continue
        T, lens = item
        x = torch.randn(T, B, 128, device="cuda")
        if T > 1:
            got = _steps(m, st, x, True, lens)
        else:                                                      # one captured step, replayed with the row's flags
            xin.copy_(x)
            pin.copy_(torch.tensor(lens, device="cuda")[:, None] == 0)
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False), torch.cuda.graph(graph):
                    yout = m(xin, xin, xin, key_padding_mask=pin, incremental_state=st)[0]
            graph.replay()
            got = [yout[:n, b].clone() for b, n in enumerate(lens)]
        for b, n in enumerate(lens):
            want[b] += n
            if n:
                assert torch.equal(got[b], _steps(m, solo[b], x[:n, b:b + 1].contiguous(), False, [n])[0]), (item, b)
        assert m.decoding_positions(st).tolist() == want and not m.static_decoding_overflowed(st)


def test_seq_stack_generates_and_scores_ragged_rows():
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(11)
    stack = DecoderStack(97, 128, 256, 2, 2, dropout=0.0, attn_name="softmax").cuda().eval()
    lens, short = (12, 9, 10), (8, 4, 6)                           # prompts (all on attn_mm, alone too); scored rows (attn_split)
    prompt = torch.randint(2, 97, (B, 12), device="cuda")
    scored = prompt[:, :8].clone()
    for b in range(B):
        prompt[b, lens[b]:], scored[b, short[b]:] = stack.pad_idx, stack.pad_idx
    make = lambda nb, cap, seq, **kw: stack.init_kv_decoding(nb, cap, torch.bfloat16, "cuda", kv_splits=2, per_sequence=seq, **kw)  # noqa: E731
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert make(B, 24, True).options["per_sequence"] is True
        eager = stack.generate(prompt, 12, state=make(B, 24, True), graph=False)
        assert torch.equal(stack.generate(prompt, 12, state=make(B, 24, True), graph=True), eager)
        logp = stack.score(scored, stack.init_logprobs(make(B, 7, True, hold_vocab=True)))
        for b in range(B):
            assert torch.equal(stack.generate(prompt[b:b + 1, :lens[b]], 12, state=make(1, 24, False), graph=False), eager[b:b + 1])
            alone = stack.score(scored[b:b + 1, :short[b]], stack.init_logprobs(make(1, 7, False, hold_vocab=True)))
            assert torch.equal(alone[0], logp[b, :short[b] - 1]) and bool((logp[b, short[b] - 1:] == 0).all())
