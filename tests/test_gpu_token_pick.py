"""-m gpu: the parts every decoding mode of ea_harness.sequence.DecoderStack shares (ea_harness/token_pick.py): the one
decoding loop of `generate` and `beam_search`, the pick selected for a state, and the lifecycle of what a state carries.

Stack: vocab 333 (a partial 16-column tile), embed 128, ffn 256, 2 heads, ONE layer, window 16, chunks of 4; the adaptive
modes on adaptive=dict(cutoff=[96, 200], factor=2).  bf16, B = 3, a prompt of 5 tokens (the per-sequence case: row 1 holds 3
and is right-padded), 4 new tokens.

 1. generate equals its public steps: for every mode (plain, held greedy, sampled, greedy with log-probability, sampled with
    log-probability, adaptive, adaptive with log-probability) on a rolling, a static and a ragged per-sequence state,
    generate(graph=True), generate(graph=False) and a loop written here from public calls alone -- `decode`, then
    `next_tokens` / `sample_tokens` / `token_logprobs` / `sample_tokens_logprobs` (plain: `logits(..).argmax(-1)`) with out=
    the static input -- give the same tokens, rows and log-probabilities bit for bit.
 2. the launches are the mode's own: one generate(graph=True, n_new=4) issues its pick entry exactly three times (the first
    pick, the warm-up, the capture) and no other pick entry, the plain mode none; beam_search(graph=True, max_new=4) issues
    ea_ceva_sdecode_vocab_beam three times.
 3. lifecycle: on a state with a sampler and a scorer a reorder permutes (ctr, sid), a row reset gives the row counter 0 and
    a stream id no row has had, the scorer's buffers stay where they are, and decoding_state_nbytes is the sum its docstring
    states; the bytes of a beam state and of an adaptive state likewise."""
import functools
import warnings

import pytest
import torch

import test_gpu_decoder_vocab as tv
from ceva_decoding import _ctx

_bits = tv._bits
V, C, FFN, HEADS, LAYERS, B, P, N_NEW = 333, 128, 256, 2, 1, 3, 5, 4
ADAPTIVE = dict(cutoff=[96, 200], factor=2)
DTYPE = torch.bfloat16
SAMPLING = dict(seed=5, top_k=8, top_p=0.9, temperature=1.0)
ENTRY = {"plain": None, "held": "ea_ceva_sdecode_vocab_argmax", "sampled": "ea_ceva_sdecode_vocab_sample",
         "greedy_logprob": "ea_ceva_sdecode_vocab_logprob", "sampled_logprob": "ea_ceva_sdecode_vocab_sample_logprob",
         "adaptive": "ea_adaptive_pick", "adaptive_logprob": "ea_adaptive_pick"}
BEAM_ENTRY = "ea_ceva_sdecode_vocab_beam"
MODES = list(ENTRY)
KINDS = ["rolling", "static", "per_sequence_ragged"]


@functools.lru_cache(maxsize=None)
def _stack(adaptive):
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(13)
    m = DecoderStack(V, C, FFN, HEADS, LAYERS, tv.ATTN, **(dict(adaptive=ADAPTIVE) if adaptive else {})).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        for layer in m.layers:
            layer.self_attn.rel_pos_bias.relative_attention_bias.weight.mul_(20.0)
        if not adaptive:
            m.embed_tokens.weight.mul_(1.0 / 32)                             # (tests/test_gpu_decoder_vocab.py's _stack)
    return m.eval()


def _prompt(m, kind):
    g = torch.Generator().manual_seed(17)
    prompt = torch.randint(2, V, (B, P), generator=g).cuda()
    if kind == "per_sequence_ragged":
        prompt[1, 3:] = m.pad_idx
    return prompt


def _state(m, mode, kind, batch=B):
    opt = dict(rolling=kind != "static", per_sequence=kind == "per_sequence_ragged")
    if mode.startswith("adaptive"):
        return m.init_adaptive_decoding(m.init_decoding(batch, P + N_NEW, DTYPE, "cuda", **opt))
    st = m.init_decoding(batch, P + N_NEW, DTYPE, "cuda", hold_vocab=mode != "plain", **opt)
    if mode.startswith("sampled"):
        m.init_sampling(st, **SAMPLING)
    if mode.endswith("logprob"):
        m.init_logprobs(st)
    return st


def _public_pick(m, mode, rows, st, out):
    """One pick by the public method of the mode -> (tokens [1, B], logp [1, B] or None)."""
    if mode == "plain":
        tokens = m.logits(rows).argmax(-1)
        return (tokens if out is None else out.copy_(tokens)), None
    if mode in ("held", "adaptive"):
        return m.next_tokens(rows, st, out=out), None
    if mode == "sampled":
        return m.sample_tokens(rows, st, out=out), None
    if mode == "sampled_logprob":
        return m.sample_tokens_logprobs(rows, st, out=out)
    return m.token_logprobs(rows, st, out=out)


def _public_loop(m, mode, kind, prompt):
    """What generate documents, written from public calls -> (tokens [B, n_new], rows [n_new, B, C], logp [B, n_new] or None)."""
    st = _state(m, mode, kind)
    with torch.no_grad():
        if kind == "per_sequence_ragged":
            x = m.decode(prompt.t(), st, prompt.eq(m.pad_idx))
            n_b = prompt.ne(m.pad_idx).sum(1)                                # (right-padded: the count of a row's own tokens)
            last = x[n_b - 1, torch.arange(B, device="cuda")].unsqueeze(0)
        else:
            last = m.decode(prompt.t(), st)[-1:]
        tok_in, lp = _public_pick(m, mode, last, st, None)
        tokens, rows, logps = [tok_in[0].clone()], [last[0].clone()], [None if lp is None else lp[0].clone()]
        for _ in range(1, N_NEW):
            y = m.decode(tok_in, st)
            _, lp = _public_pick(m, mode, y, st, tok_in)
            tokens.append(tok_in[0].clone()), rows.append(y[0].clone()), logps.append(None if lp is None else lp[0].clone())
    return torch.stack(tokens, 1), torch.stack(rows, 0), (None if logps[0] is None else torch.stack(logps, 1))


# ---- 1. generate equals its public steps ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_generate_replayed_eager_and_the_public_steps_agree_bit_for_bit(mode, kind):
    m = _stack(mode.startswith("adaptive"))
    prompt = _prompt(m, kind)
    with_lp = mode.endswith("logprob")
    with _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = {}
        for graph in (True, False):
            st = _state(m, mode, kind)
            got[graph] = m.generate(prompt, N_NEW, st, graph=graph, return_rows=True, return_logprobs=with_lp)
            if mode.startswith("sampled"):                                   # (the warm-up's draw is undone)
                assert st.sampler.ctr.tolist() == [N_NEW] * B
        want = _public_loop(m, mode, kind, prompt)
        torch.cuda.synchronize()
    assert tuple(want[0].shape) == (B, N_NEW) and tuple(want[1].shape) == (N_NEW, B, C)
    for graph in (True, False):
        assert len(got[graph]) == (3 if with_lp else 2)
        assert torch.equal(got[graph][0], want[0]), (graph, got[graph][0].tolist(), want[0].tolist())
        assert _bits(got[graph][1], want[1]), graph
        if with_lp:
            assert got[graph][2].dtype == torch.float32 and _bits(got[graph][2], want[2]), graph
            assert torch.isfinite(want[2]).all() and (want[2] <= 0).all()
    assert int(want[0].min()) >= 0 and int(want[0].max()) < V
    print(mode, kind, "tokens", want[0].tolist())


# ---- 2. the launches are the mode's own ---------------------------------------------------------------------------------------------
class _PickCalls:
    """The names of the pick entries `nv.call` is handed inside the block, in order."""

    def __enter__(self):
        from efficient_attention import _native as nv
        self.nv, self.real, self.names = nv, nv.call, []
        picks = set(filter(None, ENTRY.values())) | {BEAM_ENTRY}

        def call(name, *a):
            if name in picks:
                self.names.append(name)
            return self.real(name, *a)
        nv.call = call
        return self

    def __exit__(self, *exc):
        self.nv.call = self.real


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_generate_issues_the_pick_entry_of_its_mode_three_times_and_no_other(mode):
    m = _stack(mode.startswith("adaptive"))
    prompt = _prompt(m, "rolling")
    with _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _state(m, mode, "rolling")
        with _PickCalls() as calls:
            m.generate(prompt, N_NEW, st, graph=True, return_logprobs=mode.endswith("logprob"))
        torch.cuda.synchronize()
    assert calls.names == ([] if ENTRY[mode] is None else [ENTRY[mode]] * 3), calls.names


@pytest.mark.gpu
def test_beam_search_issues_the_beam_entry_three_times():
    m = _stack(False)
    W = 2
    with _ctx(DTYPE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = _state(m, "held", "rolling", batch=B * W)
        with _PickCalls() as calls:
            hyps = m.beam_search(_prompt(m, "rolling"), st, beam_size=W, eos_idx=2, max_new=N_NEW, graph=True)
        torch.cuda.synchronize()
    assert calls.names == [BEAM_ENTRY] * 3, calls.names
    assert len(hyps) == B and st.beam.replays == N_NEW - 1


# ---- 3. the lifecycle of what a state carries ---------------------------------------------------------------------------------------
def _nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


@pytest.mark.gpu
def test_reorder_reset_and_bytes_of_a_state_with_a_sampler_and_a_scorer():
    m = _stack(False)
    tiles = (V + 15) // 16
    with _ctx(DTYPE):
        bare = m.decoding_state_nbytes(m.init_decoding(B, P + N_NEW, DTYPE, "cuda", per_sequence=True))
        st = _state(m, "sampled_logprob", "per_sequence_ragged")             # (a row reset needs per-sequence counts)
    sm, sc = st.sampler, st.scorer
    held = 2 * V * C + 8 * 64 * tiles
    assert m.decoding_state_nbytes(st) == bare + held + (4 * B * V + 8 * B + 4 * B) + (4 * 64 * (tiles + 1) + 8 * B)
    ptrs = [t.data_ptr() for t in (sc.ws, sc.lse, sc.logp, sm.logits, sm.ctr, sm.sid)]
    sm.ctr.copy_(torch.tensor([5, 6, 7], device="cuda"))
    assert m.reorder_decoding_state(st, torch.tensor([2, 0, 1], device="cuda")) is st
    assert sm.ctr.tolist() == [7, 5, 6] and sm.sid.tolist() == [2, 0, 1]     # a row takes its stream along
    assert m.reset_decoding_rows(st, [1]) is st
    assert sm.ctr.tolist() == [7, 0, 6] and sm.sid.tolist() == [2, B, 1] and sm.next_sid == B + 1
    assert sm.ctr.dtype == torch.long and sm.sid.dtype == torch.int32
    assert ptrs == [t.data_ptr() for t in (sc.ws, sc.lse, sc.logp, sm.logits, sm.ctr, sm.sid)]
    assert m.refresh_decoding_weights(st) is st and ptrs[0] == sc.ws.data_ptr()
    assert torch.equal(st.vocab, m.embed_tokens.weight.detach().to(DTYPE))


@pytest.mark.gpu
def test_bytes_of_a_beam_state_and_of_an_adaptive_state():
    from efficient_attention import _native as nv
    m, W, max_new = _stack(False), 2, 7
    M, S, tiles = B * W, B, (V + 15) // 16
    with _ctx(DTYPE):
        bare = m.decoding_state_nbytes(m.init_decoding(M, P + N_NEW, DTYPE, "cuda"))
        st = m.init_beam_search(_state(m, "held", "rolling", batch=M), W, 2, max_new)
    beam = 4 * M * V + nv.lib().ea_ceva_sdecode_vocab_beam_ws(M, V, W) + 4 * M + 12 * S + 8 * M + 8 * max_new * M + 12 * S * W
    assert m.decoding_state_nbytes(st) == bare + 2 * V * C + 8 * 64 * tiles + beam
    assert beam == _nbytes(*st.beam.buffers())

    a = _stack(True)
    with _ctx(DTYPE):
        bare = a.decoding_state_nbytes(a.init_decoding(B, P + N_NEW, DTYPE, "cuda"))
        st = _state(a, "adaptive", "rolling")
    cut, dims = ADAPTIVE["cutoff"] + [V], [C // 2, C // 4]
    tables = 2 * ((cut[0] + 2) * C + sum(d * C + (cut[i + 1] - cut[i]) * d for i, d in enumerate(dims)))
    assert st.adaptive.tables.cutoff == cut and st.adaptive.tables.dims == dims and st.adaptive.tables.nbytes() == tables
    assert a.decoding_state_nbytes(st) == bare + tables + st.adaptive.ws.numel() + 4 * B
