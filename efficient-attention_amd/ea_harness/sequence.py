"""A fairseq-free Time x Batch x Channel encoder around AttentionFactory.build_attention.

TimeFirstSelfAttention is the adapter of fairseq/fairseq/modules/efficient_attention.py:43-132: it
builds the attention from (attn_name, attn_args) with dim / num_heads / qkv_bias / attn_drop / proj_drop
filled in, takes `query [T, B, C]` and `key_padding_mask [B, T]` (1 = pad), calls the module batch-first
and hands back `[T, B, C]`.  EncoderLayer is the post-norm residual layer of transformer_wmt_en_de
(self-attention, LayerNorm, ReLU feed-forward, LayerNorm).  Parameter names under `self_attn.attn.*`
are the attention module's own, as in the reference adapter.

DecoderLayer / DecoderStack are the decoder-only language model of the wikitext-103 recipe around `CausalEVAttention`
(fairseq/modules/transformer_layer.py:236-308 without the encoder attention), with incremental decoding on the attention's
static and rolling states: `init_decoding`, `decode`, `generate`; `next_tokens` is the greedy pick on a vocabulary table the
state holds (ea_ceva_sdecode_vocab_argmax), `init_sampling` / `sample_tokens` the sampled one (ea_ceva_sdecode_vocab_sample);
`init_logprobs` / `token_logprobs` / `sample_tokens_logprobs` / `score` report a token's log-probability under the model's own
distribution from the same pass over the table (ea_ceva_sdecode_vocab_logprob, ea_ceva_sdecode_vocab_sample_logprob);
`init_beam_search` / `set_beam_prompt` / `beam_step` / `beam_search` are a beam search whose step -- candidates, merge,
finished hypotheses, the parent index of the state reorder, and min_len, n-gram blocking and static bans where asked for --
runs on the device (ea_ceva_sdecode_vocab_beam, ea_ceva_sdecode_vocab_beam_c).  On an adaptive stack
`init_adaptive_decoding` makes a state pick greedily, with log-probabilities, from the held adaptive tables
(ea_adaptive_pick); on such a state `init_sampling` / `init_beam_search` sample and search from the adaptive head too
(ea_adaptive_sample, ea_adaptive_beam).

What the modes share lives in token_pick.py: the DecodingState and what the `init_*` methods attach to it, the operand
helpers, and one pick per launch.  Every public method above is its argument checks and that pick's `run`; `generate` and
`beam_search` are one prefill (`_prefill`) and one warm-up / capture / replay loop (`_run_steps`) around the pick
`select_pick` returns for the state, and the four lifecycle methods (`refresh_decoding_weights`, `reorder_decoding_state`,
`reset_decoding_rows`, `decoding_state_nbytes`) loop over `state.attachments()`."""
import argparse
import contextlib
import functools
import inspect
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from efficient_attention import AttentionFactory, CausalEVAttention

from . import token_pick as tp
from .token_pick import (AdaptivePick, AdaptiveTables, Beam, DecodingState, Sampler, Scorer,    # noqa: F401  (they lived here)
                         MAX_ROWS as _FUSED_MAX_ROWS)


class TimeFirstSelfAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, attn_name, attn_args=None):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        args = dict(attn_args or {})
        args.update(dim=embed_dim, num_heads=num_heads, qkv_bias=True, attn_drop=0.0, proj_drop=0.0)
        self.attn = AttentionFactory.build_attention(attn_name=attn_name, attn_args=args)

    def forward(self, query, key=None, value=None, key_padding_mask=None, attn_mask=None):
        T, B, C = query.shape
        assert C == self.embed_dim and attn_mask is None
        if key_padding_mask is not None:
            assert tuple(key_padding_mask.shape) == (B, T)
        out = self.attn(query.transpose(0, 1), key_padding_mask)            # [B, T, C]
        return out.transpose(0, 1).contiguous().view(T, B, C), None


class EncoderLayer(nn.Module):
    def __init__(self, embed_dim, ffn_dim, num_heads, attn_name, attn_args, dropout=0.1, normalize_before=False):
        super().__init__()
        self.self_attn = TimeFirstSelfAttention(embed_dim, num_heads, attn_name, attn_args)
        self.self_attn_layer_norm = nn.LayerNorm(embed_dim)
        self.fc1 = nn.Linear(embed_dim, ffn_dim)
        self.fc2 = nn.Linear(ffn_dim, embed_dim)
        self.final_layer_norm = nn.LayerNorm(embed_dim)
        self.dropout = nn.Dropout(dropout)
        self.normalize_before = normalize_before

    def forward(self, x, key_padding_mask=None):
        res = x
        if self.normalize_before:
            x = self.self_attn_layer_norm(x)
        x, _ = self.self_attn(x, x, x, key_padding_mask=key_padding_mask)
        x = res + self.dropout(x)
        if not self.normalize_before:
            x = self.self_attn_layer_norm(x)
        res = x
        if self.normalize_before:
            x = self.final_layer_norm(x)
        x = self.fc2(self.dropout(F.relu(self.fc1(x))))
        x = res + self.dropout(x)
        if not self.normalize_before:
            x = self.final_layer_norm(x)
        return x


class EncoderStack(nn.Module):
    """Token embedding (scaled) + sinusoidal positions -> `layers` EncoderLayers -> [T, B, C]; a tied
    output projection turns it into token logits so that a training step has a loss."""

    def __init__(self, vocab, embed_dim, ffn_dim, num_heads, layers, attn_name, attn_args=None, dropout=0.1,
                 max_positions=4096, pad_idx=1):
        super().__init__()
        self.embed_dim, self.pad_idx = embed_dim, pad_idx
        self.embed_tokens = nn.Embedding(vocab, embed_dim, padding_idx=pad_idx)
        nn.init.normal_(self.embed_tokens.weight, mean=0, std=embed_dim ** -0.5)
        nn.init.constant_(self.embed_tokens.weight[pad_idx], 0)
        self.register_buffer("positions", self._sinusoid(max_positions, embed_dim), persistent=False)
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.ModuleList([EncoderLayer(embed_dim, ffn_dim, num_heads, attn_name, attn_args, dropout)
                                     for _ in range(layers)])

    @staticmethod
    def _sinusoid(n, dim):
        half = dim // 2
        freq = torch.exp(torch.arange(half, dtype=torch.float32) * -(torch.log(torch.tensor(10000.0)) / (half - 1)))
        ang = torch.arange(n, dtype=torch.float32).unsqueeze(1) * freq.unsqueeze(0)
        return torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)

    def forward(self, tokens, key_padding_mask=None):                      # tokens [B, T] int64, mask [B, T] (1 = pad)
        B, T = tokens.shape
        x = self.embed_tokens(tokens) * (self.embed_dim ** 0.5) + self.positions[:T].to(self.embed_tokens.weight.dtype)
        x = self.dropout(x).transpose(0, 1)                                 # [T, B, C]
        for layer in self.layers:
            x = layer(x, key_padding_mask)
        return x

    def logits(self, x):                                                    # [T, B, C] -> [T, B, vocab]
        return F.linear(x, self.embed_tokens.weight)


def wmt_en_de_encoder(attn_name, attn_args=None, vocab=32768, **kw):
    """Encoder half of transformer_wmt_en_de (512 / 2048 / 8 heads / 6 layers, post-norm)."""
    return EncoderStack(vocab, 512, 2048, 8, 6, attn_name, attn_args, **kw)


# ---- the decoder ----------------------------------------------------------------------------------------------------------------
_FUSED = "ea_ceva_sdecode_linear_fused"                   # (at most _FUSED_MAX_ROWS rows: EA_CEVA_LINEAR_MAX_ROWS of include/ea_hip.h)


def _fused_linear(x2, ln, weight, bias, act, res2, y2):
    """y2 = act(LN(x2) weight^T + bias) + res2 on ea_ceva_sdecode_linear_fused.  x2 [M <= 64, K] fp32 or the weight's type;
    ln: an nn.LayerNorm over K or None; weight [N, K], bias [N] 16-bit; act 0 | 1 (ReLU); res2 [M, N] fp32 or the weight's
    type, or None, and may be y2 itself; y2 [M, N] fp32 or the weight's type -> y2."""
    from efficient_attention import _native as nv
    code = tp.type_code
    gamma = beta = None
    eps = 0.0
    if ln is not None:                                  # (fp32 masters are read where they are)
        gamma, beta, eps = ln.weight.detach(), ln.bias.detach(), ln.eps
        if gamma.dtype != torch.float32:
            gamma, beta = gamma.float(), beta.float()
    nv.call(_FUSED, x2.shape[0], weight.shape[1], weight.shape[0], nv.ptr(x2), code(x2), x2.stride(0),
            nv.ptr(gamma), nv.ptr(beta), eps, nv.ptr(weight), nv.io_dtype(weight), nv.ptr(bias), act,
            nv.ptr(res2), 0 if res2 is None else code(res2), 0 if res2 is None else res2.stride(0),
            nv.ptr(y2), code(y2), y2.stride(0), nv.stream())
    return y2


class DecoderLayer(nn.Module):
    """fairseq's TransformerDecoderLayerBase without encoder attention, under its member names: `self_attn` (a
    CausalEVAttention built as transformer_layer.py:298-308 builds it, no adapter in between), `self_attn_layer_norm`, `fc1`,
    ReLU, `fc2`, `final_layer_norm`; pre-norm (the wikitext-103 recipe) or post-norm."""

    def __init__(self, embed_dim, ffn_dim, num_heads, attn_args=None, dropout=0.1, attention_dropout=0.0,
                 activation_dropout=0.0, normalize_before=True):
        super().__init__()
        self.embed_dim, self.ffn_dim = embed_dim, ffn_dim
        if not isinstance(attn_args, argparse.Namespace):
            attn_args = argparse.Namespace(**dict(attn_args or {}))
        self.self_attn = CausalEVAttention(embed_dim, num_heads, dropout=attention_dropout, self_attention=True,
                                           q_noise=0.0, qn_block_size=8, attn_args=attn_args)
        self.dropout_module = nn.Dropout(dropout)
        self.activation_dropout_module = nn.Dropout(activation_dropout)
        self.normalize_before = normalize_before
        self.self_attn_layer_norm = nn.LayerNorm(embed_dim)
        self.fc1 = nn.Linear(embed_dim, ffn_dim)
        self.fc2 = nn.Linear(ffn_dim, embed_dim)
        self.final_layer_norm = nn.LayerNorm(embed_dim)

    def forward(self, x, key_padding_mask=None):
        """The full causal path: x [T, B, C], key_padding_mask [B, T] (1 = pad) -> [T, B, C]."""
        return self._feed_forward(self._attend(x, key_padding_mask, None), None)

    def _attend(self, x, key_padding_mask, incremental_state):
        res = x
        if self.normalize_before:
            x = self.self_attn_layer_norm(x)
        x, _ = self.self_attn(x, x, x, key_padding_mask=key_padding_mask, incremental_state=incremental_state,
                              need_weights=False)
        x = res + self.dropout_module(x)
        return x if self.normalize_before else self.self_attn_layer_norm(x)

    def _feed_forward(self, x, held):
        """x [T, B, C] behind the attention block -> the layer's output.  held: None -- the layer's own modules; else the
        16-bit (w1, b1, w2, b2) of a decoding state: at most 64 rows run as two ea_ceva_sdecode_linear_fused launches (the
        LayerNorm of a pre-norm layer in the first one's prologue, ReLU in its epilogue, the residual in the second one's:
        fc2's fp32 sums meet the residual unrounded, one rounding fewer than the full path), more rows as the library GEMM
        on the held operands."""
        if held is None:
            res = x
            if self.normalize_before:
                x = self.final_layer_norm(x)
            x = self.fc2(self.activation_dropout_module(F.relu(self.fc1(x))))
            x = res + self.dropout_module(x)
            return x if self.normalize_before else self.final_layer_norm(x)
        w1, b1, w2, b2 = held
        T, B, C = x.shape
        if x.dtype not in (torch.float32, w1.dtype):
            x = x.float()
        if T * B <= _FUSED_MAX_ROWS:
            # (x is this step's own tensor -- the sum behind the attention, or its LayerNorm: the residual stream in place)
            x2 = x.contiguous().view(T * B, C)
            h = torch.empty((T * B, self.ffn_dim), dtype=w1.dtype, device=x.device)
            _fused_linear(x2, self.final_layer_norm if self.normalize_before else None, w1, b1, 1, None, h)
            _fused_linear(h, None, w2, b2, 0, x2, x2)
            x = x2.view(T, B, C)
        else:
            res = x
            if self.normalize_before:
                x = self.final_layer_norm(x)
            with torch.autocast(device_type="cuda", enabled=False):
                h = F.relu(F.linear(x.to(w1.dtype), w1, b1))
                x = res + F.linear(h, w2, b2)
        return x if self.normalize_before else self.final_layer_norm(x)


# ---- decoding states, what they carry and the picks made on them: token_pick.py -----------------------------------------------
_SAMPLE_MAX_K, _BEAM_MAX_W = tp.SAMPLE_MAX_K, tp.BEAM_MAX_W
_SCORE = "ea_vocab_score"
_ADAPTIVE = "ea_adaptive_score"


def _hold_vocab_option(init):
    """`init_decoding` with the keyword-only option `hold_vocab` on top of its parameters.  The parameter list of
    `init_decoding` itself is pinned by the interface test (tests/test_decoder_stack_cpu.py compares the whole list), so the
    option is taken off here, in front of it, and the state it returns is completed behind it; `functools.wraps` keeps the
    pinned list what introspection reports.
    hold_vocab=True: the DecodingState also holds `vocab`, a copy of embed_tokens.weight in the state's dtype (2 V C bytes,
    taken once; `refresh_decoding_weights` re-reads it in place), and the workspace of ea_ceva_sdecode_vocab_argmax for 64
    rows (8 * 64 * ceil(V / 16) bytes): `next_tokens` picks on them, and `generate` ends its step in that kernel.  A 16-bit
    dtype only -- fp32 is refused with hold_weights' ValueError, before anything is allocated; independent of hold_weights
    and of the attention's options."""
    params = inspect.signature(init)

    @functools.wraps(init)
    def init_decoding(self, *args, hold_vocab=False, **kw):
        if hold_vocab and self.is_adaptive:
            raise NotImplementedError("hold_vocab=True on an adaptive stack: the held pick, sampler, scorer and beam entries "
                                      "read one [V, C] table; the greedy pick from the adaptive head is "
                                      "init_adaptive_decoding(state) (then init_sampling(state, ...) and init_beam_search(state, ...) run from it)")
        if hold_vocab:
            given = params.bind(self, *args, **kw).arguments
            if given["dtype"] == torch.float32:
                raise ValueError("hold_vocab=True holds 16-bit projection weights (the vocabulary table of the output "
                                 "projection): an fp32 decoding state (the fidelity path) keeps the library's fp32 GEMM")
        state = init(self, *args, **kw)
        if hold_vocab:                                  # (a state made without the option is what it was, `options` included)
            from efficient_attention import _native as nv
            state.options["hold_vocab"] = True
            w = self.embed_tokens.weight
            dtype, device = state.options["dtype"], state.options["device"]
            ws_bytes = nv.lib().ea_ceva_sdecode_vocab_ws(_FUSED_MAX_ROWS, w.shape[0])
            state.vocab = torch.empty(w.shape, dtype=dtype, device=device)
            state.vocab_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            self._load_held_vocab(state)
        return state
    return init_decoding


class DecoderStack(nn.Module):
    """Decoder-only language model shaped like EncoderStack: token embedding (scaled) + sinusoidal positions -> `layers`
    DecoderLayers (-> a final LayerNorm with final_norm=True) -> [T, B, C]; `logits` is the tied output projection.
    Without `adaptive` a plain tied embedding is both the input and the output layer.  adaptive=dict(cutoff=[...], factor=4,
    dropout=0.0, tie_weights=True, tie_proj=True) builds fairseq's adaptive input and adaptive softmax (the wikitext-103
    recipe's embedding and output layers, ea_harness/adaptive.py) under fairseq's member names, `embed_tokens` and
    `adaptive_softmax`: a reference checkpoint's decoder keys load.  On such a stack `forward`, `decode`, `evaluate` and
    `rows_logprobs` (teacher-forced scoring on ea_adaptive_score, C ABI 33) work, and `init_adaptive_decoding(state)` makes a
    decoding state pick greedily from the held adaptive tables (ea_adaptive_pick, C ABI 34): `next_tokens`, `token_logprobs`,
    `score` and `generate` run on it.  `logits` is the slow torch route (a state without it), and
    `init_decoding(hold_vocab=True)` raises: sampled and beam decoding from the adaptive head are out of scope.
    `adaptive_loss` is such a stack's training loss (fairseq's criterion, ea_harness/adaptive_loss.py); `loss` is the plain one's.

    Incremental decoding runs on the attention's static / rolling states (CausalEVAttention.init_*_decoding):
        state = stack.init_decoding(B, max_tokens, torch.bfloat16, "cuda")
        rows = stack.decode(tokens [T, B], state)              # [T, B, C], prompts and single tokens alike
        new = stack.generate(prompt [B, P], n_new, state)      # greedy, one captured step replayed"""

    def __init__(self, vocab, embed_dim, ffn_dim, num_heads, layers, attn_args=None, dropout=0.1, attention_dropout=0.0,
                 activation_dropout=0.0, normalize_before=True, final_norm=False, max_positions=4096, pad_idx=1,
                 adaptive=None):
        super().__init__()
        self.embed_dim, self.pad_idx = embed_dim, pad_idx
        if adaptive is None:
            self.embed_tokens = nn.Embedding(vocab, embed_dim, padding_idx=pad_idx)
            nn.init.normal_(self.embed_tokens.weight, mean=0, std=embed_dim ** -0.5)
            nn.init.constant_(self.embed_tokens.weight[pad_idx], 0)
        else:
            from .adaptive import AdaptiveInput, AdaptiveSoftmax
            opt = dict(dict(factor=4, dropout=0.0, tie_weights=True, tie_proj=True), **adaptive)
            unknown = set(opt) - {"cutoff", "factor", "dropout", "tie_weights", "tie_proj"}
            if unknown or "cutoff" not in opt:
                raise ValueError("adaptive takes cutoff (required), factor, dropout, tie_weights, tie_proj; got %s"
                                 % sorted(adaptive))
            self.embed_tokens = AdaptiveInput(vocab, pad_idx, embed_dim, opt["factor"], embed_dim, list(opt["cutoff"]))
            self.adaptive_softmax = AdaptiveSoftmax(vocab, embed_dim, list(opt["cutoff"]), opt["dropout"], opt["factor"],
                                                    self.embed_tokens if opt["tie_weights"] else None, opt["tie_proj"])
        self.register_buffer("positions", EncoderStack._sinusoid(max_positions, embed_dim), persistent=False)
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.ModuleList([DecoderLayer(embed_dim, ffn_dim, num_heads, attn_args, dropout, attention_dropout,
                                                  activation_dropout, normalize_before) for _ in range(layers)])
        self.layer_norm = nn.LayerNorm(embed_dim) if final_norm else None

    def forward(self, tokens, key_padding_mask=None):                      # tokens [B, T] int64, mask [B, T] (1 = pad)
        B, T = tokens.shape
        x = self.embed_tokens(tokens) * (self.embed_dim ** 0.5) + self.positions[:T].to(self._embed_dtype())
        x = self.dropout(x).transpose(0, 1)                                 # [T, B, C]
        for layer in self.layers:
            x = layer(x, key_padding_mask)
        return x if self.layer_norm is None else self.layer_norm(x)

    @property
    def is_adaptive(self):
        return hasattr(self, "adaptive_softmax")

    def _embed_dtype(self):
        return self.embed_tokens.dtype if self.is_adaptive else self.embed_tokens.weight.dtype

    def logits(self, x):                                                    # [T, B, C] -> [T, B, vocab]
        """The tied output projection.  On an adaptive stack: the log-probabilities of the WHOLE vocabulary by the torch
        restatement (AdaptiveSoftmax.get_log_prob: every tail on every row, a [T, B, V] tensor) -- the slow route, for
        `generate` on a state without `init_adaptive_decoding`; scoring runs on `rows_logprobs`."""
        if self.is_adaptive:
            return self.adaptive_softmax.get_log_prob(x)
        return F.linear(x, self.embed_tokens.weight)

    # ---- incremental decoding -----------------------------------------------------------------------------------------------
    @_hold_vocab_option
    def init_decoding(self, batch_size, max_tokens, dtype, device, rolling=True, hold_weights=True, per_sequence=False,
                      landmark_splits=1, compact_landmarks=False, max_step_tokens=None):
        """One static (rolling=False) or rolling decoding state per layer's attention, made by `init_static_decoding` /
        `init_rolling_decoding` with `per_sequence`, `landmark_splits`, `compact_landmarks` (and, rolling, `max_step_tokens`)
        handed on and `hold_projections=hold_weights` -> a DecodingState.  With hold_weights (a 16-bit `dtype` only: fp32 is
        refused with the attention's ValueError) the state also holds 16-bit copies of every layer's fc1 / fc2 weights and
        biases, 2 (C F + F + F C + C) bytes per layer, taken here once: a capture fixes the weights, and
        `refresh_decoding_weights` re-reads them.  `max_tokens` may not pass the position table.
        Keyword-only, on top of these: `hold_vocab=False` (see `_hold_vocab_option`)."""
        if hold_weights:
            self.layers[0].self_attn._check_hold_projections(True, dtype)
        if int(max_tokens) > self.positions.shape[0]:
            raise ValueError("max_tokens %d passes the %d positions of the table (max_positions)"
                             % (int(max_tokens), self.positions.shape[0]))
        options = dict(batch_size=int(batch_size), max_tokens=int(max_tokens), dtype=dtype, device=device, rolling=bool(rolling),
                       hold_weights=bool(hold_weights), per_sequence=bool(per_sequence), landmark_splits=landmark_splits,
                       compact_landmarks=bool(compact_landmarks), max_step_tokens=max_step_tokens)
        opt = dict(per_sequence=per_sequence, landmark_splits=landmark_splits, hold_projections=hold_weights,
                   compact_landmarks=compact_landmarks)
        incremental = {}
        for layer in self.layers:
            if rolling:
                layer.self_attn.init_rolling_decoding(incremental, batch_size, max_tokens, dtype, device,
                                                      max_step_tokens=max_step_tokens, **opt)
            else:
                layer.self_attn.init_static_decoding(incremental, batch_size, max_tokens, dtype, device, **opt)
        ffn = None
        if hold_weights:
            ffn = [tuple(torch.empty(p.shape, dtype=dtype, device=device)
                         for p in (layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias)) for layer in self.layers]
        state = DecodingState(incremental, ffn, options)
        self._load_held_ffn(state)
        return state

    def _load_held_ffn(self, state):
        if state.ffn is None:
            return
        with torch.no_grad():
            for layer, held in zip(self.layers, state.ffn):
                for dst, src in zip(held, (layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias)):
                    dst.copy_(src)                      # (rounded to nearest even, in place: every data_ptr() stays)

    def _load_held_vocab(self, state):
        if state.vocab is not None:
            tp.HeldVocab(state).refresh(self)

    def refresh_decoding_weights(self, state):
        """Re-read the parameters into what the state holds of them, in place and by device ops only: every layer's attention
        (`CausalEVAttention.refresh_decoding_weights`), the held fc1 / fc2 and the held vocabulary table.  A step captured
        before sees the new weights."""
        for layer in self.layers:
            layer.self_attn.refresh_decoding_weights(state.incremental)
        self._load_held_ffn(state)
        for held in state.attachments():
            held.refresh(self)
        return state

    def reorder_decoding_state(self, state, new_order):
        for layer in self.layers:
            layer.self_attn.reorder_incremental_state(state.incremental, new_order)
        for held in state.attachments():
            held.reorder(new_order)
        return state

    def reset_decoding_rows(self, state, rows):
        for layer in self.layers:
            layer.self_attn.reset_decoding_rows(state.incremental, rows)
        for held in state.attachments():
            held.reset_rows(rows)
        return state

    def decoding_state_nbytes(self, state):
        """Bytes of every layer's attention state, of the held feed-forward weights, of the held vocabulary table with
        its workspace, of a sampler's logits, counters and stream ids (4 B V + 8 B + 4 B) and of a scorer's workspace and
        buffers (4 * 64 * (ceil(V / 16) + 1) + 8 B), and of a beam search's buffers for M = S W rows (`init_beam_search`):
        4 M V (logits) + ea_ceva_sdecode_vocab_beam_ws(M, V, W) (workspace) + 4 M (score) + 12 S (t, nfin, done) + 8 M
        (parent) + 8 max_new M (the history) + 12 S W (the records), and of an adaptive pick's tables, workspace
        (ea_adaptive_pick_ws for 64 rows) and 4 B (logp).  On a state with an adaptive pick the sampler's logits give way to
        ea_adaptive_sample_ws(B, ..) and the beam's logits and workspace to ea_adaptive_beam_ws(M, .., W)."""
        n = sum(layer.self_attn.decoding_state_nbytes(state.incremental) for layer in self.layers)
        n += sum(t.numel() * t.element_size() for held in (state.ffn or ()) for t in held)
        return n + sum(t.numel() * t.element_size() for held in state.attachments() for t in held.tensors())

    def decoding_overflowed(self, state):
        """True once a step of any layer would have passed the state's capacity.  Reads device flags back."""
        return any(layer.self_attn.static_decoding_overflowed(state.incremental) for layer in self.layers)

    def decode(self, tokens, state, key_padding_mask=None):
        """One decoding step: tokens [T, B] int64 (a prompt, a single token, a short verify step) -> [T, B, C], the rows
        `forward` gives for these positions.  Positions are gathered from the sinusoid table by the DEVICE counts of the first
        layer's state (`decoding_positions_tensor`): no read-back, so the step can be captured, and a row of a per-sequence
        state gets its own positions.  key_padding_mask: handed to every attention (a per-sequence state: a row's tokens are
        those before its first flag).  Every launch is a device op; under autocast the residual stream stays fp32 as in
        `forward`.  On a state made with hold_weights a step of T B <= 64 rows runs each layer as
            LayerNorm, ea_ceva_sdecode_linear, the attention's launches, ea_ceva_sdecode_linear, add,
            ea_ceva_sdecode_linear_fused (LayerNorm, fc1, ReLU), ea_ceva_sdecode_linear_fused (fc2, residual, in place)
        (post-norm: the two LayerNorms behind the sums, by the framework); a larger step runs the library GEMM on the held
        operands; without hold_weights the feed-forward is the layer's own modules."""
        if self.training:
            raise NotImplementedError("incremental decoding in training mode")
        T, B = tokens.shape
        attn0 = self.layers[0].self_attn
        pos = attn0.decoding_positions_tensor(state.incremental)             # [1] or [B] int32, on the device
        idx = pos.to(torch.long).view(1, -1) + torch.arange(T, device=pos.device).view(T, 1)
        idx = idx.clamp_(max=self.positions.shape[0] - 1).expand(T, B)       # (a step past the table overflows the state too)
        x = self.embed_tokens(tokens) * (self.embed_dim ** 0.5) + self.positions[idx].to(self._embed_dtype())
        for i, layer in enumerate(self.layers):
            x = layer._attend(x, key_padding_mask, state.incremental)
            x = layer._feed_forward(x, None if state.ffn is None else state.ffn[i])
        return x if self.layer_norm is None else self.layer_norm(x)

    # ---- the decoding loop of `generate` and `beam_search` ------------------------------------------------------------------
    def _decoding_context(self):
        """-> (the context a decoding call runs its steps in, the dtype of a state it makes for itself): under autocast that
        autocast again without its weight-cast cache (a capture may not use it) and its dtype, else the embedding's."""
        if torch.is_autocast_enabled():
            dtype = torch.get_autocast_dtype("cuda")
            return torch.autocast("cuda", dtype=dtype, cache_enabled=False), dtype
        return contextlib.nullcontext(), self._embed_dtype()

    def _prefill(self, prompt, state):
        """The prompt [B, P] fed in one `decode` -> [1, B, C], the row of each sequence's last token (a per-sequence state:
        the prompt may be ragged and right-padded with `pad_idx`)."""
        B, P = prompt.shape
        if not state.options["per_sequence"]:
            return self.decode(prompt.t(), state, None)[P - 1:P]
        mask = prompt.eq(self.pad_idx)
        x = self.decode(prompt.t(), state, mask)                             # [P, B, C]
        n_b = P - mask.ne(0).to(torch.int32).cumsum(1).ne(0).sum(1)
        return x[(n_b - 1).clamp_(min=0), torch.arange(B, device=x.device)].unsqueeze(0)

    def _run_steps(self, step, state, n, graph, tok_in, scratch, pick=None, each=None):
        """Steps 1 .. n - 1 behind a first pick: step(st) is one step on the state `st`, reading and writing the static input
        `tok_in`, -> its rows.  graph=True: warmed up on a side stream on `scratch()`, a state of its own, with `tok_in` and
        what `pick` saved restored behind it; then captured on `state` once and replayed.  each(i, rows), behind step i (the
        rows are the capture's static ones), ends the loop by returning True.  An overflow flagged by any layer raises."""
        g = y = None
        if graph and n > 1:
            st = scratch()
            first = tok_in.clone()
            saved = None if pick is None else pick.save()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step(st)
            torch.cuda.current_stream().wait_stream(side)
            tok_in.copy_(first)
            if saved is not None:                                            # (the warm-up drew once)
                pick.restore(saved)
            del st
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                y = step(state)
        for i in range(1, n):
            if g is None:
                y = step(state)
            else:
                g.replay()
            if each is not None and each(i, y):
                break
        if self.decoding_overflowed(state):
            raise RuntimeError("the decoding state overflowed: a step passed its %d tokens (init_decoding(max_tokens=...))"
                               % state.options["max_tokens"])

    def next_tokens(self, rows, state, out=None, return_logits=False):
        """The greedy pick on the table the state holds: rows [T, B, C] (final-layer rows: what `decode` returns) -> int64
        [T, B], token[t, b] = argmax_v sum_c round(rows[t, b, c]) vocab[v, c], on ea_ceva_sdecode_vocab_argmax: the table is
        streamed once, the sums are fp32 and the pick is made ON THE FP32 SUMS under torch.argmax's rule (ties: the lowest
        index).  `logits(rows).argmax(-1)` under autocast picks on logits already rounded to 16 bits; where two logits round
        to the same 16-bit value the two can differ, and this one is the pick of the unrounded sums.
        out: an int64 [T, B] contiguous tensor the tokens are written into (and returned) -- a captured step hands its own
        static input.  return_logits=True: -> (tokens, fp32 [T, B, V] logits), for a caller that samples.  Rows that are
        neither fp32 nor the table's type are widened to fp32 first (the kernel rounds fp32 rows to the table's type as it
        loads them).  More than 64 rows run in pieces of 64.  Device launches only.
        On a state with an adaptive pick (`init_adaptive_decoding`) the token is the argmax of the adaptive softmax's joint
        log-probabilities, on ea_adaptive_pick; return_logits is not offered there."""
        if state.adaptive is not None:
            if return_logits:
                raise ValueError("next_tokens(return_logits=True) on an adaptive pick: no [T, B, V] tensor exists there "
                                 "(`logits` is the slow route)")
            return tp.AdaptiveGreedy(self, state).run(rows, None, out, None)[0]
        if state.vocab is None:
            raise RuntimeError("next_tokens needs a decoding state that holds the vocabulary table: "
                               "init_decoding(..., hold_vocab=True)")
        return tp.HeldGreedy(self, state).run(rows, out, return_logits)

    def init_sampling(self, state, seed, top_k, top_p=1.0, temperature=1.0):
        """Make `state` (made with hold_vocab=True) sample its tokens: `sample_tokens` draws on it, and `generate` takes both
        of its picks from there.  A token is drawn from the `top_k` (1 .. 64) largest logits of its row, softmax weights at
        `temperature` (> 0), cut to the smallest head of that list whose weight reaches `top_p` (0 < top_p <= 1) of the
        list's -- ea_ceva_sdecode_vocab_sample, include/ea_hip.h.  The draws are Philox4x32-10 words keyed by `seed`
        (0 .. 2^64 - 1) at the counter (ctr[b], sid[b]): row b starts as stream b at draw 0, every draw advances ctr[b] on the
        device, so a captured step draws afresh at every replay; `reorder_decoding_state` moves (ctr, sid) with the rows and
        `reset_decoding_rows` starts a reset row on a stream id no row of this state has had.  A row's tokens are therefore
        what it would draw decoded alone with its (seed, sid), whatever batch it sits in.
        Attaches `state.sampler` (a Sampler: fp32 logits [batch_size, V], ctr, sid, the scalars; 4 B V + 12 B bytes; the
        pick's workspace is `vocab_ws`) and returns the state.  Values outside the envelope raise ValueError before anything
        is allocated; full-vocabulary sampling stays with `next_tokens(return_logits=True)`.
        On a state with an adaptive pick (`init_adaptive_decoding`) the list is the `top_k` largest JOINT log-probabilities of
        the adaptive softmax and the temperature acts on them -- ea_adaptive_sample, include/ea_hip.h (ABI 35); fairseq
        divides the features by it instead.  The Sampler then holds `ws`, that entry's workspace for batch_size rows (every
        band's fp32 logits: about 4 B V bytes) in place of the logits buffer; everything else above holds."""
        if state.vocab is None and state.adaptive is None:
            raise RuntimeError("init_sampling needs a decoding state that holds the vocabulary table: "
                               "init_decoding(..., hold_vocab=True)")
        seed, top_k, top_p, temperature = int(seed), int(top_k), float(top_p), float(temperature)
        if not 1 <= top_k <= _SAMPLE_MAX_K:
            raise ValueError("top_k must be in 1 .. %d, got %d" % (_SAMPLE_MAX_K, top_k))
        if not 0.0 < top_p <= 1.0:
            raise ValueError("top_p must be in (0, 1], got %r" % top_p)
        if not (math.isfinite(temperature) and temperature > 0.0):
            raise ValueError("temperature must be finite and > 0, got %r" % temperature)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must be in 0 .. 2^64 - 1, got %d" % seed)
        B = state.options["batch_size"]
        if state.adaptive is not None:
            from efficient_attention import _native as nv
            tables = state.adaptive.tables
            device = tables.device
            nbytes = nv.lib().ea_adaptive_sample_ws(B, len(tables.dims), *tables.host_arrays()[:2])
            if nbytes < 0:
                raise ValueError("a state of %d rows is outside ea_adaptive_sample's envelope (at most %d)" % (B, _FUSED_MAX_ROWS))
            logits, ws = None, torch.empty(nbytes, dtype=torch.uint8, device=device)
        else:
            device = state.vocab.device
            logits, ws = torch.empty((B, state.vocab.shape[0]), dtype=torch.float32, device=device), None
        state.sampler = Sampler(logits, torch.zeros(B, dtype=torch.long, device=device),
                                torch.arange(B, dtype=torch.int32, device=device), seed, top_k, top_p, temperature, ws=ws)
        return state

    def sample_tokens(self, rows, state, out=None, return_details=False):
        """The sampled pick on a state with a sampler (`init_sampling`): rows [1, B, C] (final-layer rows of a single-token
        step, B <= 64 and at most the state's batch size) -> int64 [1, B], one draw per row from ea_ceva_sdecode_vocab_sample on
        the held table; row b draws at (ctr[b], sid[b]) and its counter advances.  out: as in `next_tokens`.
        return_details=True: -> (tokens, sel_idx int32 [B, top_k], sel_val fp32 [B, top_k], kept int32 [B]): the selection in
        order (entries from min(top_k, V) on are not written; log-probabilities follow from sel_val), and how many of it the
        nucleus kept (0: a row whose best logit is NaN or infinite, which gets the greedy pick).  Device launches only.
        On a state with an adaptive pick the draw is ea_adaptive_sample's: sel_idx are vocabulary indices, sel_val their
        joint log-probabilities."""
        if state.sampler is None:
            raise RuntimeError("sample_tokens needs a decoding state with a sampler: init_sampling(state, seed, top_k, ...)")
        if state.adaptive is not None:
            got = tp.AdaptiveSampled(self, state).run(rows, out, None, return_details)
            return (got[0],) + got[2:] if return_details else got[0]
        return tp.HeldSampled(self, state).run(rows, out, return_details)

    def init_logprobs(self, state):
        """Make `state` (made with hold_vocab=True) report log-probabilities: `token_logprobs`, `sample_tokens_logprobs`,
        `score` and `generate(return_logprobs=True)` run on it.  A log-probability is log softmax(logits)[token] of the row's
        WHOLE, raw distribution at temperature 1 -- of a sampled token too, whatever the sampler's temperature, top_k and
        top_p -- formed in the pass that picks the token: ea_ceva_sdecode_vocab_logprob, include/ea_hip.h.
        Attaches `state.scorer` (a Scorer: the workspace for 64 rows, 4 * 64 * (ceil(V / 16) + 1) bytes, and fp32 `lse`,
        `logp` [batch_size]) and returns the state.  A beam reorder, a row reset and a weight refresh have nothing of it to
        move."""
        if state.vocab is None:
            raise RuntimeError("init_logprobs needs a decoding state that holds the vocabulary table: "
                               "init_decoding(..., hold_vocab=True)")
        from efficient_attention import _native as nv
        B, device = state.options["batch_size"], state.vocab.device
        nbytes = nv.lib().ea_ceva_sdecode_vocab_lse_ws(_FUSED_MAX_ROWS, state.vocab.shape[0])
        state.scorer = Scorer(torch.empty(nbytes, dtype=torch.uint8, device=device),
                              torch.empty(B, dtype=torch.float32, device=device),
                              torch.empty(B, dtype=torch.float32, device=device))
        return state

    def token_logprobs(self, rows, state, targets=None, out=None, return_lse=False):
        """The greedy pick of `next_tokens` and a log-probability per row, on a state with a scorer (`init_logprobs`): rows
        [T, B, C] -> (tokens int64 [T, B], logp fp32 [T, B]); return_lse=True: and lse fp32 [T, B], the log-sum-exp of the row's
        fp32 logits.  logp[t, b] = logit[targets[t, b]] - lse with `targets` (int64 [T, B] on the device; one outside [0, V)
        gives NaN), else the picked token's, top - lse.  `tokens` is the greedy pick either way, bit for bit `next_tokens`'.
        The distribution is the model's own at temperature 1; the table is streamed once per 64 rows, no [T B, V] tensor
        exists.  A row's results do not depend on the rows beside it.  out: as in `next_tokens`.  Device launches only.
        On a state with an adaptive pick (`init_adaptive_decoding`; no `init_logprobs` needed) logp is the joint
        log-probability under the adaptive softmax, of targets[t, b] or of the picked token; there is no single log-sum-exp,
        so return_lse raises."""
        if state.adaptive is not None:
            if return_lse:
                raise ValueError("token_logprobs(return_lse=True) on an adaptive pick: an adaptive softmax has no single "
                                 "log-sum-exp to return")
            return tp.AdaptiveGreedy(self, state).run(rows, targets, out, None)
        if state.vocab is None or state.scorer is None:
            raise RuntimeError("token_logprobs needs a decoding state with a scorer: init_logprobs(state), on a state made "
                               "with init_decoding(..., hold_vocab=True)")
        tokens, logp, lse = tp.HeldGreedyLogprob(self, state).run(rows, targets, out, None, None)
        return (tokens, logp, lse) if return_lse else (tokens, logp)

    # ---- the greedy pick from the adaptive head (ea_adaptive_pick, C ABI 34) ---------------------------------------------------
    def init_adaptive_decoding(self, state, tables=None):
        """Make `state` (a 16-bit decoding state of an adaptive stack) pick its tokens from the adaptive head on HIP:
        `next_tokens`, `token_logprobs`, `score` and `generate` (with return_logprobs too) then end in ea_adaptive_pick
        (include/ea_hip.h, ABI 34) -- the head, the projections and the tails are streamed once per 64 rows (89 MB on the
        recipe's geometry against the 548 MB of a plain [V, C] table), no [rows, V] tensor exists, and the call can be
        captured.  tables: an AdaptiveTables in the state's dtype on its device (default: `adaptive_tables` of them).
        Attaches `state.adaptive` (an AdaptivePick: the tables, the workspace for 64 rows, fp32 logp [batch_size]) and
        returns the state.  A beam reorder and a row reset have nothing of it to move; `refresh_decoding_weights` re-reads
        the tables in place."""
        if not self.is_adaptive:
            raise RuntimeError("init_adaptive_decoding needs a stack built with adaptive=dict(cutoff=...)")
        dtype, device = state.options["dtype"], state.options["device"]
        if dtype == torch.float32:
            raise ValueError("init_adaptive_decoding holds 16-bit tables: an fp32 decoding state (the fidelity path) keeps "
                             "`logits`, the slow route")
        if tables is None:
            tables = self.adaptive_tables(dtype, device)
        elif not isinstance(tables, AdaptiveTables) or tables.dtype != dtype:
            raise ValueError("tables must be an AdaptiveTables in the state's dtype (%s)" % str(dtype).replace("torch.", ""))
        from efficient_attention import _native as nv
        nbytes = nv.lib().ea_adaptive_pick_ws(_FUSED_MAX_ROWS, len(tables.dims), *tables.host_arrays()[:2])
        if nbytes < 0:
            raise ValueError("cutoffs %s at widths %s are outside ea_adaptive_pick's envelope" % (tables.cutoff, tables.dims))
        state.adaptive = AdaptivePick(tables, torch.empty(nbytes, dtype=torch.uint8, device=tables.device),
                                      torch.empty(state.options["batch_size"], dtype=torch.float32, device=tables.device))
        return state

    def sample_tokens_logprobs(self, rows, state, out=None):
        """`sample_tokens` and the drawn tokens' log-probabilities, on a state with a sampler and a scorer: rows [1, B, C] ->
        (tokens int64 [1, B], logp fp32 [1, B]).  The tokens, and the counters behind them, are `sample_tokens`' at the same
        (seed, ctr, sid).  logp is the token's log-probability under the RAW distribution at temperature 1 -- not inside the
        top-k list or the nucleus, not at the sampler's temperature.  Device launches only.
        On a state with an adaptive pick and a sampler (no scorer needed) logp is the drawn token's joint log-probability,
        from the same ea_adaptive_sample call."""
        if state.sampler is not None and state.adaptive is not None:
            return tp.AdaptiveSampled(self, state).run(rows, out, None, False, who="a sampled pick")
        if state.sampler is None or state.scorer is None:
            raise RuntimeError("sample_tokens_logprobs needs a decoding state with a sampler and a scorer: "
                               "init_sampling(state, seed, top_k, ...) and init_logprobs(state)")
        tokens, logp, _ = tp.HeldSampledLogprob(self, state).run(rows, out, None, None)
        return tokens, logp

    def score(self, tokens, state=None):
        """Teacher-forced log-probabilities: tokens [B, T] int64 -> fp32 [B, T - 1], entry [b, t] = log p(tokens[b, t + 1] |
        tokens[b, :t + 1]) under the model's own distribution; entries whose target is `pad_idx` are 0.  One `decode` of
        tokens[:, :-1] on `state` (a fresh state with a scorer, or with an adaptive pick; default: one made here with
        hold_vocab -- on an adaptive stack with `init_adaptive_decoding` -- and the autocast or the weights' 16-bit dtype),
        then `token_logprobs` with the targets.  The vocabulary table is re-streamed once per 64
        rows of T - 1 times B: this serves prompt scoring, not corpus-scale evaluation."""
        if self.training:
            raise NotImplementedError("incremental decoding in training mode")
        B, T = tokens.shape
        if T < 2:
            raise ValueError("score needs at least two tokens per row, got %d" % T)
        ctx, dtype = self._decoding_context()
        with torch.no_grad(), ctx:
            if state is None:
                if self.is_adaptive:
                    state = self.init_adaptive_decoding(self.init_decoding(B, T - 1, dtype, tokens.device))
                else:
                    state = self.init_logprobs(self.init_decoding(B, T - 1, dtype, tokens.device, hold_vocab=True))
            elif state.scorer is None and state.adaptive is None:
                raise RuntimeError("score needs a decoding state with a scorer: init_logprobs(state)")
            fed = tokens[:, :-1]
            mask = fed.eq(self.pad_idx) if state.options["per_sequence"] else None
            rows = self.decode(fed.t(), state, mask)                         # [T - 1, B, C]
            targets = tokens[:, 1:].t().contiguous()
            _, logp = self.token_logprobs(rows, state, targets=targets)
            return logp.masked_fill_(targets.eq(self.pad_idx), 0.0).t().contiguous()

    # ---- corpus-scale scoring (ea_vocab_score, C ABI 30) --------------------------------------------------------------------
    def rows_logprobs(self, rows, table, targets=None, return_lse=False):
        """`token_logprobs` for ANY number of rows, on a table the caller holds: rows [T, B, C], table a contiguous 16-bit
        [V, C] tensor on the rows' device (`state.vocab` of a hold_vocab state serves) -> (tokens int64 [T, B], logp fp32
        [T, B]); return_lse=True: and lse fp32 [T, B].  tokens is the greedy pick, logp[t, b] = logit[targets[t, b]] - lse
        with `targets` (int64 [T, B] on the device; one outside [0, V) gives NaN), else top - lse.  ONE call of
        ea_vocab_score (include/ea_hip.h, ABI 30) on a workspace sized by its query: a tiled GEMM on the matrix cores with
        the pick and an online log-sum-exp as its epilogue -- no framework GEMM, no [T B, V] tensor; the table is read once
        per 128 rows.  A logit's order of summation is that kernel's own: results agree with `token_logprobs` to rounding,
        not bit for bit.  A row's results do not depend on the rows beside it.
        table an AdaptiveTables (`adaptive_tables`): ONE call of ea_adaptive_score (ABI 33) -> (head_tokens int64 [T, B], the
        greedy pick among the head's c0 + n columns, logp fp32 [T, B]), the targets' log-probabilities under the adaptive
        softmax; `targets` is required there (the whole distribution is `logits`, the slow route), return_lse is not offered."""
        if isinstance(table, AdaptiveTables):
            return self._adaptive_rows_logprobs(rows, table, targets, return_lse)
        from efficient_attention import _native as nv
        x2 = tp.score_operand(table, rows)
        T, B, C = rows.shape
        V, dev = table.shape[0], x2.device
        targets = tp.checked_targets(targets, T, B, dev)
        nv.require_cuda(x2, "rows")
        # (the entry's sizes are int32: a count of 2^31 or more would wrap on its way into the query)
        nbytes = nv.lib().ea_vocab_score_ws(T * B, V) if max(T * B, V, C) < 2 ** 31 else -1
        if nbytes < 0:
            raise ValueError("%d rows against %d table rows are outside ea_vocab_score's envelope" % (T * B, V))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((T, B), dtype=torch.long, device=dev)
        logp = torch.empty((T, B), dtype=torch.float32, device=dev)
        lse = torch.empty((T, B), dtype=torch.float32, device=dev)
        nv.call(_SCORE, T * B, C, V, nv.ptr(x2), tp.type_code(x2), C, nv.ptr(table), nv.io_dtype(table), nv.ptr(targets), None, nv.EA_F32,
                V, nv.ptr(ws), ws.numel(), nv.ptr(out), None, nv.ptr(lse), nv.ptr(logp), nv.stream())
        return (out, logp, lse) if return_lse else (out, logp)

    def adaptive_tables(self, dtype=torch.bfloat16, device=None):
        """The 16-bit operands of `rows_logprobs` on an adaptive stack, copied once (an AdaptiveTables; `refresh()` re-reads
        them in place): about 2 (c0 C + sum_i (d_i C + V_i d_i)) bytes."""
        if not self.is_adaptive:
            raise RuntimeError("adaptive_tables needs a stack built with adaptive=dict(cutoff=...)")
        if device is None:
            device = self.adaptive_softmax.tail_table(0).device
        return AdaptiveTables(self.adaptive_softmax, dtype, device)

    def _adaptive_rows_logprobs(self, rows, tables, targets, return_lse):
        if targets is None:
            raise ValueError("rows_logprobs on adaptive tables scores targets: pass targets (the whole distribution is "
                             "`logits`, the slow route)")
        if return_lse:
            raise ValueError("rows_logprobs on adaptive tables has no single log-sum-exp to return")
        from efficient_attention import _native as nv
        x2 = tp.score_operand(tables.head, rows)
        T, B, C = rows.shape
        dev, n = x2.device, len(tables.dims)
        targets = tp.checked_targets(targets, T, B, dev)
        nv.require_cuda(x2, "rows")
        cut, dims, proj, tabs = tables.host_arrays()
        nbytes = nv.lib().ea_adaptive_score_ws(T * B, n, cut, dims) if max(T * B, C) < 2 ** 31 else -1
        if nbytes < 0:
            raise ValueError("%d rows against cutoffs %s are outside ea_adaptive_score's envelope" % (T * B, tables.cutoff))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        head = torch.empty((T, B), dtype=torch.long, device=dev)
        logp = torch.empty((T, B), dtype=torch.float32, device=dev)
        nv.call(_ADAPTIVE, T * B, C, n, cut, dims, nv.ptr(x2), tp.type_code(x2), C, nv.ptr(targets), nv.ptr(tables.head),
                nv.io_dtype(tables.head), proj, tabs, nv.ptr(ws), ws.numel(), nv.ptr(logp), nv.ptr(head), nv.stream())
        return head, logp

    def evaluate(self, tokens, table=None, key_padding_mask=None, return_tokens=False):
        """Teacher-forced log-probabilities for corpus-scale evaluation (perplexity): tokens [B, T] int64 -> fp32 [B, T - 1],
        entry [b, t] = log p(tokens[b, t + 1] | tokens[b, :t + 1]); entries whose target is `pad_idx` are 0, as in `score`;
        return_tokens=True: and the greedy tokens, int64 [B, T - 1].  Runs the FULL path, `self(tokens[:, :-1],
        key_padding_mask)`, under no_grad, then `rows_logprobs` on `table` (default: a 16-bit copy of embed_tokens.weight made
        for the call, in the autocast dtype under autocast, else bfloat16).
        How it differs from `score`: that one feeds the tokens through `decode` -- the incremental DECODING path and its
        state -- and streams the table once per 64 rows, ceil(rows / 64) passes; this one runs the full (training-shaped)
        forward and passes over the table in proportion to ceil(rows / 128), the row tile of ea_vocab_score, each pass on
        the matrix cores at full tiles.  The two agree to rounding, not bit for bit.
        On an adaptive stack `table` is an AdaptiveTables (default: `adaptive_tables` in the autocast dtype, else bfloat16)
        and the rows are scored by ONE ea_adaptive_score call: no [rows, V] and no [rows, c0 + n] tensor exists;
        return_tokens gives the greedy pick among the head's columns (a class column c0 + i stands for tail i)."""
        if self.training:
            raise NotImplementedError("evaluate in training mode")
        B, T = tokens.shape
        if T < 2:
            raise ValueError("evaluate needs at least two tokens per row, got %d" % T)
        with torch.no_grad():
            if table is None:
                dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else torch.bfloat16
                table = self.adaptive_tables(dtype, tokens.device) if self.is_adaptive \
                    else self.embed_tokens.weight.detach().to(dtype).contiguous()
            rows = self(tokens[:, :-1], key_padding_mask)                    # [T - 1, B, C]
            targets = tokens[:, 1:].t().contiguous()
            greedy, logp = self.rows_logprobs(rows, table, targets)
            logp = logp.masked_fill_(targets.eq(self.pad_idx), 0.0).t().contiguous()
            return (logp, greedy.t().contiguous()) if return_tokens else logp

    # ---- the training loss (ea_vocab_score forward, ea_vocab_nll_grad / ea_gemm_nt16 backward, C ABI 38) -----------------------
    def loss(self, tokens, key_padding_mask=None, reduction="mean"):
        """The next-token cross-entropy with a gradient: tokens [B, T] int64 -> the negative log-likelihood of tokens[:, 1:]
        given what precedes them.  Runs the full (training-shaped) forward on tokens[:, :-1], then
        `ea_harness.vocab_loss.vocab_nll` on embed_tokens.weight: the scorer of `evaluate` forward, HIP kernels backward, no
        [rows, V] tensor in either direction and a log-sum-exp over unrounded fp32 sums.  Targets equal to `pad_idx` have
        loss 0 and add exact zeros to every gradient.  reduction: "mean" (over the non-pad targets, counted on the device;
        nothing is read back), "sum", or "none" (fp32 [B, T - 1]; in eval mode -`evaluate(tokens)` bit for bit).  The table
        is the tied embedding: autograd adds the lookup's gradient to the projection's by itself.
        On an adaptive stack: NotImplementedError; the adaptive-softmax loss is `adaptive_loss`."""
        if self.is_adaptive:
            raise NotImplementedError("loss on an adaptive stack: the adaptive-softmax training loss is a follow-up to this "
                                      "method and lives in adaptive_loss(tokens, ...); loss takes the plain tied table")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none', got %r" % (reduction,))
        B, T = tokens.shape
        if T < 2:
            raise ValueError("loss needs at least two tokens per row, got %d" % T)
        from .vocab_loss import vocab_nll
        rows = self(tokens[:, :-1], key_padding_mask)                        # [T - 1, B, C]
        targets = tokens[:, 1:].t().contiguous()
        pad = targets.eq(self.pad_idx)
        nll = -vocab_nll(rows, self.embed_tokens.weight, targets).masked_fill(pad, 0.0)
        if reduction == "none":
            return nll.t().contiguous()
        if reduction == "sum":
            return nll.sum()
        return nll.sum() / pad.logical_not().sum().clamp(min=1)

    # ---- the adaptive-softmax training loss (ea_adaptive_score forward, ea_adaptive_nll.hip backward) ---------------------------
    def adaptive_loss(self, tokens, key_padding_mask=None, reduction="mean"):
        """fairseq's `adaptive_loss` criterion with a gradient, on an adaptive stack: the contract of `loss` (tokens [B, T]
        int64 -> the negative log-likelihood of tokens[:, 1:]; pad targets have loss 0 and add exact zeros to every gradient;
        reduction "mean" over the non-pad targets counted on the device, "sum", or "none": fp32 [B, T - 1], in eval mode
        -`evaluate(tokens)` bit for bit).  Runs the full forward on tokens[:, :-1], then `ea_harness.adaptive_loss.adaptive_nll`
        on the adaptive softmax's parameters: ea_adaptive_score forward, HIP kernels backward, no [rows, V], [rows, c0 + n] or
        [rows_i, V_i] tensor and nothing read back.  The band tables and projections are tied to the adaptive input: autograd
        adds the input side's gradients by itself.
        In training mode with `adaptive_softmax.dropout` = p > 0 both of fairseq's dropouts apply: F.dropout on the rows in
        front, and inside each tail a mask of {0, 1 / (1 - p)} in the tables' dtype on h_i, drawn by the framework's generator
        (graph-safe), one row per position of the tail's list.  On a stack without `adaptive`: RuntimeError."""
        if not self.is_adaptive:
            raise RuntimeError("adaptive_loss needs a stack built with adaptive=dict(cutoff=...); a plain tied table trains with loss")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none', got %r" % (reduction,))
        B, T = tokens.shape
        if T < 2:
            raise ValueError("adaptive_loss needs at least two tokens per row, got %d" % T)
        from .adaptive_loss import adaptive_nll, operand_dtype
        sm = self.adaptive_softmax
        rows = self(tokens[:, :-1], key_padding_mask)                        # [T - 1, B, C]
        targets = tokens[:, 1:].t().contiguous()
        pad = targets.eq(self.pad_idx)
        masks = None
        if self.training and sm.dropout > 0:
            rows = F.dropout(rows, sm.dropout, True)
            E = operand_dtype(rows, sm)
            masks = [F.dropout(torch.ones(((T - 1) * B, d), dtype=E, device=rows.device), sm.dropout, True) for d in sm.band_dims()]
        nll = -adaptive_nll(rows, sm, targets, tail_masks=masks).masked_fill(pad, 0.0)
        if reduction == "none":
            return nll.t().contiguous()
        if reduction == "sum":
            return nll.sum()
        return nll.sum() / pad.logical_not().sum().clamp(min=1)

    # ---- beam search (ea_ceva_sdecode_vocab_beam, C ABI 32) ------------------------------------------------------------------
    def init_beam_search(self, state, beam_size, eos_idx, max_new, len_penalty=1.0):
        """Make `state` (made with hold_vocab=True, no sampler; its batch size M a multiple of `beam_size`) search with beams:
        rows s W .. s W + W - 1 are the W = beam_size beams of sentence s, S = M / W sentences.  `eos_idx` (0 <= eos_idx < V)
        ends a hypothesis; `max_new` >= 1 is the largest number of generated tokens of one, the closing eos included (the
        step that would pass it ends every live beam with eos); `len_penalty`: a finished hypothesis ranks by its raw score
        (the fp32 sum of its tokens' log-probabilities) over length ** len_penalty, on the host, behind the search.
        Envelope: 1 <= W <= 32, M <= 64.  Values outside it raise ValueError before anything is allocated.  Attaches
        `state.beam` (a Beam: the static buffers of the step, initialised; bytes: `decoding_state_nbytes`) and returns the
        state.  On a state with an adaptive pick (`init_adaptive_decoding`) the step is ea_adaptive_beam (ABI 35): a row's 2 W
        candidates are its best JOINT log-probabilities; the Beam's `ws` is that entry's workspace (it holds the bands'
        fp32 logits, about 4 M V bytes) and `logits` is None.  min_len, n-gram blocking and static bans:
        `init_beam_constraints(state, ...)` behind this call."""
        if state.vocab is None and state.adaptive is None:
            raise RuntimeError("init_beam_search needs a decoding state that holds the vocabulary table: "
                               "init_decoding(..., hold_vocab=True)")
        if state.sampler is not None:
            raise RuntimeError("init_beam_search on a state with a sampler: a beam search draws nothing")
        W, eos, max_new, len_penalty = int(beam_size), int(eos_idx), int(max_new), float(len_penalty)
        tables = None if state.adaptive is None else state.adaptive.tables
        M, V = int(state.options["batch_size"]), state.vocab.shape[0] if tables is None else tables.cutoff[-1]
        if not 1 <= W <= _BEAM_MAX_W:
            raise ValueError("beam_size must be in 1 .. %d, got %d" % (_BEAM_MAX_W, W))
        if M > _FUSED_MAX_ROWS or M % W:
            raise ValueError("beam_size %d on a state of %d rows: the batch size must be a multiple of beam_size and at most %d"
                             % (W, M, _FUSED_MAX_ROWS))
        if not 0 <= eos < V:
            raise ValueError("eos_idx must be in 0 .. %d, got %d" % (V - 1, eos))
        if max_new < 1:
            raise ValueError("max_new must be >= 1, got %d" % max_new)
        if not math.isfinite(len_penalty):
            raise ValueError("len_penalty must be finite, got %r" % len_penalty)
        from efficient_attention import _native as nv
        if tables is None:
            S, device = M // W, state.vocab.device
            nbytes = nv.lib().ea_ceva_sdecode_vocab_beam_ws(M, V, W)
        else:
            S, device = M // W, tables.device
            nbytes = nv.lib().ea_adaptive_beam_ws(M, len(tables.dims), *tables.host_arrays()[:2], W)

        def buf(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=device)
        i32, f32 = torch.int32, torch.float32
        state.beam = Beam(W, eos, max_new, len_penalty, buf((M, V), f32) if tables is None else None, buf(nbytes, torch.uint8),
                          buf(M, f32), buf(S, i32),
                          buf(S, i32), buf(S, i32), buf(M, torch.long), buf((max_new, M), i32), buf((max_new, M), i32),
                          buf((S, W), f32), buf((S, W), i32), buf((S, W), i32))
        return self.reset_beam_search(state)

    def init_beam_constraints(self, state, *, min_len=0, no_repeat_ngram_size=0, ban_tokens=(), prompt_cap=0):
        """Constrain the beam search of `state` (behind `init_beam_search`, at its start): fairseq's --min-len,
        --no-repeat-ngram-size and its ban on pad, decided on the device inside the step (ABI 36, include/ea_hip.h has the
        rule).  `min_len` (0 .. max_new - 1: no eos before that many tokens), `no_repeat_ngram_size` (0 .. 16: no n-gram of
        prompt ++ generated tokens ends twice), `ban_tokens` (at most 16 ids in [0, V), eos not among them: never picked) and
        `prompt_cap` (the longest prompt `set_beam_prompt` will be given: the prompt counts for the n-grams).  The forced step
        (the max_new-th token) ignores them all.  Values outside the envelope raise ValueError before anything is allocated.
        With all four at their defaults nothing is attached (a constraint the beam had is taken off) and the step is the
        unconstrained entry: the state is what `init_beam_search` left.  Otherwise `state.beam.constraint` (a BeamConstraint)
        holds the scalars with its buffers -- 4 S prompt_cap + 4 S bytes of prompt, 8 M max_new of generated tokens -- the
        Beam's `ws` becomes the constrained entry's (the ban list behind the step's: 4 M (prompt_cap + max_new + 18) bytes
        more, rounded), all counted by `decoding_state_nbytes`, and the step is ea_ceva_sdecode_vocab_beam_c /
        ea_adaptive_beam_c.  Returns the state."""
        bm = state.beam
        if bm is None:
            raise RuntimeError("init_beam_constraints needs a decoding state with a beam search: init_beam_search(state, ...)")
        tables = None if state.adaptive is None else state.adaptive.tables
        V = state.vocab.shape[0] if tables is None else tables.cutoff[-1]
        W, eos, max_new, M = bm.beam_size, bm.eos_idx, bm.max_new, bm.score.numel()
        min_len, ngram, prompt_cap = int(min_len), int(no_repeat_ngram_size), int(prompt_cap)
        bans = tuple(int(v) for v in ban_tokens)
        if not 0 <= min_len <= max_new - 1:
            raise ValueError("min_len must be in 0 .. max_new - 1 = %d, got %d" % (max_new - 1, min_len))
        if not 0 <= ngram <= tp.BAN_MAX_NGRAM:
            raise ValueError("no_repeat_ngram_size must be in 0 .. %d, got %d" % (tp.BAN_MAX_NGRAM, ngram))
        if len(bans) > tp.BAN_MAX_STATIC:
            raise ValueError("at most %d ban_tokens, got %d" % (tp.BAN_MAX_STATIC, len(bans)))
        for v in bans:
            if not 0 <= v < V or v == eos:
                raise ValueError("ban_tokens must lie in 0 .. %d and not hold eos_idx (%d), got %d" % (V - 1, eos, v))
        if prompt_cap < 0:
            raise ValueError("prompt_cap must be >= 0, got %d" % prompt_cap)
        constrained = bool(min_len or ngram or bans or prompt_cap)
        from efficient_attention import _native as nv
        S, device = M // W, bm.score.device
        if tables is None:
            nbytes = nv.lib().ea_ceva_sdecode_vocab_beam_c_ws(M, V, W, prompt_cap, max_new) if constrained \
                else nv.lib().ea_ceva_sdecode_vocab_beam_ws(M, V, W)
        else:
            geometry = (M, len(tables.dims), *tables.host_arrays()[:2], W)
            nbytes = nv.lib().ea_adaptive_beam_c_ws(*geometry, prompt_cap, max_new) if constrained \
                else nv.lib().ea_adaptive_beam_ws(*geometry)
        if nbytes < 0:
            raise ValueError("prompt_cap %d with max_new %d is outside the constrained step's envelope" % (prompt_cap, max_new))
        i32 = torch.int32
        bm.constraint = None
        if constrained:
            bm.constraint = tp.BeamConstraint(min_len, ngram, bans, prompt_cap,
                                              torch.zeros((S, prompt_cap), dtype=i32, device=device) if prompt_cap else None,
                                              torch.zeros(S, dtype=i32, device=device) if prompt_cap else None,
                                              torch.zeros((2, M, max_new), dtype=i32, device=device))
        if bm.ws.numel() != nbytes:
            bm.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return state

    def set_beam_prompt(self, state, prompt, lengths=None):
        """Tell a constrained beam search (`init_beam_constraints(state, ..., prompt_cap=P_max)`) the prompts its n-gram
        blocking counts: prompt [S, P] int64 or int32 with P <= prompt_cap, one row per sentence; lengths: None (every prompt has P tokens) or
        an integer [S] tensor of the prompts' lengths (right-padded rows; values are clamped to 0 .. P).  Device ops only; for
        callers who run their own loop around `beam_step` -- `beam_search` does it itself.  Returns the state."""
        bm = state.beam
        if bm is None or bm.constraint is None:
            raise RuntimeError("set_beam_prompt needs a beam search with constraints: init_beam_constraints(state, ..., prompt_cap=P)")
        c, S = bm.constraint, bm.t.numel()
        if prompt.dim() != 2 or prompt.shape[0] != S or prompt.dtype not in (torch.long, torch.int32):
            raise ValueError("prompt must be an integer [%d, P] tensor, got %s %s" % (S, prompt.dtype, tuple(prompt.shape)))
        P = prompt.shape[1]
        if P > c.prompt_cap:
            raise ValueError("a prompt of %d tokens on a beam search made with prompt_cap = %d" % (P, c.prompt_cap))
        if lengths is not None and (tuple(lengths.shape) != (S,) or lengths.dtype.is_floating_point):
            raise ValueError("lengths must be an integer [%d] tensor" % S)
        if c.prompt_cap == 0:
            return state
        c.prompt_tok.zero_()
        c.prompt_tok[:, :P].copy_(prompt)
        if lengths is None:
            c.prompt_len.fill_(P)
        else:
            c.prompt_len.copy_(lengths.clamp(0, P))
        return state

    def reset_beam_search(self, state):
        """Back to the start of a search, in place and by device ops only: score 0 for beam 0 of every sentence and -inf for
        the others, t = nfin = done = 0, the records and the history cleared; a constraint's generated tokens are cleared and
        its prompt is kept.  (The attention's own state is the caller's.)"""
        bm = state.beam
        if bm is None:
            raise RuntimeError("reset_beam_search needs a decoding state with a beam search: init_beam_search(state, ...)")
        bm.score.fill_(float("-inf")).view(-1, bm.beam_size)[:, 0].fill_(0.0)
        for t in (bm.t, bm.nfin, bm.done, bm.parent, bm.hist_tok, bm.hist_par, bm.fin_score, bm.fin_len, bm.fin_beam):
            t.zero_()
        if bm.constraint is not None:                                        # (the prompt stays: `set_beam_prompt`)
            bm.constraint.gen.zero_()
        return state

    def beam_step(self, rows, state, out=None, return_details=False):
        """One step of the beam search on a state with a beam (`init_beam_search`): rows [1, M, C] (final-layer rows of a
        single-token step, M the state's batch size) -> (tokens int64 [1, M], parent int64 [M]): the next input token of every
        beam and the row it continues -- `reorder_decoding_state(state, parent)` makes the state follow.  ONE call of
        ea_ceva_sdecode_vocab_beam (include/ea_hip.h has the rule): the table pass, a row's 2 W best candidates with their
        cumulative scores, the merge per sentence with the finished hypotheses and the history; everything it decides stays
        on the device, in the Beam's buffers (`parent` is one of them).  out: as in `next_tokens`.
        return_details=True: -> (tokens, parent, cand_idx int32 [M, 2 W], cand_score fp32 [M, 2 W], lse fp32 [M]); entries
        from min(2 W, V) on (the forced step: from 1 on) and the rows of a done sentence are not written.  Device launches
        only.  On a state with an adaptive pick: ONE call of ea_adaptive_beam; cand_idx are vocabulary indices, cand_score the
        cumulative joint log-probabilities, and the details end there (no single log-sum-exp exists)."""
        bm = state.beam
        if bm is None:
            raise RuntimeError("beam_step needs a decoding state with a beam search: init_beam_search(state, beam_size, ...)")
        T, M, C = rows.shape
        if T != 1 or M != bm.score.numel():
            raise ValueError("beam_step takes the rows of one single-token step of the whole state, [1, %d, C]; got %s"
                             % (bm.score.numel(), tuple(rows.shape)))
        return (tp.BeamStep if state.adaptive is None else tp.AdaptiveBeamStep)(self, state).run(rows, out, return_details)

    @staticmethod
    def _beam_hypotheses(bm):
        """The host's part of a search, behind the loop: the records and the history read back -> per sentence the finished
        hypotheses, the best normalised score first, ties by finishing order."""
        nfin, fin_score = bm.nfin.tolist(), bm.fin_score.cpu()
        fin_len, fin_beam = bm.fin_len.tolist(), bm.fin_beam.tolist()
        hist_tok, hist_par = bm.hist_tok.cpu(), bm.hist_par.cpu()
        W, result = bm.beam_size, []
        for s, n in enumerate(nfin):
            hyps = []
            for i in range(n):
                raw, length, b = fin_score[s, i], fin_len[s][i], fin_beam[s][i]
                tokens = [bm.eos_idx]
                for t in range(length - 2, -1, -1):
                    tokens.append(int(hist_tok[t, s * W + b]))
                    b = int(hist_par[t, s * W + b])
                hyps.append(dict(tokens=torch.tensor(tokens[::-1], dtype=torch.long), raw_score=raw,
                                 score=float(raw) / float(length) ** bm.len_penalty))
            order = sorted(range(n), key=lambda i: (not math.isnan(hyps[i]["score"]), -hyps[i]["score"], i))
            result.append([hyps[i] for i in order])
        return result

    def beam_search(self, prompt, state=None, *, beam_size, eos_idx, max_new, len_penalty=1.0, graph=True, poll=16):
        """Beam search: prompt [S, P] int64 -> per sentence a list of its finished hypotheses, the best first: dicts with
        `tokens` (int64 1-D, the closing eos included), `score` (raw_score / length ** len_penalty; ties by finishing order)
        and `raw_score` (an fp32 scalar tensor: the sum of the tokens' log-probabilities under the model's own distribution).
        At most beam_size per sentence; fewer where live beams ran out.  The rule -- fairseq's SequenceGenerator without
        prefix tokens and match_source_len, with ties decided and a -inf-scored eos dropped -- is in include/ea_hip.h (ABI 32).
        min_len, n-gram blocking and static bans (fairseq's --min-len, --no-repeat-ngram-size and its ban on pad; ABI 36) are
        `constrained_beam_search`'s keywords; this method runs them too on a state whose beam carries them
        (`init_beam_constraints`, prompt_cap >= P): it sets the prompt itself.  On an adaptive stack the state carries an adaptive pick instead of a held table
        (`init_adaptive_decoding`; the default state is made so) and the step is ea_adaptive_beam (ABI 35).
        state: a fresh DecodingState of S beam_size rows made with hold_vocab=True (default: rolling, held weights, the
        autocast dtype, P + max_new tokens); one without a beam gets `init_beam_search(state, beam_size, eos_idx, max_new,
        len_penalty)`, one with a beam must have been given the same four values and be at its start (`reset_beam_search`).
        The prompt is repeated beam_size times and fed eagerly in one `decode` (a per-sequence state: ragged, right-padded
        with `pad_idx`, as in `generate`); `beam_step` on the last rows and `reorder_decoding_state(state, parent)` follow.
        graph=True: then ONE step -- `decode` of the beams' tokens, `beam_step` writing the next tokens into the step's
        static input, the reorder by the parents it has just written; device ops only -- is warmed up on a scratch state and
        scratch beam buffers, captured, and replayed at most max_new - 1 times; every `poll` replays `done` is read back and
        the loop ends once every sentence is done.  graph=False runs the same steps eagerly: the same bits.  An overflow
        flagged by any layer raises after the loop."""
        return self._beam_search(prompt, state, beam_size, eos_idx, max_new, len_penalty, graph, poll, None)

    def constrained_beam_search(self, prompt, state=None, *, beam_size, eos_idx, max_new, len_penalty=1.0, graph=True, poll=16,
                                min_len=0, no_repeat_ngram_size=0, ban_tokens=()):
        """`beam_search` with fairseq's --min-len, --no-repeat-ngram-size and a list of tokens that are never picked (what
        fairseq does to pad): see `init_beam_constraints` for the three and include/ea_hip.h (ABI 36) for the rule.  They are
        decided on the device inside the step -- the captured step still replays without a host decision -- the prompt counts
        for the n-grams, and the forced step (the max_new-th token) ignores them.  Not built: prefix tokens (the prompt is
        prefilled) and match_source_len (no encoder).
        A state without a beam gets `init_beam_search` and `init_beam_constraints(prompt_cap=P)`; one with a beam must have
        been given the same values (and a prompt_cap >= P) and be at its start.  The prompt is set by this call: on a
        per-sequence state a ragged, right-padded prompt counts up to its first pad, as the prefill reads it.  The warm-up's
        scratch state gets the same constraints on buffers of its own.  With the three at their defaults this is `beam_search`.
        Everything else -- arguments, result, graph and poll -- is `beam_search`'s."""
        limits = (int(min_len), int(no_repeat_ngram_size), tuple(int(v) for v in ban_tokens))
        return self._beam_search(prompt, state, beam_size, eos_idx, max_new, len_penalty, graph, poll, limits)

    def _beam_search(self, prompt, state, beam_size, eos_idx, max_new, len_penalty, graph, poll, limits):
        """The search behind `beam_search` (limits None: the constraints the state's beam carries, if any) and
        `constrained_beam_search` (limits: (min_len, no_repeat_ngram_size, ban_tokens))."""
        if self.training:
            raise NotImplementedError("incremental decoding in training mode")
        S, P = prompt.shape
        W, max_new, poll = int(beam_size), int(max_new), int(poll)
        if poll < 1:
            raise ValueError("poll must be >= 1, got %d" % poll)
        M = S * W
        ctx, dtype = self._decoding_context()
        with torch.no_grad(), ctx:
            if state is None:
                if self.is_adaptive:
                    state = self.init_adaptive_decoding(self.init_decoding(M, P + max(max_new, 1), dtype, prompt.device))
                else:
                    state = self.init_decoding(M, P + max(max_new, 1), dtype, prompt.device, hold_vocab=True)
            if state.beam is None:
                self.init_beam_search(state, W, eos_idx, max_new, len_penalty)
                if limits is not None and any(limits):
                    self.init_beam_constraints(state, min_len=limits[0], no_repeat_ngram_size=limits[1], ban_tokens=limits[2],
                                               prompt_cap=P)
            bm = state.beam
            had = (0, 0, ()) if bm.constraint is None else bm.constraint.scalars()
            made = (bm.beam_size, bm.eos_idx, bm.max_new, bm.len_penalty)
            if made != (W, int(eos_idx), max_new, float(len_penalty)):
                raise ValueError("the state's beam search was made with (beam_size, eos_idx, max_new, len_penalty) = %r" % (made,))
            if limits is not None and had != limits:
                raise ValueError("the state's beam search was made with (min_len, no_repeat_ngram_size, ban_tokens) = %r" % (had,))
            if M != bm.score.numel():
                raise ValueError("a prompt of %d sentences at beam_size %d on a state of %d rows" % (S, W, bm.score.numel()))
            if bm.constraint is not None:                                    # (ragged prompts: the lengths `_prefill` reads)
                if P > bm.constraint.prompt_cap:
                    raise ValueError("a prompt of %d tokens on a beam search made with prompt_cap = %d" % (P, bm.constraint.prompt_cap))
                lengths = None
                if state.options["per_sequence"]:
                    lengths = P - prompt.eq(self.pad_idx).to(torch.int32).cumsum(1).ne(0).sum(1)
                self.set_beam_prompt(state, prompt, lengths)
            prompt = prompt.repeat_interleave(W, 0)                          # [M, P]: row s W + b is beam b of sentence s
            tok_in, parent = self.beam_step(self._prefill(prompt, state), state)     # [1, M]: the step's static input
            self.reorder_decoding_state(state, parent)

            def step(st):
                self.beam_step(self.decode(tok_in, st), st, out=tok_in)
                self.reorder_decoding_state(st, st.beam.parent)

            def scratch():                                                   # (the table is shared, the beam buffers are not)
                st = self.init_decoding(**dict(state.options, max_tokens=1, hold_vocab=False))
                st.vocab, st.vocab_ws, st.adaptive = state.vocab, state.vocab_ws, state.adaptive
                self.init_beam_search(st, W, eos_idx, max_new, len_penalty)
                if bm.constraint is None:
                    return st
                self.init_beam_constraints(st, min_len=had[0], no_repeat_ngram_size=had[1], ban_tokens=had[2],
                                           prompt_cap=bm.constraint.prompt_cap)
                if bm.constraint.prompt_cap:                                 # (the same constraints, on its own buffers)
                    st.beam.constraint.prompt_tok.copy_(bm.constraint.prompt_tok)
                    st.beam.constraint.prompt_len.copy_(bm.constraint.prompt_len)
                return st

            def each(i, _):
                bm.replays = i
                return i % poll == 0 and i + 1 < max_new and bool(bm.done.ne(0).all())
            bm.replays = 0
            self._run_steps(step, state, max_new, graph, tok_in, scratch, each=each)
            return self._beam_hypotheses(bm)

    def generate(self, prompt, n_new, state=None, graph=True, return_rows=False, return_logprobs=False):
        """Greedy decoding: prompt [B, P] int64 -> the n_new tokens that follow, [B, n_new] (return_rows: and the final-layer
        rows they were read from, [n_new, B, C]).  state: a fresh DecodingState of this stack (default: rolling, held weights,
        the autocast dtype).  The prompt is fed eagerly in one `decode`; on a per-sequence state it may be ragged and
        right-padded with `pad_idx`, and each row continues behind its own last token.
        graph=True: a warm-up step runs on a side stream, on a scratch state made with the same options, so that the state
        itself is untouched; then ONE single-token step -- embedding, layers, logits, argmax and the copy of the new token into
        the step's static input, device ops only -- is captured and replayed n_new - 1 times.  graph=False runs the same steps
        eagerly: the same tokens and rows bit for bit.  An overflow flagged by any layer raises after the loop.
        On a state made with hold_vocab both picks -- the first token's and the step's -- are `next_tokens`: the step ends in
        ea_ceva_sdecode_vocab_argmax, which reads the held 16-bit table once, picks on the fp32 sums and writes the token
        into the step's static input itself (no logits tensor, no argmax, no copy).  On any other state the path is unchanged.
        On a state with a sampler (`init_sampling`) both picks are `sample_tokens` instead: sampled, not greedy, decoding.  The
        warm-up's draw is undone -- the counters are saved before it and restored behind it -- so replayed and eager runs
        draw the same tokens.
        return_logprobs=True (a state with a scorer, `init_logprobs`; its absence is reported before the prefill): both picks
        run on ea_ceva_sdecode_vocab_logprob / ea_ceva_sdecode_vocab_sample_logprob instead and write each token's
        log-probability under the model's own distribution (temperature 1, nothing truncated) into the scorer's static
        buffer; -> (tokens[, rows], logp fp32 [B, n_new]).  The tokens are those of the same call without the keyword.
        On a state with an adaptive pick (`init_adaptive_decoding`) both picks are ea_adaptive_pick: the step ends in that
        kernel, which writes the token into the step's static input and its joint log-probability into
        `state.adaptive.logp`, where return_logprobs=True takes it from (no scorer needed).  With a sampler on such a state
        (`init_sampling`) both picks are ea_adaptive_sample: sampled decoding from the adaptive head, the drawn tokens' joint
        log-probabilities in the same buffer."""
        if self.training:
            raise NotImplementedError("incremental decoding in training mode")
        B, P = prompt.shape
        n_new = int(n_new)
        if n_new < 1:
            raise ValueError("generate needs n_new >= 1, got %d" % n_new)
        pick = tp.select_pick(self, state, B, return_logprobs)               # (what is not attached is reported here)
        ctx, dtype = self._decoding_context()
        with torch.no_grad(), ctx:
            if state is None:
                state = self.init_decoding(B, P + n_new, dtype, prompt.device, hold_weights=dtype != torch.float32)
            last = self._prefill(prompt, state)
            tok_in = pick(last)                                              # [1, B]: the step's static input
            out = torch.empty((B, n_new), dtype=torch.long, device=prompt.device)
            rows = torch.empty((n_new,) + tuple(last.shape[1:]), dtype=last.dtype, device=prompt.device) if return_rows else None
            logps = torch.empty((B, n_new), dtype=torch.float32, device=prompt.device) if return_logprobs else None

            def record(i, y):
                out[:, i] = tok_in[0]
                if rows is not None:
                    rows[i] = y[0]
                if logps is not None:
                    logps[:, i] = pick.logp[0]
            record(0, last)

            def step(st):                                                    # (the pick's table and workspaces are `state`'s)
                y = self.decode(tok_in, st)
                pick(y, out=tok_in)
                return y

            def scratch():
                return self.init_decoding(**dict(state.options, max_tokens=1, hold_vocab=False))
            self._run_steps(step, state, n_new, graph, tok_in, scratch, pick, record)
        if logps is not None:
            return (out, rows, logps) if return_rows else (out, logps)
        return (out, rows) if return_rows else out


def wikitext103_decoder(attn_args=None, vocab=32768, adaptive=None, **kw):
    """The decoder of the wikitext-103 recipe (transformer_lm_wiki103: 1024 / 4096 / 8 heads / 16 layers, pre-norm, no final
    decoder norm) around CausalEVAttention; attn_args default to the recipe's (window 128, chunks of 8, causal, adaptive 'qk',
    T5 bias).  adaptive=None: a plain tied embedding stands in for the recipe's adaptive input and adaptive softmax.
    adaptive=True (with vocab=267744, the recipe's dictionary): the recipe's own -- cutoffs 20000, 60000, factor 4, softmax
    dropout 0.2, weights and projections tied; a dict is handed to DecoderStack as it is."""
    if adaptive is True:
        adaptive = dict(cutoff=[20000, 60000], factor=4, dropout=0.2, tie_weights=True, tie_proj=True)
    if adaptive:
        kw["adaptive"] = adaptive
    if attn_args is None:
        attn_args = dict(window_size=128, chunk_size=8, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
                         overlap_window=False)
    return DecoderStack(vocab, 1024, 4096, 8, 16, attn_args, normalize_before=True, final_norm=False, **kw)
