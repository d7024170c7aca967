"""Incremental decoding of `CausalEVAttention` (reference causal_eva.py:537-665), as a mixin of the module.

A decoding step is append, close, attn, advance over a STATE, and the state says where the step starts and how a token
index becomes a cache row (csrc/ea_ceva_decode.hip).  There is one step body, `_decode`; the three kinds of state differ in

                      dynamic (fairseq's, grown on demand)     static / rolling (`init_*_decoding`, capturable)
    makes room        grow + slice-assign, on the host          ea_ceva_sdecode_append
    bias, fp32 mu     the module's DerivedCaches                the copies taken at init (a capture fixes the weights)
    entry points      ea_ceva_decode_* (t0, chunks from host)   ea_ceva_sdecode_* (t0 = *pos on the device)
    close             skipped when no chunk completes           always launched (its workgroups decide)
    count             host `attn_pos`, tensor `pos`             ea_ceva_sdecode_advance (+ host shadow, eager only)

and in nothing else.  A static or rolling state made with `per_sequence=True` keeps one count PER BATCH ROW (`pos [B]`): the
same four launches, each row taking its own number of the step's tokens (`_step_flags`), with no host shadow at all.
A static or rolling state made with `landmark_splits=P > 1` runs attn of a step of at most 8 tokens as two launches,
ea_ceva_sdecode_attn_split (P workgroups per window block share the landmark rows) and ea_ceva_sdecode_merge.
A static or rolling state made with `hold_projections=True` also HOLDS THE TWO PROJECTIONS, as 16-bit copies taken at init like
the bias table and the mu parameters: a step of at most 64 rows (T_new B) runs them as two more launches,
ea_ceva_sdecode_linear in front of append and behind advance, that stream the held weights once; no framework kernel of
such a step touches a weight.
A bf16 or fp16 static or rolling state made with `compact_landmarks=True` keeps its landmark rows (`rf_k_bar`, `beta`) in its
own dtype instead of fp32: close, attn and attn_split run as ea_ceva_sdecode_close_l16, _attn_l16 and _attn_split_l16, which
round the two rows of a closed chunk once and read them as they read key and value rows; the arithmetic stays fp32.
"""
import ctypes
import functools
import inspect
import numbers

import torch

from . import _ops
from . import _f32

_NEEDS_CHUNK_SIZE = ("incremental decoding needs --chunk-size (with --num-chunks the chunk length depends on the final "
                     "sequence length)")
# the buffers of a static state that a beam reorder permutes; a rolling state has the same (its ring slots are per batch
# element, the token count `pos` is shared); a per-sequence state adds its per-row counters
_STATIC_BATCH_FIRST = ("qkv", "rf_k_bar", "beta", "pad")
_PER_SEQUENCE = ("pos", "status", "ntok")
_SPLIT_MAX_STEP = 8          # QPW of ea_ceva_decode.hip: a step of at most this many tokens has one query group per window block
_SPLIT_MAX_PARTS = 64
_LINEAR_MAX_ROWS = 64        # EA_CEVA_LINEAR_MAX_ROWS of include/ea_hip.h: the rows (T_new B) ea_ceva_sdecode_linear takes
# what a state made with hold_projections=True adds to the buffer (step-invariant like `bias` and `mu`: a beam reorder and
# reset_decoding_rows leave them alone)
_HELD = ("w_qkv", "b_qkv", "w_out", "b_out", "proj_rows")


def _state_options(init):
    """The keyword-only `per_sequence=False`, `landmark_splits=1`, `hold_projections=False` and `compact_landmarks=False` of
    the two `init_*_decoding` methods.  The methods keep
    the positional interface they had, and that is the signature they report (`__signature__`: callers that pin the parameter
    list, this package's own tests among them, see what they saw); the options are taken off here and handed to the method
    as its last arguments.  Arguments are bound as Python binds them: an option by position, or an unknown keyword, is a
    TypeError.  (`landmark_splits` is handed on as given: the method checks it behind its other refusals.)"""
    positional = inspect.signature(init)
    positional = positional.replace(parameters=list(positional.parameters.values())[:-4])

    @functools.wraps(init)
    def with_options(self, *args, per_sequence=False, landmark_splits=1, hold_projections=False, compact_landmarks=False,
                     **kwargs):
        bound = positional.bind(self, *args, **kwargs)
        bound.apply_defaults()
        return init(*bound.args, bool(per_sequence), landmark_splits, bool(hold_projections), bool(compact_landmarks),
                    **bound.kwargs)
    with_options.__signature__ = positional
    return with_options


def _check_landmark_splits(P):
    if isinstance(P, bool) or not isinstance(P, numbers.Integral) or not 1 <= P <= _SPLIT_MAX_PARTS:
        raise ValueError("landmark_splits must be an int in [1, %d], got %r" % (_SPLIT_MAX_PARTS, P))
    return int(P)


class CevaDecoding:
    def _refuse_decoding(self):
        """The cases incremental decoding does not define, dynamic and static state alike."""
        if not self.self_attention:
            raise NotImplementedError("incremental decoding of encoder-decoder attention")
        if not self.causal:
            raise NotImplementedError("incremental decoding needs --causal: without the causal masks every query of the "
                                      "training path sees the landmarks of future chunks (causal_eva.py:716-738)")
        if self.training:
            raise NotImplementedError("incremental decoding in training mode")
        if self.adaptive_proj not in ("qk", "no-ln"):
            raise NotImplementedError("Other adaptive projection methods are not implemented yet.")

    # ---- what a step reads besides the cache: built here for both kinds of state ---------------------------------------
    def _decode_bias_table(self, device):
        """The dense single-head [w, w + e] T5 table (already scaled), or None."""
        if not self.use_t5_rpe:
            return None
        return self.rel_pos_bias.dense(self.window_size, self.window_size + self.ext_size, device)[0].contiguous()

    def _decode_mu_f32(self):
        """The close kernel reads fp32 parameters: fp32 masters pass through, a module converted with .half() / .bfloat16()
        (fairseq's 16-bit generation) hands over fp32 copies, as the full path's _f32c does."""
        return [_ops._f32c(p) for p in self._mu_params()]

    # ---- static and rolling states ----------------------------------------------------------------------------------------
    @_state_options
    def init_static_decoding(self, incremental_state, batch_size, max_tokens, dtype, device, per_sequence=False,
                             landmark_splits=1, hold_projections=False, compact_landmarks=False):
        """Allocate, once, every buffer a decoding step touches and mark this module's incremental state as STATIC: every
        later `forward(..., incremental_state=incremental_state)` then runs a step that can be captured into a graph
        (`torch.cuda.graph`) and replayed -- the token count lives in device memory and the kernels advance it: four
        launches of the attention core (ea_ceva_sdecode_append, _close, _attn, _advance) that read the token count from
        `pos`, no allocation but the step's own outputs, no read-back, no host counter a replay would need.  The arithmetic
        is the dynamic step's, so the outputs equal its outputs bit for bit.
        State, allocated here (cap = ceil(max_tokens / w) w):
            qkv       [B, cap, 3, h, d]   `dtype` (bf16, fp16, or fp32 when the fp32 cores are enabled)
            rf_k_bar  [B, h, cap / r, d]  fp32
            beta      [B, h, cap / r, d]  fp32
            pad       [B, cap]            uint8, zeros
            pos       [1]                 int32 on the device: tokens decoded so far
            status    [1]                 int32 on the device: 1 once a step would have passed cap
            bias, mu                      the dense T5 table and fp32 copies of the mu parameters, built here once (a
                                          capture fixes the weights)
        A step's token count and the batch are fixed for a given capture; the prompt can go through the same state eagerly.
        Refuses what dynamic decoding refuses, with the same messages, and CPU devices (there is no CPU fallback).
        `per_sequence=True`: every batch row has its own token count, so that ragged prompts need no left padding (which
        would shift a row's chunk and window boundaries) and a finished row can be restarted while the others go on:
            pos       [B]                 int32: tokens decoded so far, per row
            status    [B]                 int32: 1 once a step of that row would have passed cap
            ntok      [B]                 int32: the tokens each row took from the last step (written by the step)
        and every other buffer as above.  A row's share of a step is given by the step's `key_padding_mask`: of its last
        T_new columns, row b's tokens are the positions BEFORE ITS FIRST FLAGGED ONE, n_b of them (0 <= n_b <= T_new; no
        mask: all T_new).  They are appended at pos[b] .. pos[b] + n_b - 1 and pos[b] advances by n_b; nothing is stored
        for the flagged positions (no cache row, pad flag or landmark slot), and the attention core delivers zero rows for
        them, so the module returns out_proj of zero there.  Right-padded ragged prompts, and a row that sits a step out
        (all flagged), are the two uses.  The host does not know the counts: a step makes no host-side capacity check,
        and overflow is per row -- a row whose step would pass cap writes nothing, gets status[b] = 1 and NaN output rows
        and keeps its count, the other rows of the step are unaffected (`static_decoding_overflowed_rows`).  With equal
        counts and no mask the outputs and the state equal those of the shared count bit for bit.
        `reset_decoding_rows` restarts rows; `decoding_positions` reads the counts back.
        `landmark_splits=P` (an int in [1, 64], default 1; combines with `per_sequence`): a step's attn launch runs one
        workgroup per (window block, b, h) and streams every landmark row of the context through it, so a 1-token step at a
        long context and a small batch keeps B h of the device's 256 compute units busy and is bound by the latency of one.
        With P > 1 a step of AT MOST 8 TOKENS (the single-token step, a short verify step) takes five launches instead:
        append, close, ea_ceva_sdecode_attn_split -- P workgroups per (window block, b, h) share the 64-column tiles of
        [local keys, landmarks] and write unnormalised (max, sum, acc) partials -- ea_ceva_sdecode_merge, advance.  A larger
        step (a prompt, and every piece a rolling state cuts it into) keeps the four launches: its many queries already give
        it workgroups.  The choice depends on the step's token count alone, which a capture fixes.  The state holds one more tensor,
            split_ws  [B, h, 8, P, d + 4] fp32: the partials of one step, allocated here so that a captured step allocates
                                          nothing; scratch, fully rewritten by every step that reads it (a beam reorder and
                                          `reset_decoding_rows` leave it alone; `decoding_state_nbytes` counts it).
        Choosing P: about 256 / (B h) workgroups per (b, h) fill the device (B = 1, h = 8: 32; B = 8, h = 8: 4); more parts
        than the context has 64-landmark tiles, ceil(tokens / (64 r)) of them, buy nothing, and at a short context the
        extra launch costs more than the split saves.  The split changes the order in which a row's partial sums are merged,
        so its outputs equal the unsplit step's to rounding, not bit for bit; P = 1 is the unsplit state in every respect.
        `hold_projections=True` (default False; combines with the other two; a 16-bit `dtype` only -- fp32 decoding is the
        fidelity path and keeps the library's fp32 GEMMs -- and projections that all have a bias or all have none): the state
        also holds the module's two projections, taken here once like the bias table and the mu parameters (a capture fixes
        the weights):
            w_qkv     [3 C, C]            `dtype`: q_proj, k_proj, v_proj weights stacked in that order
            b_qkv     [3 C]               `dtype`, or None without biases
            w_out     [C, C]              `dtype`: out_proj
            b_out     [C]                 `dtype`, or None
            proj_rows [64, 3 C]           `dtype`: the projected rows of a step, so that a captured step allocates only its
                                          outputs; scratch like split_ws
        A plain step rebuilds the stacked weight and casts both weights from the fp32 masters every time it is replayed (a
        capture must record the producing kernels): about 56 MB of weight traffic and a dozen launches per layer at C = 1024
        for a step whose inputs are 1 .. 8 rows.  On a held state a step of AT MOST 64 ROWS (T_new B) is
            ea_ceva_sdecode_linear (query rows -> proj_rows), append, close, attn (or attn_split + merge), advance,
            ea_ceva_sdecode_linear (attention rows -> the output)
        -- the 8 MB of 16-bit weights read once, by a kernel that multiplies a handful of rows at the speed the weight can be
        read, and no framework kernel that touches a weight.  The query is rounded to `dtype` as it is loaded (an fp32 query
        outside autocast: with the one-time rounding warning), products are summed in fp32 and rounded once; the output has
        the dtype the plain step returns.  A larger step (a prompt; every piece a rolling state cuts it into) runs the library
        GEMM on the held operands: no concatenation and no cast of a weight either.  Outputs equal the plain state's to
        rounding (16-bit weights, another summation order), not bit for bit.  After the parameters have changed,
        `refresh_decoding_weights` re-reads them in place.
        `compact_landmarks=True` (default False; combines with the other three; a 16-bit `dtype` only -- the fp32 state is
        the fidelity path and has nothing to compact): the landmark rows are kept in the state's dtype,
            rf_k_bar  [B, h, cap / r, d]  `dtype`
            beta      [B, h, cap / r, d]  `dtype`
        which halves them -- at h = 8, d = 128, r = 8 and 32k tokens they are 33.5 MB of a 35 MB state in fp32 -- and halves
        what a single-token step at a long context reads.  A step runs ea_ceva_sdecode_close_l16 and ea_ceva_sdecode_attn_l16
        (or ea_ceva_sdecode_attn_split_l16 + merge) in place of their twins, for steps, prompt pieces and captured steps alike;
        append, merge and advance are the same launches.  close computes what it computes on a plain state, in fp32 and in the
        same order -- mu and beta from the unrounded rf_k_bar -- and rounds only the two rows it stores, once, to nearest even:
        the landmark rows of a compact state are the plain state's rows rounded, bit for bit.  attn widens them as it widens key
        and value rows, so the outputs differ from the plain state's by that one rounding of the landmark operands (about 5e-3
        of the largest output for bf16, 1e-3 for fp16, on N(0, 1) operands) and are equal bit for bit while no landmark is
        visible.  The token rows, pad flags and counters are those of the plain state.  The other methods need nothing
        beyond what the dtype carries: `reorder_incremental_state` copies rows of whatever type, `reset_decoding_rows`,
        `decoding_positions` and the overflow queries read no landmark row, `refresh_decoding_weights` touches none, and
        `decoding_state_nbytes` counts the bytes the tensors have."""
        B, T, device = self._check_static_decoding(batch_size, max_tokens, dtype, device)
        P = _check_landmark_splits(landmark_splits)
        self._check_hold_projections(hold_projections, dtype)
        self._check_compact_landmarks(compact_landmarks, dtype)
        w = self.window_size
        cap = -(-T // w) * w
        return self._alloc_static_decoding(incremental_state, B, cap, cap, dtype, device, {"count": 0}, per_sequence, P,
                                           hold_projections, compact_landmarks)

    @_state_options
    def init_rolling_decoding(self, incremental_state, batch_size, max_tokens, dtype, device, max_step_tokens=None,
                              per_sequence=False, landmark_splits=1, hold_projections=False, compact_landmarks=False):
        """`init_static_decoding` with the token rows in a fixed RING: the state is static in every respect (the same step,
        capturable and replayable; `static_decoding_overflowed` and the in-place `reorder_incremental_state` work on it), but
        `qkv` and `pad` hold R token slots instead of one row per token ever decoded, token n in slot n % R:
            qkv       [B, R, 3, h, d]     `dtype`
            pad       [B, R]              uint8
            rf_k_bar  [B, h, cap / r, d]  fp32   } linear, as in the static state: cap = ceil(max_tokens / w) w bounds
            beta      [B, h, cap / r, d]  fp32   } only the landmark rows (and `pos`); `dtype` with compact_landmarks
            pos, status, bias, mu         as in the static state
        S = `max_step_tokens` (default w) is the largest step one launch sequence may hold, and R is the smallest multiple
        of w with R >= w + e + S.  Why that is enough: a step of T <= S tokens that starts at token t0 reads the local keys /
        values of tokens >= floor(t0 / w) w - e (the window block of its first token with its left extension), the rows of
        the chunks it closes (inside those blocks, r divides w) and its own rows, and writes rows t0 .. t0 + T - 1.  From
        the earliest token read to the last one written that is at most (w - 1) + e + S tokens, fewer than R, so the rows it
        appends overwrite only tokens older than the earliest one it reads.  R does not depend on `max_tokens`.  A ring is
        never larger than the linear cache would be: with R >= cap the layout is the linear one (R = cap, no wrap).
        A step with more than S tokens (a prompt) is fed through the ring by the module itself, eagerly, in consecutive
        pieces of at most S tokens, each an ordinary static step; while a stream is capturing it raises instead.
        Arithmetic and its order are the static step's: for one sequence of step sizes the outputs equal bit for bit.
        Refuses what `init_static_decoding` refuses, with the same messages, and `max_step_tokens <= 0`.
        `per_sequence=True`: per-row counts as in `init_static_decoding`; every row walks its own ring.  The pieces of a long
        ragged prompt carry the matching slices of the (monotone) mask, so a row that ended in one piece takes nothing from
        the later ones.
        `landmark_splits=P`: as in `init_static_decoding` -- the landmark rows, which a rolling state keeps for the whole
        context, are what a step of at most 8 tokens shares between P workgroups per (window block, b, h).  About
        256 / (B h) parts fill the device; more than ceil(tokens / (64 r)) buy nothing.
        `hold_projections=True`: as in `init_static_decoding` -- the state holds 16-bit copies of the two projections (a capture
        fixes the weights; `refresh_decoding_weights` re-reads them), a step of at most 64 rows runs them on
        ea_ceva_sdecode_linear, and the pieces of a prompt run the library GEMM on the held operands.
        `compact_landmarks=True`: as in `init_static_decoding` -- a bf16 or fp16 state keeps `rf_k_bar` and `beta` in its own
        dtype, the plain state's rows rounded once, and its steps run the `_l16` entry points.  The landmark rows are nearly
        all of a rolling state at a long context (33.5 of 35 MB per layer and sequence at 32k tokens, h = 8, d = 128, r = 8),
        so the option about halves it."""
        B, T, device = self._check_static_decoding(batch_size, max_tokens, dtype, device)
        w, e = self.window_size, self.ext_size
        S = w if max_step_tokens is None else int(max_step_tokens)
        if S <= 0:
            raise ValueError("rolling decoding needs max_step_tokens > 0, got %d" % S)
        P = _check_landmark_splits(landmark_splits)
        self._check_hold_projections(hold_projections, dtype)
        self._check_compact_landmarks(compact_landmarks, dtype)
        cap = -(-T // w) * w
        ring = -(-(w + e + S) // w) * w
        rows = min(ring, cap)
        static = {"count": 0, "cap": cap, "ring": ring if ring < cap else 0, "max_step": S}
        return self._alloc_static_decoding(incremental_state, B, cap, rows, dtype, device, static, per_sequence, P,
                                           hold_projections, compact_landmarks)

    @staticmethod
    def _check_compact_landmarks(compact, dtype):
        """What `compact_landmarks=True` refuses, behind every other refusal and before anything is allocated."""
        if compact and dtype == torch.float32:
            raise ValueError("compact_landmarks=True keeps the landmark rows in the state's 16-bit dtype: an fp32 decoding "
                             "state is the fidelity path and has nothing to compact")

    def _check_hold_projections(self, hold, dtype):
        """What `hold_projections=True` refuses, behind every other refusal and before anything is allocated."""
        if not hold:
            return
        if dtype == torch.float32:
            raise ValueError("hold_projections=True holds 16-bit projection weights: an fp32 decoding state (the fidelity "
                             "path) keeps the library's fp32 GEMMs")
        has_b = [lin.bias is not None for lin in (self.q_proj, self.k_proj, self.v_proj)]
        if any(has_b) != all(has_b):
            raise ValueError("hold_projections=True needs q_proj, k_proj and v_proj to all have a bias or all have none")

    def _check_static_decoding(self, batch_size, max_tokens, dtype, device):
        """What a static (or rolling) state refuses, before anything is allocated -> (B, max_tokens, device)."""
        self._refuse_decoding()
        if self.chunk_size is None:
            raise NotImplementedError(_NEEDS_CHUNK_SIZE)
        if dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError("static decoding caches bf16, fp16 or fp32 rows, not %s" % (dtype,))
        if dtype == torch.float32 and not _f32.ENABLED:
            raise ValueError("an fp32 static decoding cache needs the fp32 cores (EA_F32_CORES=1)")
        device = torch.device(device)
        _ops.nv.require_cuda(torch.empty(0, device=device), "the static decoding state")
        B, T = int(batch_size), int(max_tokens)
        if B <= 0 or T <= 0:
            raise ValueError("static decoding needs batch_size > 0 and max_tokens > 0, got %d, %d" % (B, T))
        return B, T, device

    def _alloc_static_decoding(self, incremental_state, B, cap, rows, dtype, device, static, per_sequence=False, splits=1,
                               hold=False, compact=False):
        """The buffers of a static state: `rows` token rows (cap, or a ring), cap / r landmark rows (fp32; compact: `dtype`);
        one counter and one overflow flag, or (per_sequence) one of each per batch row and the rows' token counts of a step;
        splits > 1: the workspace of a short step's partials; hold: the 16-bit projections and the staging rows of a step."""
        h, d, r = self.num_heads, self.head_dim, self.chunk_size
        nc = B if per_sequence else 1
        ldtype = dtype if compact else torch.float32
        state = {
            "qkv": torch.zeros((B, rows, 3, h, d), dtype=dtype, device=device),
            "rf_k_bar": torch.zeros((B, h, cap // r, d), dtype=ldtype, device=device),
            "beta": torch.zeros((B, h, cap // r, d), dtype=ldtype, device=device),
            "pad": torch.zeros((B, rows), dtype=torch.uint8, device=device),
            "pos": torch.zeros((nc,), dtype=torch.int32, device=device),
            "status": torch.zeros((nc,), dtype=torch.int32, device=device),
        }
        if per_sequence:
            state["ntok"] = torch.zeros((B,), dtype=torch.int32, device=device)
            static["per_sequence"] = True
        static["landmark_splits"] = splits
        if splits > 1:
            state["split_ws"] = torch.zeros((B, h, _SPLIT_MAX_STEP, splits, d + 4), dtype=torch.float32, device=device)
        if hold:
            C = self.embed_dim
            qkv_b, out_b = self.q_proj.bias is not None, self.out_proj.bias is not None
            state["proj_rows"] = torch.zeros((_LINEAR_MAX_ROWS, 3 * C), dtype=dtype, device=device)
            state["w_qkv"] = torch.empty((3 * C, C), dtype=dtype, device=device)
            state["b_qkv"] = torch.empty((3 * C,), dtype=dtype, device=device) if qkv_b else None
            state["w_out"] = torch.empty((C, C), dtype=dtype, device=device)
            state["b_out"] = torch.empty((C,), dtype=dtype, device=device) if out_b else None
            static["hold_projections"] = True
        if compact:
            static["compact_landmarks"] = True
        with torch.no_grad():
            state["bias"] = self._decode_bias_table(device)
            state["mu"] = self._decode_mu_f32()
        if hold:
            self._load_held_projections(state)
        self._set_input_buffer(incremental_state, state)
        # host side: the shadow count of EAGER steps (a replay advances only the device count), for the eager overflow check;
        # a rolling state adds its landmark capacity, its ring length (0: linear rows) and its largest step
        self.set_incremental_state(incremental_state, "attn_static", static)
        return incremental_state

    def _load_held_projections(self, state):
        """The module's projection parameters -> the held 16-bit tensors, in place (rounded to nearest even, the values
        `multi_cast` produces); rows of w_qkv: q_proj, k_proj, v_proj, as `_project` stacks them.  Device copies only."""
        C = self.embed_dim
        with torch.no_grad():
            for i, lin in enumerate((self.q_proj, self.k_proj, self.v_proj)):
                state["w_qkv"][i * C:(i + 1) * C].copy_(lin.weight)
                if state["b_qkv"] is not None:
                    state["b_qkv"][i * C:(i + 1) * C].copy_(lin.bias)
            state["w_out"].copy_(self.out_proj.weight)
            if state["b_out"] is not None:
                state["b_out"].copy_(self.out_proj.bias)

    def refresh_decoding_weights(self, incremental_state):
        """Re-read the module's parameters into what a static or rolling state holds of them, IN PLACE: the dense bias table,
        the fp32 copies of the mu parameters (fp32 masters are read where they are and need none) and, on a state made with
        `hold_projections=True`, the 16-bit projection weights and biases.  A capture fixes the weights -- a replayed step
        reads these tensors, not the parameters -- so call this after the parameters have changed (an optimizer step, a loaded
        checkpoint) and between replays: device ops only, every `data_ptr()` stays what it was, and a step captured before
        sees the new weights without being captured again.  A state without held projections refreshes what it holds."""
        buf, _ = self._static_buffer(incremental_state, "refresh_decoding_weights")
        with torch.no_grad():
            if buf.get("bias") is not None:
                buf["bias"].copy_(self._decode_bias_table(buf["bias"].device))
            for held, param in zip(buf["mu"], self._mu_params()):
                if held.data_ptr() != param.data_ptr():
                    held.copy_(param)
        if "w_qkv" in buf:
            self._load_held_projections(buf)
        return incremental_state

    def decoding_state_nbytes(self, incremental_state):
        """Bytes of every tensor in this module's decoding buffer (dynamic, static or rolling): token rows, pad flags,
        landmark rows (fp32, or 16-bit on a state made with `compact_landmarks=True`), counters and, for a static state, the bias table, the fp32 mu parameters it holds, the workspace
        of `landmark_splits` and what `hold_projections` holds.  Host only."""
        def nbytes(v):
            if torch.is_tensor(v):
                return v.numel() * v.element_size()
            if isinstance(v, (list, tuple)):
                return sum(nbytes(x) for x in v)
            return 0
        return sum(nbytes(v) for v in self._get_input_buffer(incremental_state).values())

    def static_decoding_overflowed(self, incremental_state):
        """True once a step on this static state would have passed its capacity (the step wrote nothing; its outputs are
        NaN).  Reads the device flag back: call it after a replay, not inside a captured step."""
        status = self._get_input_buffer(incremental_state)["status"]
        return bool(status.item() if status.numel() == 1 else status.any().item())      # (per-sequence: any row)

    def _static_buffer(self, incremental_state, what):
        """(buffer, host dict) of a static or rolling state, or a clear error."""
        static = self.get_incremental_state(incremental_state, "attn_static")
        buf = self._get_input_buffer(incremental_state)
        if static is None or not buf or "pos" not in buf:
            raise RuntimeError("%s needs a static or rolling decoding state (init_static_decoding / "
                               "init_rolling_decoding); this incremental state holds none" % what)
        return buf, static

    def static_decoding_overflowed_rows(self, incremental_state):
        """The overflow flags per batch row, a [B] bool tensor on the host (a shared-count state: its one flag repeated).
        Reads the device flags back: call it after a replay, not inside a captured step."""
        buf, _ = self._static_buffer(incremental_state, "static_decoding_overflowed_rows")
        return buf["status"].ne(0).expand(buf["qkv"].shape[0]).cpu()

    def decoding_positions(self, incremental_state):
        """The tokens decoded so far per batch row, a [B] int32 copy on the host (a shared-count state: its one count
        repeated).  Reads the device counts back: call it after a replay, not inside a captured step."""
        buf, _ = self._static_buffer(incremental_state, "decoding_positions")
        return buf["pos"].expand(buf["qkv"].shape[0]).cpu().clone()

    def decoding_positions_tensor(self, incremental_state):
        """The DEVICE tensor a static or rolling state counts in -- `pos [1]` int32, or `[B]` on a per-sequence state -- itself,
        not a copy: no read-back, so a captured step may index with it (the positions of a decoder's new tokens); the steps
        advance it.  Raises on a dynamic state, as `decoding_positions` does."""
        buf, _ = self._static_buffer(incremental_state, "decoding_positions_tensor")
        return buf["pos"]

    def reset_decoding_rows(self, incremental_state, rows):
        """Restart batch rows of a per-sequence state: `pos` and `status` of `rows` (indices: a sequence of ints or an
        integer tensor) back to 0, in place and by device ops only -- between replays, or captured itself when `rows` is a
        device tensor.  It clears no cache: nothing at or past a row's count is ever read, so the next tokens of that row
        are those of a new sequence whatever the row held."""
        buf, static = self._static_buffer(incremental_state, "reset_decoding_rows")
        if not static.get("per_sequence"):
            raise RuntimeError("reset_decoding_rows needs a per-sequence state (init_*_decoding(per_sequence=True)): "
                               "this state has one token count for the whole batch")
        idx = torch.as_tensor(rows, device=buf["pos"].device).reshape(-1).long()
        buf["pos"].index_fill_(0, idx, 0)
        buf["status"].index_fill_(0, idx, 0)
        return incremental_state

    def reorder_incremental_state(self, incremental_state, new_order):
        """Permute the batch rows of this module's decoding buffer.  A static or rolling state: `qkv`, `rf_k_bar`, `beta`, `pad`
        (and the per-row counters of a per-sequence state), in place; the landmark rows are copied in the type they have, fp32
        or the 16 bits of a compact state."""
        buf = self._get_input_buffer(incremental_state)
        if buf and self.get_incremental_state(incremental_state, "attn_static") is not None:
            # a static state reorders IN PLACE: the pointers a captured step holds stay valid, and the reorder can itself
            # be captured (pos, status and the step-invariant tensors are not per element)
            static = self.get_incremental_state(incremental_state, "attn_static")
            for k in _STATIC_BATCH_FIRST + (_PER_SEQUENCE if static.get("per_sequence") else ()):
                buf[k].copy_(buf[k].index_select(0, new_order))
            return incremental_state
        if buf:
            for k, t in buf.items():
                if t is not None:
                    buf[k] = t.index_select(0, new_order)
            incremental_state = self._set_input_buffer(incremental_state, buf)
        return incremental_state

    # ---- how each kind of state makes room for a step -------------------------------------------------------------------------
    def _static_room(self, state, static, T_new, B):
        """A static step's host checks -> (capturing, pieces): `pieces` is the piece length when a rolling state must be fed
        the step in consecutive pieces (a prompt above its `max_step_tokens`; eager only), else None."""
        cache = state["qkv"]
        cap, max_step = static.get("cap", cache.shape[1]), static.get("max_step")
        if cache.shape[0] != B:
            raise RuntimeError("static decoding state holds batch %d, the step has %d" % (cache.shape[0], B))
        capturing = torch.cuda.is_current_stream_capturing()
        # (a per-sequence state: the host does not know the counts, overflow is reported by the device flags only)
        if not capturing and not static.get("per_sequence") and static["count"] + T_new > cap:
            raise RuntimeError("static decoding state is full: %d of its %d tokens decoded, the step adds %d "
                               "(%s(max_tokens=...))" % (static["count"], cap, T_new, "init_static_decoding"
                                                         if max_step is None else "init_rolling_decoding"))
        if max_step is None or T_new <= max_step:
            return capturing, None
        if capturing:
            raise RuntimeError("a captured step of %d tokens does not fit the rolling decoding state: max_step_tokens "
                               "is %d (init_rolling_decoding(max_step_tokens=...))" % (T_new, max_step))
        return capturing, max_step

    def _dynamic_room(self, incremental_state, state, dtype, B, T_new, dev):
        """The dynamic state: created by the first step (which fixes the cache's dtype), doubled when the step passes it
        -> t0.  The token count also lives on the host, under its own key of the incremental state -- reading `pos` back
        would synchronise every step, and reorder_incremental_state only touches the tensors of the buffer."""
        w, h, d, r = self.window_size, self.num_heads, self.head_dim, self.chunk_size
        if "qkv" not in state:
            cap = max(2 * w, 64)
            state["qkv"] = torch.zeros((B, cap, 3, h, d), dtype=dtype, device=dev)
            lcap = max(cap // r, 1)
            state["rf_k_bar"] = torch.zeros((B, h, lcap, d), dtype=torch.float32, device=dev)
            state["beta"] = torch.zeros((B, h, lcap, d), dtype=torch.float32, device=dev)
            state["pos"] = torch.zeros((B,), dtype=torch.long, device=dev)
            state["pad"] = torch.zeros((B, cap), dtype=torch.uint8, device=dev)
            self.set_incremental_state(incremental_state, "attn_pos", 0)
            self.set_incremental_state(incremental_state, "attn_has_pad", False)
        t0 = int(self.get_incremental_state(incremental_state, "attn_pos") or 0)
        if state["qkv"].shape[0] != B:
            raise RuntimeError("incremental state holds batch %d, the step has %d" % (state["qkv"].shape[0], B))
        need = ((t0 + T_new + w - 1) // w) * w
        if need > state["qkv"].shape[1]:
            cap = max(need, 2 * state["qkv"].shape[1])

            def grown(t, dim, n):                                  # zeros, n long in `dim`, that start with t
                g = torch.zeros(t.shape[:dim] + (n,) + t.shape[dim + 1:], dtype=t.dtype, device=dev)
                g.narrow(dim, 0, t.shape[dim]).copy_(t)
                return g
            state["qkv"], state["pad"] = grown(state["qkv"], 1, cap), grown(state["pad"], 1, cap)
            state["rf_k_bar"], state["beta"] = grown(state["rf_k_bar"], 2, cap // r), grown(state["beta"], 2, cap // r)
        return t0

    @staticmethod
    def _step_flags(key_padding_mask, T_new):
        """A per-sequence step's flags [B, T_new], made monotone along the step: a position after a flagged one counts as
        flagged, so a row's tokens are the positions before its first flag however a rolling state cuts the step into
        pieces.  A device op, no read-back."""
        if key_padding_mask is None:
            return None
        return key_padding_mask[:, -T_new:].ne(0).to(torch.int32).cumsum(1).ne(0)

    # ---- the step -------------------------------------------------------------------------------------------------------------
    def _decode(self, query, key_padding_mask, incremental_state, piece=False):
        """Token-by-token decoding with fairseq's incremental state.

        The reference's branch for this (causal_eva.py:537-665) cannot run as shipped -- `N` and `B` are bound only when
        `incremental_state is None` (:503-509), so any call with a state raises -- and what it sketches (a sliding window of
        the last `window_size` keys) would not agree with the module's own training path (block windows with a left
        extension).  This build therefore defines decoding by PREFIX CONSISTENCY with the pinned full-sequence path: the
        output for token t equals row t of `forward()` on the tokens 0..t (tests/test_gpu_causal_eva.py).  The dynamic
        state, all batch-first so that `reorder_incremental_state` can index it:
            qkv       [B, cap, 3, h, d]   projected rows of every token so far (16-bit, or fp32 outside autocast; the
                                          window needs the last w + e, a chunk its own rows)
            rf_k_bar  [B, h, Lcap, d]     fp32, the landmark keys of the COMPLETED chunks (:588-634)
            beta      [B, h, Lcap, d]     fp32, their control variates
            pos       [B]                 tokens decoded so far
            pad       [B, cap]            uint8, 1 = padded position (`key_padding_mask`, e.g. left-padded prompts of a batch):
                                          handed to the kernels exactly as the full path hands them its mask -- a padded key
                                          is invisible, a padded query sees no local key, a chunk's means skip its padded rows
        A step projects its tokens (fp32 stays fp32 outside autocast when the fp32 cores are usable: the cache dtype is fixed by
        the first step, a later step of another dtype is cast to it), writes them into the cache, closes every chunk its tokens
        complete with ONE close launch (chunk means -> mu networks -> beta, on the module's fp32 mu parameters) and produces
        the outputs of all its tokens with ONE attn launch (each token against its block window [left extension, block] and
        the landmarks of the chunks before its own, masked after itself).  Both kernels compute in fp32 on rows of the
        cache's dtype, so fp32 decoding equals the fp32 full path; on a dynamic state which chunks close is decided on the
        host from the token count, with no read-back.  No limit on the context length or the number of landmarks.
        A state made by `init_static_decoding` / `init_rolling_decoding` (docstrings there) takes the same step with the
        right-hand column of this module's table; on a rolling state the launches address the token rows through the ring, on
        a state with `landmark_splits > 1` a step of at most 8 tokens runs attn as attn_split + merge, and on a state with
        `compact_landmarks` close, attn and attn_split are the `_l16` entry points over 16-bit landmark rows."""
        nv = _ops.nv
        self._refuse_decoding()
        nv.require_cuda(query, "query")                            # (before any state is built: no CPU fallback)
        T_new, B, C = query.shape
        if key_padding_mask is not None:
            # fairseq hands the decoder either the flags of the new positions [B, T_new] or of every position so far
            # [B, t0 + T_new] (`self_attn_padding_mask`): the last T_new columns are this step's in both cases
            if key_padding_mask.dim() != 2 or key_padding_mask.shape[0] != B or key_padding_mask.shape[1] < T_new:
                raise ValueError("key_padding_mask %s does not cover the %d new positions of a batch of %d"
                                 % (tuple(key_padding_mask.shape), T_new, B))
        w, e, h, d, r = self.window_size, self.ext_size, self.num_heads, self.head_dim, self.chunk_size
        if r is None:
            raise NotImplementedError(_NEEDS_CHUNK_SIZE)
        static = self.get_incremental_state(incremental_state, "attn_static")
        dev = query.device
        state = self._get_input_buffer(incremental_state)
        if static is not None:
            capturing, pieces = self._static_room(state, static, T_new, B)
            if static.get("per_sequence"):
                key_padding_mask = self._step_flags(key_padding_mask, T_new)
            if pieces:
                # a prompt: consecutive pieces, each an ordinary step; the pad flags of the step are the last T_new columns
                # in both of fairseq's mask shapes, sliced with the pieces
                step_pad = None if key_padding_mask is None else key_padding_mask[:, -T_new:]
                ys = [self._decode(query[a:a + pieces], None if step_pad is None else step_pad[:, a:a + pieces],
                                   incremental_state, piece=True)[0] for a in range(0, T_new, pieces)]
                return torch.cat(ys, 0), None
        held = static is not None and "w_qkv" in state
        # (like the split: the rows of the step the caller handed over decide, and a capture fixes them)
        held_rows = held and T_new * B <= _LINEAR_MAX_ROWS and not piece
        if held_rows:
            qkv_new = self._held_linear(query.reshape(T_new * B, C), state["w_qkv"], state["b_qkv"], state["proj_rows"])
        elif held:
            qkv_new = self._held_gemm(query, state["w_qkv"], state["b_qkv"]).reshape(T_new, B, 3, h, d)
        else:
            qkv_new = self._project(query, None, None, keep_f32=True)  # [T_new, B, 3, h, d]
        if static is None:
            t0 = self._dynamic_room(incremental_state, state, qkv_new.dtype, B, T_new, dev)
        cache = state["qkv"]
        if not held and qkv_new.dtype != cache.dtype:
            # the cache's dtype is fixed: an fp32 step on a 16-bit cache rounds (with the one-time warning of
            # _ops.to_io_dtype), a 16-bit step on an fp32 cache widens exactly
            qkv_new = _ops.to_io_dtype(qkv_new) if cache.dtype != torch.float32 else qkv_new.float()
            if static is not None:                                 # (append copies the rows as they are; the slice
                qkv_new = qkv_new.to(cache.dtype)                  #  assignment of the dynamic state converts)
        step_pad = None
        if static is not None:
            qkv_new = qkv_new if held_rows else qkv_new.contiguous()     # (proj_rows: the step's rows lead the buffer)
            if key_padding_mask is not None:
                step_pad = key_padding_mask[:, -T_new:].to(device=dev, dtype=torch.uint8).contiguous()
            has_pad, bias = True, state["bias"]
        else:
            cache[:, t0:t0 + T_new] = qkv_new.transpose(0, 1)
            # (whether a mask was ever given lives on the host: the unpadded case passes no mask without reading a flag back
            #  from the device)
            has_pad = bool(self.get_incremental_state(incremental_state, "attn_has_pad"))
            if key_padding_mask is not None:
                state["pad"][:, t0:t0 + T_new] = key_padding_mask[:, -T_new:].to(device=dev, dtype=torch.uint8)
                if not has_pad:
                    has_pad = True
                    self.set_incremental_state(incremental_state, "attn_has_pad", True)
            bias = None
            if self.use_t5_rpe:
                # the module is in eval mode, so the table is built once per weight and reused by every step
                if not hasattr(self, "_decode_bias_cache"):
                    self._decode_bias_cache = _ops.DerivedCache()
                bias = self._decode_bias_cache.get(self, [self.rel_pos_bias.relative_attention_bias.weight],
                                                   lambda: self._decode_bias_table(dev))
        pad = state["pad"]
        io = nv.EA_F32 if cache.dtype == torch.float32 else nv.io_dtype(cache)
        adaptive, has_bias = 1 if self.adaptive_proj == "qk" else 0, 0 if bias is None else 1
        if static is not None:
            family, closes = "ea_ceva_sdecode_", True
            l16 = "_l16" if static.get("compact_landmarks") else ""     # (16-bit landmark rows: close, attn, attn_split)
            geom = nv.ea_ceva_sdec_geom(B, h, d, io, w, e, r, T_new, static.get("cap", cache.shape[1]), adaptive, has_bias,
                                        static.get("ring", 0), state["pos"].data_ptr(), state["status"].data_ptr(),
                                        state["ntok"].data_ptr() if "ntok" in state else None)
        else:
            family, l16 = "ea_ceva_decode_", ""
            c_first, c_last = t0 // r, (t0 + T_new) // r - 1        # the chunks this step's tokens complete
            closes = c_last >= c_first
            geom = nv.ea_ceva_dec_geom(B, h, d, io, w, e, r, t0, T_new, c_first, c_last, cache.shape[1], adaptive, has_bias,
                                       1 if has_pad else 0)
        g = ctypes.byref(geom)
        tq, tk, tv = [nv.t4(cache[:, :, i].transpose(1, 2)) for i in range(3)]      # [B, h, cap (or ring), d] views
        tl, tb = nv.t4(state["rf_k_bar"]), nv.t4(state["beta"])
        mask_p = nv.ptr(pad) if has_pad else None
        rows = (ctypes.byref(tq), ctypes.byref(tk), ctypes.byref(tv), mask_p)      # the token rows and their pad flags
        lmk = (ctypes.byref(tl), ctypes.byref(tb))                                 # the landmark rows
        st = nv.stream()
        if static is not None:
            nv.call("ea_ceva_sdecode_append", g, nv.ptr(qkv_new), nv.ptr(step_pad), nv.ptr(cache), nv.ptr(pad), st)
        if closes:
            if static is not None:
                mlp = state["mu"]
            else:                                                  # (built once per weight)
                if not hasattr(self, "_decode_mu_cache"):
                    self._decode_mu_cache = _ops.DerivedCache()
                mlp = self._decode_mu_cache.get(self, self._mu_params(), self._decode_mu_f32)
            mp = (ctypes.c_void_p * len(mlp))(*[p.data_ptr() for p in mlp])
            nv.call(family + "close" + l16, g, *rows, mp, *lmk, st)
        out = torch.empty((T_new, B, h, d), dtype=cache.dtype, device=dev)
        to = nv.t4(out.permute(1, 2, 0, 3))                        # [B, h, T_new, d] view of the time-first rows
        if static is not None and "split_ws" in state and T_new <= _SPLIT_MAX_STEP and not piece:
            # (the token count of the step the caller handed over decides, and a capture fixes it; the pieces of a prompt,
            #  its short tail included, are the prompt's)
            ws, parts = state["split_ws"], state["split_ws"].shape[3]
            nv.call("ea_ceva_sdecode_attn_split" + l16, g, *rows, nv.ptr(bias), *lmk, ctypes.byref(to), parts, nv.ptr(ws), st)
            nv.call("ea_ceva_sdecode_merge", g, ctypes.byref(to), parts, nv.ptr(ws), st)
        else:
            nv.call(family + "attn" + l16, g, *rows, nv.ptr(bias), *lmk, ctypes.byref(to), st)
        if static is not None:
            nv.call("ea_ceva_sdecode_advance", g, st)
            if not capturing and "ntok" not in state:              # (a replay advances only the device count; per-sequence
                static["count"] += T_new                           #  counts live on the device alone)
        else:
            self.set_incremental_state(incremental_state, "attn_pos", t0 + T_new)
            state["pos"] = state["pos"] + T_new
            self._set_input_buffer(incremental_state, state)
        if held:
            ydtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else query.dtype
            if held_rows:
                ytype = ydtype if ydtype in (cache.dtype, torch.float32) else torch.float32
                y = torch.empty((T_new, B, C), dtype=ytype, device=dev)
                self._held_linear(out.view(T_new * B, C), state["w_out"], state["b_out"], y.view(T_new * B, C))
            else:
                y = self._held_gemm(out.view(T_new, B, C), state["w_out"], state["b_out"])
            return (y if y.dtype == ydtype else y.to(ydtype)), None
        return self._project_out(out.reshape(T_new, B, C), query.dtype).contiguous(), None

    # ---- the projections of a state that holds them ---------------------------------------------------------------------------
    @staticmethod
    def _held_x(x, wdtype):
        """Rows as the held projections take them: fp32 or the weights' type (an fp32 row is rounded as it is loaded;
        outside autocast that departs from the reference's fp32 arithmetic, and the caller is told once, as everywhere)."""
        if x.dtype == torch.float32:
            if not torch.is_autocast_enabled():
                _ops.warn_fp32_rounded(x.dtype)
        elif x.dtype != wdtype:
            x = x.to(wdtype)
        return x if x.is_contiguous() else x.contiguous()

    def _held_linear(self, x2, weight, bias, y2):
        """y2[:M] = x2 weight^T + bias on ea_ceva_sdecode_linear: x2 [M <= 64, K] (fp32 or the weight's type), y2 [>= M, N] rows
        of the weight's type or fp32 -> y2."""
        nv = _ops.nv
        x2 = self._held_x(x2, weight.dtype)
        code = lambda t: nv.EA_F32 if t.dtype == torch.float32 else nv.io_dtype(t)      # noqa: E731
        nv.call("ea_ceva_sdecode_linear", x2.shape[0], weight.shape[1], weight.shape[0], nv.ptr(x2), code(x2), x2.stride(0),
                nv.ptr(weight), nv.io_dtype(weight), nv.ptr(bias), nv.ptr(y2), code(y2), y2.stride(0), nv.stream())
        return y2

    def _held_gemm(self, x, weight, bias):
        """A step above 64 rows: the library GEMM the plain step ends in, on the held 16-bit operands (no concatenation and
        no cast of a weight) -> [..., N] in the weights' type."""
        x = self._held_x(x, weight.dtype)
        with torch.autocast(device_type="cuda", enabled=False):
            return torch.nn.functional.linear(x if x.dtype == weight.dtype else x.to(weight.dtype), weight, bias)
