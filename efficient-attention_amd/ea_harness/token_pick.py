"""How `sequence.DecoderStack` turns final-layer rows into tokens: the pieces every decoding mode is made of.

  operand helpers  -- what each vocabulary entry of the C ABI is handed, written once: `rows_operand` (rows [T, B, C] -> the
                      [T B, C] kernel operand), `checked_out`, `checked_targets`, `type_code`, `pieces` (at most 64 rows per
                      launch) and `AdaptiveTables.host_arrays`.
  attachments      -- what a DecodingState carries beside the attention's state: the held vocabulary pair (`HeldVocab`), `Sampler`,
                      `Scorer`, `Beam`, `AdaptivePick`.  Each is an `Attachment`: it names its `tensors()` (the byte count) and
                      follows a `reorder`, a `reset_rows` and a `refresh` of the state; `DecodingState.attachments()` lists those a
                      state has, so that the stack's four lifecycle methods name none of them.
  picks            -- one class per launch: `HeldGreedy` (ea_ceva_sdecode_vocab_argmax), `HeldSampled` (.._sample),
                      `HeldGreedyLogprob` (.._logprob), `HeldSampledLogprob` (.._sample_logprob), `AdaptiveGreedy`
                      (ea_adaptive_pick), `AdaptiveSampled` (ea_adaptive_sample), `BeamStep` (.._beam; .._beam_c on a Beam with a constraint),
                      `AdaptiveBeamStep` (ea_adaptive_beam, ea_adaptive_beam_c), and `FrameworkGreedy`, `logits(rows).argmax(-1)`.  `run` is the
                      launch behind the stack's public method of that mode; calling the pick, `pick(rows, out=None) -> tokens`,
                      is what a decoding loop does with it: `logp` is the [1, B] view of the static log-probability buffer the
                      call writes (None: the mode has none), `save()` / `restore(saved)` bracket a warm-up call (the sampler's
                      draw counters).  `select_pick` (`DecodingState.pick`) selects the pick of a state."""
import ctypes

import torch

MAX_ROWS = 64                # EA_CEVA_LINEAR_MAX_ROWS of include/ea_hip.h: the rows of one launch of the few-row entries
SAMPLE_MAX_K = 64
BEAM_MAX_W = 32
VOCAB = "ea_ceva_sdecode_vocab_argmax"
SAMPLE = "ea_ceva_sdecode_vocab_sample"
LOGPROB = "ea_ceva_sdecode_vocab_logprob"
SAMPLE_LOGPROB = "ea_ceva_sdecode_vocab_sample_logprob"
ADAPTIVE_PICK = "ea_adaptive_pick"
BEAM = "ea_ceva_sdecode_vocab_beam"
ADAPTIVE_SAMPLE = "ea_adaptive_sample"
ADAPTIVE_BEAM = "ea_adaptive_beam"
BEAM_C = "ea_ceva_sdecode_vocab_beam_c"
ADAPTIVE_BEAM_C = "ea_adaptive_beam_c"
BAN_MAX_STATIC = 16          # static bans and the largest no_repeat_ngram_size of the constrained beam step (ABI 36)
BAN_MAX_NGRAM = 16


def _native():
    from efficient_attention import _native as nv
    return nv


# ---- operand helpers --------------------------------------------------------------------------------------------------------------
def type_code(t):
    """The C ABI's code of an operand that is fp32 or 16-bit."""
    nv = _native()
    return nv.EA_F32 if t.dtype == torch.float32 else nv.io_dtype(t)


def rows_operand(table, rows):
    """rows [T, B, C] against table [V, C] -> the [T B, C] operand of the vocabulary kernels: fp32 or the table's type (other
    rows are widened to fp32), contiguous, 16-byte aligned."""
    T, B, C = rows.shape
    if C != table.shape[1]:
        raise ValueError("rows of %d channels against a table of %d" % (C, table.shape[1]))
    if rows.device != table.device:
        raise ValueError("table must be on the rows' device (%s); it is on %s" % (rows.device, table.device))
    x2 = rows.detach()
    if x2.dtype not in (torch.float32, table.dtype):
        x2 = x2.float()
    x2 = x2.contiguous().view(T * B, C)
    if x2.data_ptr() % 16:
        x2 = x2.clone()
    return x2


def score_operand(table, rows):
    """`rows_operand` against a table the caller holds: the argument errors of `rows_logprobs` first."""
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype not in (torch.bfloat16, torch.float16) \
            or not table.is_contiguous() or table.data_ptr() % 16:
        raise ValueError("table must be a contiguous, 16-byte aligned 16-bit [V, C] tensor (bfloat16 or float16); got %s"
                         % (("%s %s" % (str(table.dtype).replace("torch.", ""), list(table.shape)))
                            if isinstance(table, torch.Tensor) else type(table).__name__))
    if rows.dim() != 3 or rows.shape[0] * rows.shape[1] < 1:
        raise ValueError("rows must be a [T, B, C] tensor of at least one row; got %s" % (tuple(rows.shape),))
    return rows_operand(table, rows)


def single_step(rows, limit, who):
    """The shape check of a sampled pick: one single-token step of at most `limit` rows."""
    if rows.shape[0] != 1 or rows.shape[1] > limit:
        raise ValueError("%s takes the rows of one single-token step, [1, B <= %d, C]; got %s" % (who, limit, tuple(rows.shape)))


def checked_out(out, shape, dtype, device, what="out"):
    """`out` where the caller gave one (checked), else a new tensor."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError("%s must be a contiguous %s %s tensor on the rows' device"
                         % (what, str(dtype).replace("torch.", ""), list(shape)))
    return out


def checked_targets(targets, T, B, device):
    """targets int64 [T, B] on the rows' device -> [T B], contiguous; None stays None."""
    if targets is None:
        return None
    if targets.dtype != torch.long or tuple(targets.shape) != (T, B) or targets.device != device:
        raise ValueError("targets must be an int64 [%d, %d] tensor on the rows' device" % (T, B))
    return targets.contiguous().view(T * B)


def pieces(n):
    """(M, slice) of the launches n rows run in: at most 64 rows each."""
    for a in range(0, n, MAX_ROWS):
        yield min(MAX_ROWS, n - a), slice(a, a + MAX_ROWS)


def _ptr_or_none(nv, tensors):
    return (None, None, None) if tensors is None else [nv.ptr(t) for t in tensors]


# ---- what a decoding state carries --------------------------------------------------------------------------------------------------
class Attachment:
    """What the lifecycle of a DecodingState asks of everything attached to it.  The defaults: nothing to count, nothing to
    move with a reorder, nothing to reset with a row, nothing to re-read with the weights."""

    def tensors(self):
        return ()

    def reorder(self, new_order):
        pass

    def reset_rows(self, rows):
        pass

    def refresh(self, stack):
        pass


class HeldVocab(Attachment):
    """The pair `vocab` (the 16-bit [V, C] copy of embed_tokens.weight) and `vocab_ws` (the pick's workspace) of a state made
    with hold_vocab, as they stand on the state."""

    def __init__(self, state):
        self.state = state

    def tensors(self):
        return tuple(t for t in (self.state.vocab, self.state.vocab_ws) if t is not None)

    def refresh(self, stack):
        with torch.no_grad():
            self.state.vocab.copy_(stack.embed_tokens.weight)       # (rounded to nearest even, in place: data_ptr() stays)


class Sampler(Attachment):
    """What `DecoderStack.init_sampling` attaches to a DecodingState: the fp32 `logits` buffer [batch_size, V] of the sampled
    pick, the draw counters `ctr` (int64 [B]: draw n of a row is made at ctr = n) and the stream ids `sid` (int32 [B]), both
    on the device, the host scalars `seed`, `top_k`, `top_p`, `temperature`, and `next_sid`, the first stream id no row of
    this state has had.  On a state with an adaptive pick there is no [batch_size, V] row: `logits` is None and `ws` is the
    workspace of ea_adaptive_sample for batch_size rows (bytes; it holds every band's fp32 logits, about 4 B V)."""

    def __init__(self, logits, ctr, sid, seed, top_k, top_p, temperature, ws=None):
        self.logits, self.ctr, self.sid, self.ws = logits, ctr, sid, ws
        self.seed, self.top_k, self.top_p, self.temperature = seed, top_k, top_p, temperature
        self.next_sid = sid.numel()

    def tensors(self):
        return tuple(t for t in (self.logits, self.ws, self.ctr, self.sid) if t is not None)

    def reorder(self, new_order):                       # a row takes its stream along: counters and ids, in place
        order = new_order.to(device=self.ctr.device, dtype=torch.long)
        self.ctr.copy_(self.ctr.index_select(0, order))
        self.sid.copy_(self.sid.index_select(0, order))

    def reset_rows(self, rows):                         # a new sequence: draw 0 of a stream no row has had
        at = torch.as_tensor(rows, device=self.ctr.device).reshape(-1).long()
        if at.numel():                                  # (how many is known on the host: no read-back)
            fresh = torch.arange(self.next_sid, self.next_sid + at.numel(), dtype=torch.int32, device=self.sid.device)
            self.next_sid += at.numel()
            self.ctr.index_fill_(0, at, 0)
            self.sid.index_copy_(0, at, fresh)


class Scorer(Attachment):
    """What `DecoderStack.init_logprobs` attaches to a DecodingState: `ws`, the tile sums and target logits of
    ea_ceva_sdecode_vocab_logprob for 64 rows (bytes), and the static fp32 buffers `lse` and `logp` [batch_size] a captured
    step writes its log-sum-exp and its token's log-probability into."""

    def __init__(self, ws, lse, logp):
        self.ws, self.lse, self.logp = ws, lse, logp

    def tensors(self):
        return (self.ws, self.lse, self.logp)


class AdaptiveTables:
    """What `DecoderStack.adaptive_tables(dtype)` returns, the held 16-bit operands of ea_adaptive_score (include/ea_hip.h, ABI
    33): `cutoff` (the list, ending with V), `dims` (d_i per tail), `head` [c0 + n, C] (band 0's table with the class rows
    behind it), `proj[i]` [d_i, C] (K-contiguous: a tied [C, d_i] projection is transposed as the copy is taken) and
    `tables[i]` [V_i, d_i].  The projections are the row blocks of ONE [sum d_i, C] buffer (`proj_all`), so that
    ea_adaptive_pick forms every h_i in one launch.  `refresh()` re-reads the parameters in place (rounded to nearest even;
    every data_ptr() stays)."""

    def __init__(self, softmax, dtype, device):
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("adaptive_tables holds 16-bit operands (bfloat16 or float16), got %s" % dtype)
        self.softmax, self.cutoff, self.dims = softmax, list(softmax.cutoff), softmax.band_dims()
        n, C = len(self.dims), softmax.input_dim

        def buf(*shape):
            return torch.empty(shape, dtype=dtype, device=device)
        self.head = buf(self.cutoff[0] + n, C)
        self.proj_all = buf(sum(self.dims), C)
        self.proj = list(self.proj_all.split(self.dims, 0))
        self.tables = [buf(self.cutoff[i + 1] - self.cutoff[i], d) for i, d in enumerate(self.dims)]
        self.refresh()

    @property
    def dtype(self):
        return self.head.dtype

    @property
    def device(self):
        return self.head.device

    def refresh(self):
        sm, c0 = self.softmax, self.cutoff[0]
        with torch.no_grad():
            full = sm.head_table()
            self.head[:c0].copy_(full[:c0])
            self.head[c0:].copy_(full[c0:])
            for i in range(len(self.dims)):
                self.proj[i].copy_(sm.tail_projection(i))
                self.tables[i].copy_(sm.tail_table(i))
        return self

    def tensors(self):
        return [self.head] + self.proj + self.tables

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.tensors())

    def host_arrays(self):
        """-> (cut, dims, proj, tabs), the host array arguments of the adaptive entries: the cutoffs (int64), the tails' widths
        (int32) and the pointers of their projections and tables."""
        nv = _native()
        return (nv.host_array(ctypes.c_int64, self.cutoff), nv.host_array(ctypes.c_int32, self.dims),
                nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in self.proj]),
                nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in self.tables]))


class AdaptivePick(Attachment):
    """What `DecoderStack.init_adaptive_decoding` attaches to a DecodingState: `tables` (an AdaptiveTables in the state's
    dtype), `ws` (the workspace of ea_adaptive_pick for 64 rows, bytes) and the static fp32 buffer `logp` [batch_size] a
    captured step writes its token's log-probability into."""

    def __init__(self, tables, ws, logp):
        self.tables, self.ws, self.logp = tables, ws, logp

    def tensors(self):
        return tuple(self.tables.tensors()) + (self.ws, self.logp)

    def refresh(self, stack):
        self.tables.refresh()


class BeamConstraint:
    """What `DecoderStack.init_beam_constraints` hangs on a Beam when it is given min_len, no_repeat_ngram_size, ban_tokens or
    prompt_cap (include/ea_hip.h, ABI 36): those host scalars and the static buffers of the constrained entries --
    `prompt_tok` int32 [S, prompt_cap] and `prompt_len` int32 [S] (`set_beam_prompt`; both None at prompt_cap = 0) and `gen`
    int32 [2, M, max_new], the beams' generated tokens, row-major, a ping-pong pair the ban-list launch keeps.  The ban list
    itself lies behind the step's workspace in the Beam's `ws`."""

    def __init__(self, min_len, ngram, ban_tokens, prompt_cap, prompt_tok, prompt_len, gen):
        self.min_len, self.ngram, self.ban_tokens, self.prompt_cap = min_len, ngram, ban_tokens, prompt_cap
        self.prompt_tok, self.prompt_len, self.gen = prompt_tok, prompt_len, gen

    def tensors(self):
        return tuple(t for t in (self.prompt_tok, self.prompt_len, self.gen) if t is not None)

    def scalars(self):
        return (self.min_len, self.ngram, self.ban_tokens)

    def arguments(self, nv):
        """The constrained entries' arguments behind the unconstrained ones'."""
        bans = nv.host_array(ctypes.c_int32, list(self.ban_tokens)) if self.ban_tokens else None
        return [self.min_len, self.ngram, bans, len(self.ban_tokens), nv.ptr(self.prompt_tok), self.prompt_cap,
                nv.ptr(self.prompt_len), nv.ptr(self.gen)]


class Beam(Attachment):
    """What `DecoderStack.init_beam_search` attaches to a DecodingState: the host scalars `beam_size` (W), `eos_idx`,
    `max_new`, `len_penalty` and the static buffers of ea_ceva_sdecode_vocab_beam (include/ea_hip.h, ABI 32) for M = the
    state's batch size = S W rows: `logits` fp32 [M, V], `ws` (the entry's workspace, bytes), `score` fp32 [M], `t`, `nfin`,
    `done` int32 [S], `parent` int64 [M], `hist_tok`, `hist_par` int32 [max_new, M], `fin_score` fp32 [S, W], `fin_len`,
    `fin_beam` int32 [S, W].  `replays`: how many steps behind the first pick the last `beam_search` on it ran.
    On a state with an adaptive pick `logits` is None and `ws` is ea_adaptive_beam's workspace (it holds the bands' logits).
    `constraint`: None, or the BeamConstraint of a search with min_len, n-gram blocking or static bans (ABI 36); `ws` is then
    the constrained entry's workspace."""

    def __init__(self, beam_size, eos_idx, max_new, len_penalty, logits, ws, score, t, nfin, done, parent, hist_tok, hist_par,
                 fin_score, fin_len, fin_beam, constraint=None):
        self.constraint = constraint
        self.beam_size, self.eos_idx, self.max_new, self.len_penalty = beam_size, eos_idx, max_new, len_penalty
        self.logits, self.ws, self.score, self.t, self.nfin, self.done, self.parent = logits, ws, score, t, nfin, done, parent
        self.hist_tok, self.hist_par = hist_tok, hist_par
        self.fin_score, self.fin_len, self.fin_beam = fin_score, fin_len, fin_beam
        self.replays = 0

    def buffers(self):
        return tuple(t for t in (self.logits, self.ws, self.score, self.t, self.nfin, self.done, self.parent, self.hist_tok,
                                 self.hist_par, self.fin_score, self.fin_len, self.fin_beam) if t is not None) \
            + (() if self.constraint is None else self.constraint.tensors())

    tensors = buffers


class DecodingState:
    """What `DecoderStack.init_decoding` returns: `incremental` (the incremental state every layer's attention keeps its
    static or rolling state in, under its own key), `ffn` (per layer the held 16-bit (fc1.weight, fc1.bias, fc2.weight,
    fc2.bias), or None without hold_weights), the arguments it was made with (`options`) and, made with hold_vocab, `vocab`
    (the 16-bit [V, C] copy of embed_tokens.weight) and `vocab_ws` (the pick's workspace, bytes); both None otherwise.
    The fourth argument is that pair, (vocab, vocab_ws), or None.
    `sampler` is None until `DecoderStack.init_sampling` attaches a Sampler, `scorer` until `DecoderStack.init_logprobs`
    attaches a Scorer, `beam` until `DecoderStack.init_beam_search` attaches a Beam, `adaptive` until
    `DecoderStack.init_adaptive_decoding` attaches an AdaptivePick.  `attachments()` lists what is there, `pick` selects the pick
    that follows from it."""

    sampler = None
    scorer = None
    beam = None
    adaptive = None

    def __init__(self, incremental, ffn, options, vocab=None):
        self.incremental, self.ffn, self.options = incremental, ffn, options
        self.vocab, self.vocab_ws = (None, None) if vocab is None else vocab

    @property
    def hold_weights(self):
        return self.ffn is not None

    @property
    def hold_vocab(self):
        return self.vocab is not None

    def attachments(self):
        """The Attachments of this state: the held vocabulary pair first, then what the `init_*` methods attached."""
        if self.vocab is not None:
            yield HeldVocab(self)
        for a in (self.sampler, self.scorer, self.beam, self.adaptive):
            if a is not None:
                yield a

    def pick(self, stack, B, return_logprobs=False):
        """`select_pick` for this state."""
        return select_pick(stack, self, B, return_logprobs)


def select_pick(stack, state, B, return_logprobs=False):
    """The pick `stack.generate` ends its step in, for a prompt of B rows on `state` (None: the state `generate` makes for
    itself, which holds no table): the one selector, keyed on what is attached and on return_logprobs.  What is asked for and
    not attached raises here, before anything has run."""
    if state is not None and state.adaptive is not None:
        if B > state.adaptive.logp.numel():
            raise ValueError("a prompt of %d rows on an adaptive pick made for %d" % (B, state.adaptive.logp.numel()))
        return (AdaptiveGreedy if state.sampler is None else AdaptiveSampled)(stack, state, B)
    if return_logprobs:
        if state is None or state.scorer is None:
            raise RuntimeError("generate(return_logprobs=True) needs a decoding state with a scorer: init_logprobs(state)")
        if B > state.scorer.logp.numel():
            raise ValueError("a prompt of %d rows on a scorer made for %d" % (B, state.scorer.logp.numel()))
        return (HeldGreedyLogprob if state.sampler is None else HeldSampledLogprob)(stack, state, B)
    if state is None or state.vocab is None:
        return FrameworkGreedy(stack)
    return (HeldGreedy if state.sampler is None else HeldSampled)(stack, state)


# ---- the picks --------------------------------------------------------------------------------------------------------------------
class Pick:
    """pick(rows [T, B, C], out=None) -> tokens int64 [T, B], written into `out` where one is given: the end of a decoding
    step.  `stack` and `state` are the two it was selected for; the table and the workspaces are that state's, whichever
    state's rows it is handed."""
    logp = None                                         # a [1, B] view of the static log-probability buffer, where one is written

    def __init__(self, stack, state=None, B=None):
        self.stack, self.state = stack, state
        if B is not None:                               # (a pick made for a loop over B rows: its static views)
            self._static(B)

    def _static(self, B):
        pass

    def save(self):
        """What a warm-up call consumes and `restore` puts back."""
        return None

    def restore(self, saved):
        pass


class FrameworkGreedy(Pick):
    """`logits(rows).argmax(-1)`: the framework's pick, on a state that holds no table."""

    def __call__(self, rows, out=None):
        tokens = self.stack.logits(rows).argmax(-1)
        return tokens if out is None else out.copy_(tokens)


class HeldGreedy(Pick):
    """ea_ceva_sdecode_vocab_argmax on the held table: `next_tokens`."""

    def __call__(self, rows, out=None):
        return self.stack.next_tokens(rows, self.state, out=out)

    def run(self, rows, out, return_logits):
        nv = _native()
        table, ws = self.state.vocab, self.state.vocab_ws
        T, B, C = rows.shape
        V = table.shape[0]
        x2 = rows_operand(table, rows)
        out = checked_out(out, (T, B), torch.long, x2.device)
        tok = out.view(T * B)
        logits = torch.empty((T * B, V), dtype=torch.float32, device=x2.device) if return_logits else None
        code = type_code(x2)
        for M, s in pieces(T * B):
            nv.call(VOCAB, M, C, V, nv.ptr(x2[s]), code, C, nv.ptr(table), nv.io_dtype(table),
                    None if logits is None else nv.ptr(logits[s]), nv.EA_F32, V, nv.ptr(ws), ws.numel(), nv.ptr(tok[s]), None,
                    nv.stream())
        return (out, logits.view(T, B, V)) if return_logits else out


class HeldGreedyLogprob(Pick):
    """ea_ceva_sdecode_vocab_logprob on the held table and the scorer's workspace: `token_logprobs`; called as a pick it
    writes into the first B entries of the scorer's static `logp` and `lse`."""

    def _static(self, B):
        sc = self.state.scorer
        self.logp, self.lse = sc.logp[:B].view(1, B), sc.lse[:B].view(1, B)

    def __call__(self, rows, out=None):
        return self.run(rows, None, out, self.logp, self.lse)[0]

    def run(self, rows, targets, out, logp, lse):
        """-> (tokens, logp, lse), each [T, B]; out, logp, lse: their places (None: allocated)."""
        nv = _native()
        table, ws, lws = self.state.vocab, self.state.vocab_ws, self.state.scorer.ws
        T, B, C = rows.shape
        V = table.shape[0]
        x2 = rows_operand(table, rows)
        dev = x2.device
        out = checked_out(out, (T, B), torch.long, dev)
        logp = checked_out(logp, (T, B), torch.float32, dev, "logp")
        lse = checked_out(lse, (T, B), torch.float32, dev, "lse")
        targets = checked_targets(targets, T, B, dev)
        tok, lp, ls = out.view(T * B), logp.view(T * B), lse.view(T * B)
        code = type_code(x2)
        for M, s in pieces(T * B):
            nv.call(LOGPROB, M, C, V, nv.ptr(x2[s]), code, C, nv.ptr(table), nv.io_dtype(table), None, nv.EA_F32, V,
                    nv.ptr(ws), ws.numel(), nv.ptr(tok[s]), None, nv.ptr(lws), lws.numel(),
                    None if targets is None else nv.ptr(targets[s]), nv.ptr(ls[s]), nv.ptr(lp[s]), nv.stream())
        return out, logp, lse


class HeldSampled(Pick):
    """ea_ceva_sdecode_vocab_sample on the held table: `sample_tokens`.  A warm-up draws once: `save` / `restore` keep the
    counters."""
    who = "sample_tokens"

    def __call__(self, rows, out=None):
        return self.stack.sample_tokens(rows, self.state, out=out)

    def save(self):
        return self.state.sampler.ctr.clone()

    def restore(self, saved):
        self.state.sampler.ctr.copy_(saved)

    def _operands(self, rows):
        """-> (x2, the entry's arguments up to the logits buffer): the checks of a sampled pick, in their order."""
        nv, sm, table = _native(), self.state.sampler, self.state.vocab
        single_step(rows, min(MAX_ROWS, sm.ctr.numel()), self.who)
        x2 = rows_operand(table, rows)
        B, C, V = x2.shape[0], x2.shape[1], table.shape[0]
        return x2, [B, C, V, nv.ptr(x2), type_code(x2), C, nv.ptr(table), nv.io_dtype(table), nv.ptr(sm.logits), V]

    def _draw(self, out):
        nv, sm, ws = _native(), self.state.sampler, self.state.vocab_ws
        return [nv.ptr(ws), ws.numel(), sm.top_k, sm.top_p, sm.temperature, sm.seed, nv.ptr(sm.ctr), nv.ptr(sm.sid), nv.ptr(out)]

    def run(self, rows, out, return_details):
        nv, sm = _native(), self.state.sampler
        x2, args = self._operands(rows)
        B, dev = x2.shape[0], x2.device
        out = checked_out(out, (1, B), torch.long, dev)
        details = None
        if return_details:
            details = (torch.empty((B, sm.top_k), dtype=torch.int32, device=dev),
                       torch.empty((B, sm.top_k), dtype=torch.float32, device=dev),
                       torch.empty((B,), dtype=torch.int32, device=dev))
        nv.call(SAMPLE, *args, *self._draw(out), *_ptr_or_none(nv, details), nv.stream())
        return (out,) + details if return_details else out


class HeldSampledLogprob(HeldSampled):
    """ea_ceva_sdecode_vocab_sample_logprob on the held table, the sampler and the scorer: `sample_tokens_logprobs`; called
    as a pick it writes into the first B entries of the scorer's static `logp` and `lse`."""
    who = "a sampled pick"
    _static = HeldGreedyLogprob._static

    def __call__(self, rows, out=None):
        return self.run(rows, out, self.logp, self.lse)[0]

    def run(self, rows, out, logp, lse):
        """-> (tokens, logp, lse), each [1, B]; out, logp, lse: their places (None: allocated)."""
        nv, lws = _native(), self.state.scorer.ws
        x2, args = self._operands(rows)
        B, dev = x2.shape[0], x2.device
        out = checked_out(out, (1, B), torch.long, dev)
        logp = checked_out(logp, (1, B), torch.float32, dev, "logp")
        lse = checked_out(lse, (1, B), torch.float32, dev, "lse")
        nv.call(SAMPLE_LOGPROB, *args, *self._draw(out), None, None, None, nv.ptr(lws), lws.numel(), nv.ptr(lse), nv.ptr(logp),
                nv.stream())
        return out, logp, lse


class AdaptiveGreedy(Pick):
    """ea_adaptive_pick on the held adaptive tables: `next_tokens` and `token_logprobs` of a state with an adaptive pick;
    called as a pick it writes into the first B entries of the static `state.adaptive.logp`."""

    def _static(self, B):
        self.logp = self.state.adaptive.logp[:B].view(1, B)

    def __call__(self, rows, out=None):
        return self.run(rows, None, out, self.logp)[0]

    def run(self, rows, targets, out, logp):
        """-> (tokens int64 [T, B], logp fp32 [T, B]), in pieces of 64 rows; out, logp: their places (None: allocated)."""
        nv, ad = _native(), self.state.adaptive
        tb = ad.tables
        x2 = score_operand(tb.head, rows)
        T, B, C = rows.shape
        dev, n = x2.device, len(tb.dims)
        out = checked_out(out, (T, B), torch.long, dev)
        logp = checked_out(logp, (T, B), torch.float32, dev, "logp")
        targets = checked_targets(targets, T, B, dev)
        nv.require_cuda(x2, "rows")
        cut, dims, proj, tabs = tb.host_arrays()
        tok, lp = out.view(T * B), logp.view(T * B)
        code = type_code(x2)
        for M, s in pieces(T * B):
            nv.call(ADAPTIVE_PICK, M, C, n, cut, dims, nv.ptr(x2[s]), code, C, None if targets is None else nv.ptr(targets[s]),
                    nv.ptr(tb.head), nv.io_dtype(tb.head), proj, tabs, nv.ptr(ad.ws), ad.ws.numel(), nv.ptr(tok[s]),
                    nv.ptr(lp[s]), nv.stream())
        return out, logp


class AdaptiveSampled(Pick):
    """ea_adaptive_sample on the held adaptive tables and the sampler's workspace: `sample_tokens` and
    `sample_tokens_logprobs` of a state with an adaptive pick and a sampler; called as a pick it writes the drawn tokens'
    joint log-probabilities into the first B entries of the static `state.adaptive.logp`.  A warm-up draws once: `save` /
    `restore` keep the counters."""
    save, restore = HeldSampled.save, HeldSampled.restore

    def _static(self, B):
        self.logp = self.state.adaptive.logp[:B].view(1, B)

    def __call__(self, rows, out=None):
        return self.run(rows, out, self.logp, False)[0]

    def run(self, rows, out, logp, return_details, who="sample_tokens"):
        """-> (tokens int64 [1, B], logp fp32 [1, B]), with return_details and (sel_idx, sel_val, kept); out, logp: their
        places (None: allocated)."""
        nv, sm, tb = _native(), self.state.sampler, self.state.adaptive.tables
        single_step(rows, min(MAX_ROWS, sm.ctr.numel()), who)
        x2 = score_operand(tb.head, rows)
        B, C = x2.shape
        dev, n = x2.device, len(tb.dims)
        out = checked_out(out, (1, B), torch.long, dev)
        logp = checked_out(logp, (1, B), torch.float32, dev, "logp")
        nv.require_cuda(x2, "rows")
        details = None
        if return_details:
            details = (torch.empty((B, sm.top_k), dtype=torch.int32, device=dev),
                       torch.empty((B, sm.top_k), dtype=torch.float32, device=dev),
                       torch.empty((B,), dtype=torch.int32, device=dev))
        cut, dims, proj, tabs = tb.host_arrays()
        nv.call(ADAPTIVE_SAMPLE, B, C, n, cut, dims, nv.ptr(x2), type_code(x2), C, nv.ptr(tb.head), nv.io_dtype(tb.head), proj,
                tabs, nv.ptr(sm.ws), sm.ws.numel(), sm.top_k, sm.top_p, sm.temperature, sm.seed, nv.ptr(sm.ctr), nv.ptr(sm.sid),
                nv.ptr(out), nv.ptr(logp), *_ptr_or_none(nv, details), nv.stream())
        return (out, logp) + details if return_details else (out, logp)


class BeamStep(Pick):
    """ea_ceva_sdecode_vocab_beam on the held table and the state's Beam: `beam_step`.  The tokens it picks are the beams' next
    inputs; the parents they continue are written into `state.beam.parent`.  (No pick of `generate`: a search's step also
    reorders the state, `DecoderStack.beam_search`.)"""

    def run(self, rows, out, return_details):
        nv, bm, table = _native(), self.state.beam, self.state.vocab
        x2 = rows_operand(table, rows)
        M, C, V, W, dev = x2.shape[0], x2.shape[1], table.shape[0], bm.beam_size, x2.device
        out = checked_out(out, (1, M), torch.long, dev)
        details = None
        if return_details:
            details = (torch.empty((M, 2 * W), dtype=torch.int32, device=dev),
                       torch.empty((M, 2 * W), dtype=torch.float32, device=dev),
                       torch.empty((M,), dtype=torch.float32, device=dev))
        c = bm.constraint
        nv.call(BEAM if c is None else BEAM_C, M, C, V, nv.ptr(x2), type_code(x2), C, nv.ptr(table), nv.io_dtype(table),
                nv.ptr(bm.logits), V,
                nv.ptr(bm.ws), bm.ws.numel(), W, bm.eos_idx, bm.max_new, nv.ptr(bm.score), nv.ptr(bm.t), nv.ptr(bm.nfin),
                nv.ptr(bm.done), nv.ptr(out), nv.ptr(bm.parent), nv.ptr(bm.hist_tok), nv.ptr(bm.hist_par), nv.ptr(bm.fin_score),
                nv.ptr(bm.fin_len), nv.ptr(bm.fin_beam), *_ptr_or_none(nv, details), None,
                *(() if c is None else c.arguments(nv)), nv.stream())
        return (out, bm.parent) + details if return_details else (out, bm.parent)


class AdaptiveBeamStep(Pick):
    """ea_adaptive_beam on the held adaptive tables and the state's Beam: `beam_step` of a state with an adaptive pick.  What
    `BeamStep` says of tokens and parents holds; the details have no single log-sum-exp."""

    def run(self, rows, out, return_details):
        nv, bm, tb = _native(), self.state.beam, self.state.adaptive.tables
        x2 = score_operand(tb.head, rows)
        M, C = x2.shape
        W, dev, n = bm.beam_size, x2.device, len(tb.dims)
        out = checked_out(out, (1, M), torch.long, dev)
        nv.require_cuda(x2, "rows")
        details = None
        if return_details:
            details = (torch.empty((M, 2 * W), dtype=torch.int32, device=dev),
                       torch.empty((M, 2 * W), dtype=torch.float32, device=dev))
        cut, dims, proj, tabs = tb.host_arrays()
        c = bm.constraint
        nv.call(ADAPTIVE_BEAM if c is None else ADAPTIVE_BEAM_C, M, C, n, cut, dims, nv.ptr(x2), type_code(x2), C, nv.ptr(tb.head),
                nv.io_dtype(tb.head), proj, tabs,
                nv.ptr(bm.ws), bm.ws.numel(), W, bm.eos_idx, bm.max_new, nv.ptr(bm.score), nv.ptr(bm.t), nv.ptr(bm.nfin),
                nv.ptr(bm.done), nv.ptr(out), nv.ptr(bm.parent), nv.ptr(bm.hist_tok), nv.ptr(bm.hist_par), nv.ptr(bm.fin_score),
                nv.ptr(bm.fin_len), nv.ptr(bm.fin_beam), *(_ptr_or_none(nv, details)[:2]),
                *(() if c is None else c.arguments(nv)), nv.stream())
        return (out, bm.parent) + details if return_details else (out, bm.parent)
