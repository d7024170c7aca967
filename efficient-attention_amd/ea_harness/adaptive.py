"""fairseq's adaptive input and adaptive softmax (the embedding and the output layer of the wikitext-103 recipe,
transformer_lm_wiki103 with --criterion adaptive_loss), restated from their mathematics.

With cutoffs c0 < c1 < .. < c_n = V the vocabulary falls into band 0 = [0, c0) and the n tail bands [c_i, c_{i+1}); band i has
width d_i = initial_dim // factor ** i (d_0 = initial_dim).

  AdaptiveInput     token t of band i embeds as E_i[t - c_{i-1}] P_i^T, E_i [V_i, d_i], P_i [C, d_i] (every band has a
                    projection, band 0 too).
  AdaptiveSoftmax   head logits x [E_0; W_class]^T, c0 + n columns; a head target scores head_logit[t] - lse_head, a target
                    of tail i (head_logit[c0 + i] - lse_head) + (tail_logit_i[t - c_i] - lse_tail_i) with tail_logit_i =
                    (x Q_i) E_{i+1}^T; Q_i is P_{i+1} itself (tie_proj), else a weight [d_i, C] of its own.

The members, and so the state_dict keys, shapes and buffers (the tied duplicates included), are the reference modules': a
reference checkpoint's decoder keys load with strict=True.  Both classes here are plain torch: AdaptiveInput is what the
stack runs (device ops only, no read-back: a captured decoding step may hold it); AdaptiveSoftmax.get_log_prob is the SLOW
route and the CPU yardstick -- the scoring hot path is ea_adaptive_score (DecoderStack.rows_logprobs)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _cutoffs(vocab_size, cutoff):
    cutoff = [int(c) for c in cutoff]
    if vocab_size > cutoff[-1]:
        cutoff = cutoff + [int(vocab_size)]
    elif vocab_size != cutoff[-1]:
        raise ValueError("a cutoff (%d) beyond the vocabulary (%d)" % (cutoff[-1], vocab_size))
    if cutoff[0] < 1 or any(b <= a for a, b in zip(cutoff, cutoff[1:])):
        raise ValueError("cutoffs must be positive and increasing, got %s" % (cutoff,))
    return cutoff


def _no_q_noise(q_noise):
    if q_noise != 0:
        raise NotImplementedError("q_noise > 0 (quantisation noise) on the adaptive layers is out of scope")


class AdaptiveInput(nn.Module):
    """tokens [...] int64 -> [..., output_dim].  embeddings[i] = Sequential(Embedding(V_i, d_i), Linear(d_i, output_dim,
    bias=False)); `cutoff` ends with the vocabulary size."""

    def __init__(self, vocab_size, padding_idx, initial_dim, factor, output_dim, cutoff, q_noise=0, qn_block_size=8):
        super().__init__()
        _no_q_noise(q_noise)
        self.cutoff = _cutoffs(vocab_size, cutoff)
        self.embedding_dim, self.padding_idx = output_dim, padding_idx
        self.embeddings = nn.ModuleList()
        for i, end in enumerate(self.cutoff):
            start = self.cutoff[i - 1] if i else 0
            dim = int(initial_dim // (factor ** i))
            emb = nn.Embedding(end - start, dim, padding_idx if i == 0 else None)
            nn.init.normal_(emb.weight, mean=0, std=dim ** -0.5)
            if i == 0 and padding_idx is not None:
                nn.init.constant_(emb.weight[padding_idx], 0)
            proj = nn.Linear(dim, output_dim, bias=False)
            nn.init.xavier_uniform_(proj.weight)
            self.embeddings.append(nn.Sequential(emb, proj))
        self.register_buffer("_float_tensor", torch.zeros(1))

    def weights_for_band(self, band):
        return self.embeddings[band][0].weight, self.embeddings[band][1].weight

    @property
    def dtype(self):
        return self.embeddings[0][0].weight.dtype

    def forward(self, tokens):
        """Per band: clamp the local index into the band, look it up, project, select by the band's mask.  Every band runs
        on every token -- no mask.any(), no nonzero: nothing here waits for the device."""
        out = None
        for i, end in enumerate(self.cutoff):
            start = self.cutoff[i - 1] if i else 0
            emb, proj = self.embeddings[i]
            y = F.linear(F.embedding((tokens - start).clamp(0, end - start - 1), emb.weight), proj.weight)
            out = y if out is None else torch.where((tokens >= start).unsqueeze(-1), y, out)
        return out


class _Tied(nn.Module):
    """A module whose `weight` IS another module's parameter (the state_dict lists it under both names)."""

    def __init__(self, weight):
        super().__init__()
        self.weight = weight


class _TiedHead(nn.Module):
    def __init__(self, band0, input_dim, num_classes):
        super().__init__()
        if band0.shape[1] != input_dim:
            raise NotImplementedError("a tied head whose band-0 width differs from the model width")
        self.word_proj = _Tied(band0)
        self.class_proj = nn.Linear(input_dim, num_classes, bias=False)
        nn.init.xavier_uniform_(self.class_proj.weight)
        self.register_buffer("_float_tensor", torch.zeros(1))

    def table(self):
        return torch.cat([self.word_proj.weight, self.class_proj.weight], 0)


class AdaptiveSoftmax(nn.Module):
    """head: a Linear(input_dim, c0 + n) (`head.weight`), or with adaptive_inputs the tied head (`head.word_proj.weight` is
    band 0's table, `head.class_proj.weight` [n, input_dim]).  tail[i] = Sequential(Q_i, Dropout, table): `tail.i.0.weight` is
    [input_dim, d_i] when tied to the input's projection (used transposed), else [d_i, input_dim]; `tail.i.2.weight` [V_i, d_i]."""

    def __init__(self, vocab_size, input_dim, cutoff, dropout, factor=4.0, adaptive_inputs=None, tie_proj=False, q_noise=0,
                 qn_block_size=8):
        super().__init__()
        _no_q_noise(q_noise)
        self.vocab_size, self.input_dim, self.factor, self.dropout = vocab_size, input_dim, factor, float(dropout)
        self.cutoff = _cutoffs(vocab_size, cutoff)
        n = len(self.cutoff) - 1
        self.tie_proj = bool(tie_proj and adaptive_inputs is not None)
        if adaptive_inputs is not None:
            self.head = _TiedHead(adaptive_inputs.weights_for_band(0)[0], input_dim, n)
        else:
            self.head = nn.Linear(input_dim, self.cutoff[0] + n, bias=False)
            nn.init.xavier_uniform_(self.head.weight)
        self.tail = nn.ModuleList()
        for i in range(n):
            dim = int(input_dim // factor ** (i + 1))
            size = self.cutoff[i + 1] - self.cutoff[i]
            emb, proj = adaptive_inputs.weights_for_band(i + 1) if adaptive_inputs is not None else (None, None)
            if self.tie_proj:
                q = _Tied(proj)
            else:
                q = nn.Linear(input_dim, dim if proj is None else proj.shape[1], bias=False)
                nn.init.xavier_uniform_(q.weight)
            if emb is None:
                table = nn.Linear(dim, size, bias=False)
                nn.init.xavier_uniform_(table.weight)
            else:
                table = _Tied(emb)
            self.tail.append(nn.Sequential(q, nn.Dropout(self.dropout), table))
        self.register_buffer("version", torch.LongTensor([1]))

    # ---- the operands, as the scoring kernel takes them --------------------------------------------------------------------
    def band_dims(self):
        return [self.tail[i][2].weight.shape[1] for i in range(len(self.tail))]

    def head_table(self):
        """[c0 + n, input_dim]: band 0's rows with the class rows behind them."""
        return self.head.table() if isinstance(self.head, _TiedHead) else self.head.weight

    def tail_projection(self, i):
        """[d_i, input_dim], K-contiguous: h = x @ tail_projection(i).t()"""
        w = self.tail[i][0].weight
        return w.t() if self.tie_proj else w

    def tail_table(self, i):
        return self.tail[i][2].weight

    # ---- the slow route ----------------------------------------------------------------------------------------------------
    def _tail_logits(self, i, x):
        h = F.linear(x, self.tail_projection(i))
        return F.linear(self.tail[i][1](h), self.tail_table(i))

    def get_log_prob(self, x, target=None):
        """x [..., input_dim].  target None: log-probabilities of the whole vocabulary, [..., V] (every tail on every row).
        target [...] int64: the targets' log-probabilities alone, shaped like target; tail i runs on the rows whose target
        lies in it only (their indices are read back: this is not the capturable path); a target outside [0, V) gives NaN."""
        lead = x.shape[:-1]
        x = F.dropout(x.reshape(-1, x.shape[-1]), self.dropout, self.training)
        c0, n = self.cutoff[0], len(self.tail)
        head = F.log_softmax(F.linear(x, self.head_table()), dim=-1)
        if target is None:
            parts = [head[:, :c0]]
            for i in range(n):
                parts.append(F.log_softmax(self._tail_logits(i, x), dim=-1) + head[:, c0 + i, None])
            return torch.cat(parts, -1).reshape(*lead, self.vocab_size)
        t = target.reshape(-1)
        out = torch.full((t.numel(),), float("nan"), dtype=head.dtype, device=x.device)
        at = ((t >= 0) & (t < c0)).nonzero().squeeze(1)
        out[at] = head[at, t[at]]
        for i in range(n):
            at = ((t >= self.cutoff[i]) & (t < self.cutoff[i + 1])).nonzero().squeeze(1)
            if at.numel():
                tail = F.log_softmax(self._tail_logits(i, x[at]), dim=-1)
                out[at] = head[at, c0 + i] + tail[torch.arange(at.numel(), device=at.device), t[at] - self.cutoff[i]]
        return out.reshape(target.shape)
