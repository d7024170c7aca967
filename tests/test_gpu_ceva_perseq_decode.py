"""-m gpu: per-sequence token counts of static / rolling incremental decoding (init_*_decoding(per_sequence=True)).

Every batch row has its own count `pos[b]`; of a step's T_new positions a row takes those before its first flag in the
step's key_padding_mask.  Pinned here: with equal counts and no mask the state is the shared-count state bit for bit; every
row of a ragged batch decodes as if it were alone (against forward() on its own tokens); a row's bits do not depend on what
the other rows do, their overflow included; a row restarted by reset_decoding_rows is a fresh sequence whatever its slots
held; the mask's monotone reading; per-row overflow; the beam reorder; the launches of a step.

The drivers: `_Session` holds one state, feeds a right-padded prompt eagerly and then replays ONE captured 1-token step in
which the rows that have nothing to say are flagged.  Its warm-up step flags every row, so it moves nothing."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

from test_gpu_causal_eva import _build                                       # noqa: E402
from ceva_decoding import DTYPES, IDS, STATIC, _Calls, _check_full, _ctx, _geometry, _skip_f32   # noqa: E402

VARIANTS = ["recipe_d64", "recipe_d128", "overlap_d64", "no_rpe_noln", "many_chunks"]
KINDS = ["static", "rolling"]
STATE_ROWS = ("qkv", "pad", "rf_k_bar", "beta")


def _init(m, kind, B, T, dtype, S=None, per=True):
    """A fresh state of `kind`; per=None leaves the new argument out (the shared count as every caller before wrote it)."""
    st, kw = {}, ({} if per is None else {"per_sequence": per})
    if kind == "static":
        m.init_static_decoding(st, B, T, dtype, "cuda", **kw)
    else:
        m.init_rolling_decoding(st, B, T, dtype, "cuda", max_step_tokens=S, **kw)
    return st


def _ring(m, S=None):
    w, e = m.window_size, m.ext_size
    return -(-(w + e + (w if S is None else S)) // w) * w


def _quiet():
    warnings.simplefilter("ignore")


class _Session:
    """One per-sequence state of `kind` for a batch of B rows, and one captured 1-token step on it."""

    def __init__(self, m, kind, dtype, B, C, max_tokens, S=None):
        self.m, self.B, self.C = m, B, C
        self.state = _init(m, kind, B, max_tokens, dtype, S)
        self.graph = None

    def buf(self):
        return self.m._get_input_buffer(self.state)

    def step(self, x, mask):
        return self.m(x, x, x, key_padding_mask=mask, incremental_state=self.state)[0]

    def prefill(self, seqs, p):
        """One eager right-padded step: row b's first p[b] tokens, the rest of its columns flagged -> [max p, B, C]."""
        P = max(p)
        x = torch.zeros(P, self.B, self.C, device="cuda")
        mask = torch.ones(self.B, P, dtype=torch.bool, device="cuda")
        for b in range(self.B):
            x[:p[b], b] = seqs[b][:p[b]]
            mask[b, :p[b]] = False
        return self.step(x, mask)

    def _capture(self):
        self.x = torch.zeros(1, self.B, self.C, device="cuda")
        self.mask = torch.ones(self.B, 1, dtype=torch.bool, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.step(self.x, self.mask)                        # warm-up: every row flagged, nothing moves
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.y = self.step(self.x, self.mask)

    def replay(self, x, mask):
        if self.graph is None:
            self._capture()
        self.x.copy_(x)
        self.mask.copy_(mask)
        self.graph.replay()
        return self.y.clone()

    def run(self, feeds, K=None, hooks=None):
        """feeds: (row, first replay, tokens [n, C]); a row without a token in a replay is flagged.  hooks[k](self) runs
        ahead of replay k.  -> [K, B, C]"""
        K = max(s + len(t) for _, s, t in feeds) if K is None else K
        xs = torch.zeros(K, self.B, self.C, device="cuda")
        mk = torch.ones(K, self.B, dtype=torch.bool, device="cuda")
        for b, s, t in feeds:
            n = min(len(t), K - s)
            xs[s:s + n, b] = t[:n]
            mk[s:s + n, b] = False
        ys = []
        for k in range(K):
            if hooks and k in hooks:
                hooks[k](self)
            ys.append(self.replay(xs[k:k + 1], mk[k].unsqueeze(1)))
        torch.cuda.synchronize()
        return torch.cat(ys, 0)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _state_rows(buf, b):
    return {k: buf[k][b].clone() for k in STATE_ROWS}


def _same_rows(a, b):
    return [k for k in STATE_ROWS if not _bits(a[k], b[k])]


def _zero_row(m, buf, B, C):
    """What the module returns where the attention core delivered a zero row: out_proj of zero, [B, C]."""
    return m._project_out(torch.zeros(1, B, C, dtype=buf["qkv"].dtype, device="cuda"), torch.float32)[0]


# ---- 4. equal counts, no mask: the shared-count state, bit for bit -----------------------------------------------------------
def _steps_over(T, w):
    out, t, cyc, i = [], 0, (w - 3, 1, 1, 5, 17, 1, w, 2, 1, 11), 0
    while t < T:
        out.append(min(cyc[i % len(cyc)], T - t))
        t += out[-1]
        i += 1
    return out


def _uniform(m, x, dtype, kind, per, P=None):
    """x [T, B, C] without a mask.  P = None: eager steps of mixed sizes (all <= w).  P: that many tokens eagerly, a warm-up
    token, then one captured 1-token step replayed for the rest (ceva_decoding._captured_run for one layer)."""
    T, B = x.shape[:2]
    st, rows = _init(m, kind, B, T, dtype, None, per), []
    f = lambda a: m(a, a, a, incremental_state=st)[0]           # noqa: E731
    if P is None:
        t = 0
        for n in _steps_over(T, m.window_size):
            rows.append(f(x[t:t + n]))
            t += n
        return torch.cat(rows, 0), st
    rows.append(f(x[:P]))
    xin = x[P:P + 1].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rows.append(f(xin).clone())
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = f(xin)
    for t in range(P + 1, T):
        xin.copy_(x[t:t + 1])
        g.replay()
        rows.append(y.clone())
    torch.cuda.synchronize()
    return torch.cat(rows, 0), st


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["eager", "replay"])
def test_uniform_equals_shared(dtype, variant, kind, how):
    """The same steps without a mask on a per-sequence and on a shared-count state of the same kind: outputs, qkv, pad,
    rf_k_bar and beta equal bit for bit; the ring (R = 2 w or 3 w) goes round at least twice, and the replays cross its end."""
    _skip_f32(dtype)
    aa, embed, heads, T, B = _geometry(variant)
    m = _build(embed, heads, aa)
    R = _ring(m)
    T = 2 * R + 24
    P = None if how == "eager" else 2 * R - 16
    torch.manual_seed(41)
    x = torch.randn(T, B, embed, device="cuda")
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        want, shared = _uniform(m, x, dtype, kind, None, P)
        got, per = _uniform(m, x, dtype, kind, True, P)
    assert _bits(got, want)
    sb, pb = m._get_input_buffer(shared), m._get_input_buffer(per)
    assert pb["pos"].shape == (B,) and pb["status"].shape == (B,) and pb["ntok"].shape == (B,) and sb["pos"].shape == (1,)
    assert "ntok" not in sb
    for k in STATE_ROWS:
        assert _bits(pb[k], sb[k]), k
    if kind == "rolling":
        assert pb["qkv"].shape[1] == R and T >= 2 * R
    assert m.decoding_positions(per).tolist() == [T] * B == m.decoding_positions(shared).tolist()
    assert not m.static_decoding_overflowed(per) and not m.static_decoding_overflowed_rows(per).any()
    assert m.decoding_state_nbytes(per) == m.decoding_state_nbytes(shared) + 4 * (3 * B - 2)


# ---- 5. each sequence as if alone ---------------------------------------------------------------------------------------------
def _ragged_lengths(w, r, R):
    """Prompt and total lengths of four rows, and the conditions they are chosen for, checked on the host."""
    p = [w + 5, w + r + 3, 5, 2 * w]
    L = [2 * w + 6, 4 * w + 3, 3 * w + 1, max(2 * R + 8, 6 * w + 8)]
    K = max(Lb - pb for Lb, pb in zip(L, p))
    pos = lambda b, k: min(p[b] + k, L[b])                      # noqa: E731  (the row's count ahead of replay k)
    live = lambda b, k: p[b] + k < L[b]                         # noqa: E731
    for pb, Lb in zip(p, L):
        assert pb <= Lb and (Lb - 1) // w >= 2 and Lb // r >= 3              # two block boundaries crossed, three chunks closed
    assert any(live(a, k) and live(b, k) and pos(a, k) % r != pos(b, k) % r and pos(a, k) // w != pos(b, k) // w
               for k in range(K) for a in range(4) for b in range(a))
    # a row idle for r replays in a row while another closes a chunk in them
    assert any(all(not live(a, j) for j in range(k, k + r)) and any(live(b, j) and (pos(b, j) + 1) % r == 0 for j in range(k, k + r))
               for k in range(K - r) for a in range(4) for b in range(4) if a != b)
    assert max(L) >= 2 * R
    return p, L, K


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["many_chunks", "overlap_d64"])
@pytest.mark.parametrize("kind", KINDS)
def test_each_sequence_as_if_alone(dtype, variant, kind):
    """Four rows of different lengths, prefilled in one right-padded step, then decoded by replays of one captured 1-token
    step in which finished rows are flagged: every valid position of every row against forward() on that row's own tokens
    (_check_full's bounds)."""
    _skip_f32(dtype)
    aa, embed, heads, _, _ = _geometry(variant)
    m = _build(embed, heads, aa)
    w, r, R = m.window_size, m.chunk_size, _ring(m)
    p, L, K = _ragged_lengths(w, r, R)
    B = len(L)
    torch.manual_seed(43)
    seqs = [torch.randn(Lb, embed, device="cuda") for Lb in L]
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        ses = _Session(m, kind, dtype, B, embed, max(L))
        pre = ses.prefill(seqs, p)
        ys = ses.run([(b, 0, seqs[b][p[b]:]) for b in range(B)])
        assert ys.shape[0] == K
        fulls = [m(s.unsqueeze(1), s.unsqueeze(1), s.unsqueeze(1))[0][:, 0] for s in seqs]
        zero = _zero_row(m, ses.buf(), B, embed)
    compared = 0
    for b in range(B):
        got = torch.cat([pre[:p[b], b], ys[:L[b] - p[b], b]], 0)
        assert got.shape == fulls[b].shape and torch.isfinite(got).all()
        print("row", b, "length", L[b])
        _check_full(got, fulls[b], dtype)
        compared += got.shape[0]
        # the step positions that are not the row's: out_proj of a zero core row, on every replay
        for rest in (pre[p[b]:, b], ys[L[b] - p[b]:, b]):
            assert _bits(rest, zero[b].to(rest.dtype).expand_as(rest).contiguous())
    assert compared == sum(L)
    assert m.decoding_positions(ses.state).tolist() == L
    assert not m.static_decoding_overflowed(ses.state)
    if kind == "rolling":
        assert ses.buf()["qkv"].shape[1] == R and max(L) >= 2 * R


# ---- 6. isolation -------------------------------------------------------------------------------------------------------------
def _small():
    aa, embed, heads, _, _ = _geometry("many_chunks")           # w 32, e 32, r 4, 4 heads of 64
    return _build(embed, heads, aa), embed


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_row_zero_does_not_depend_on_the_other_rows(dtype, kind):
    """Two runs with the same step shapes and the same tokens for row 0; the other rows get other tokens, other lengths, and
    in the second run one of them passes cap: row 0's outputs (every position of every step) and state rows equal bit for bit."""
    _skip_f32(dtype)
    m, C = _small()
    w = m.window_size
    cap, B, K = 8 * w, 4, 5 * w
    torch.manual_seed(47)
    row0 = torch.randn(3 * w + 9, C, device="cuda")
    runs = []
    for seed, p, L in ((1, [w + 5, 7, 40, 2 * w], [3 * w + 9, 100, 90, 4 * w]),
                       (2, [w + 5, 2 * w, 3, 2 * w - 1], [3 * w + 9, 70, 5 * w, cap + 20])):
        torch.manual_seed(seed)
        seqs = [row0] + [torch.randn(Lb, C, device="cuda") for Lb in L[1:]]
        with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
            _quiet()
            ses = _Session(m, kind, dtype, B, C, cap)
            assert max(p) == 2 * w                                  # the same prefill shape in both runs
            pre = ses.prefill(seqs, p)
            # the last row of the second run is fed from replay 0 to the end: it reaches cap inside the run
            ys = ses.run([(b, 0, seqs[b][p[b]:]) for b in range(B)], K=K if seed == 1 else max(K, cap + 2 - p[3]))
        runs.append((pre[:, 0].clone(), ys[:K, 0].clone(), _state_rows(ses.buf(), 0), m.decoding_positions(ses.state),
                     m.static_decoding_overflowed_rows(ses.state)))
    a, b = runs
    assert _bits(a[0], b[0]) and _bits(a[1], b[1]) and not _same_rows(a[2], b[2])
    assert a[3][0] == b[3][0] == len(row0)
    assert not a[4].any() and b[4].tolist() == [False, False, False, True] and b[3][3] == cap


# ---- 7. slot reuse ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("reset", ["eager", "captured"])
def test_a_reset_row_is_a_fresh_sequence(dtype, kind, reset):
    """Row 1 finishes, is restarted by reset_decoding_rows while the others are mid-sequence, has its state rows poisoned, and
    takes a new sequence through the same captured step: its outputs equal those of that sequence fed from step 0 into a fresh
    state by the same 1-token steps, the other rows' outputs equal a run without the reset -- all bit for bit."""
    _skip_f32(dtype)
    m, C = _small()
    w, B = m.window_size, 3
    p, L = [w + 5, 9, 2 * w], [4 * w + 2, 30, 5 * w]
    k0, new_len = 40, 2 * w + 7                                    # row 1 ends after 21 replays; restarted ahead of replay 40
    K = k0 + new_len
    torch.manual_seed(53)
    seqs = [torch.randn(Lb, C, device="cuda") for Lb in L]
    fresh = torch.randn(new_len, C, device="cuda")

    def restart(ses):
        rows = torch.tensor([1], device="cuda")
        if reset == "captured":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                m.reset_decoding_rows(ses.state, rows)
            g.replay()
        else:
            m.reset_decoding_rows(ses.state, [1])
        buf = ses.buf()
        for k in ("qkv", "rf_k_bar", "beta"):
            buf[k][1] = float("nan")
        buf["pad"][1] = 1

    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        feeds = [(b, 0, seqs[b][p[b]:]) for b in range(B)]
        plain = _Session(m, kind, dtype, B, C, max(L))
        plain.prefill(seqs, p)
        want_others = plain.run(feeds, K=K)
        ses = _Session(m, kind, dtype, B, C, max(L))
        ses.prefill(seqs, p)
        got = ses.run(feeds + [(1, k0, fresh)], K=K, hooks={k0: restart})
        alone = _Session(m, kind, dtype, B, C, max(L))
        want_fresh = alone.run([(1, 0, fresh)])
    assert _bits(got[:, 0], want_others[:, 0]) and _bits(got[:, 2], want_others[:, 2])
    assert _bits(got[:k0, 1], want_others[:k0, 1])
    assert torch.isfinite(got[k0:, 1]).all() and _bits(got[k0:, 1], want_fresh[:, 1])
    assert m.decoding_positions(ses.state).tolist() == [min(L[0], p[0] + K), new_len, min(L[2], p[2] + K)]
    assert m.decoding_positions(alone.state).tolist() == [0, new_len, 0]


# ---- 8. the mask ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_mask_semantics(dtype, kind):
    """A non-monotone mask == its monotone closure; rows past n_b are out_proj of a zero row; the counts are the lengths; and
    the helpers on a shared-count state."""
    _skip_f32(dtype)
    m, C = _small()
    B, T = 4, 19                                                # (rows of 19 flags: no 16-byte aligned row but the first)
    torch.manual_seed(59)
    x0, x = torch.randn(11, B, C, device="cuda"), torch.randn(T, B, C, device="cuda")
    holes = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    holes[0, 7], holes[0, 12] = True, True                       # 7 tokens, however many unflagged columns follow
    holes[1, 0] = True                                          # none
    holes[2, T - 1] = True                                      # T - 1; row 3: all T
    closure = holes.long().cumsum(1) > 0
    n = [7, 0, T - 1, T]
    outs = []
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        for mask in (holes, closure, torch.cat([torch.zeros(B, 11, dtype=torch.bool, device="cuda"), holes], 1)):
            st = _init(m, kind, B, 64, dtype)
            m(x0, x0, x0, incremental_state=st)                  # 11 tokens everywhere first: the step starts inside a chunk
            y = m(x, x, x, key_padding_mask=mask, incremental_state=st)[0]
            outs.append((y, {k: m._get_input_buffer(st)[k].clone() for k in STATE_ROWS}, m.decoding_positions(st).tolist(),
                         m._get_input_buffer(st)["ntok"].tolist()))
        zero = _zero_row(m, m._get_input_buffer(st), B, C)
        shared = _init(m, kind, B, 64, dtype, per=False)
        m(x0, x0, x0, incremental_state=shared)
    for other in outs[1:]:                                      # (the third: fairseq's mask of every position so far)
        assert _bits(outs[0][0], other[0]) and not _same_rows(outs[0][1], other[1]) and outs[0][2:] == other[2:]
    assert outs[0][2] == [11 + v for v in n] and outs[0][3] == n
    y = outs[0][0]
    for b in range(B):
        assert torch.isfinite(y[:, b]).all()
        assert _bits(y[n[b]:, b], zero[b].to(y.dtype).expand_as(y[n[b]:, b]).contiguous())
        if n[b]:
            assert not _bits(y[:n[b], b], zero[b].to(y.dtype).expand_as(y[:n[b], b]).contiguous())
    assert not outs[0][1]["pad"].any()                          # no pad flag is stored for anything
    with pytest.raises(RuntimeError, match="per-sequence"):
        m.reset_decoding_rows(shared, [0])
    assert m.decoding_positions(shared).tolist() == [11] * B
    assert m.static_decoding_overflowed_rows(shared).tolist() == [False] * B


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_long_ragged_prompt_through_the_ring(dtype):
    """A ragged prompt longer than max_step_tokens in ONE call on a rolling state (the module cuts it into pieces) == a
    static state that the test feeds the same pieces with the matching slices of the mask: bit for bit at every valid
    position, zero-row outputs elsewhere, equal counts and landmarks."""
    _skip_f32(dtype)
    m, C = _small()
    w, B, S = m.window_size, 4, 20
    n = [150, 3, 41, 97]                                        # ends inside a piece, inside the first piece, on the last
    P = max(n)
    torch.manual_seed(61)
    x = torch.randn(P, B, C, device="cuda")
    mask = torch.ones(B, P, dtype=torch.bool, device="cuda")
    for b in range(B):
        mask[b, :n[b]] = False
    mask[3, 120] = False                                        # a hole after row 3's end, in a later piece: still ended
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        rol = _init(m, "rolling", B, 4 * w * 2, dtype, S=S)
        got = m(x, x, x, key_padding_mask=mask, incremental_state=rol)[0]
        sta = _init(m, "static", B, 4 * w * 2, dtype)
        closed = mask.long().cumsum(1) > 0
        want = torch.cat([m(x[a:a + S], x[a:a + S], x[a:a + S], key_padding_mask=closed[:, a:a + S], incremental_state=sta)[0]
                          for a in range(0, P, S)], 0)
    assert _ring(m, S) == 3 * w and m._get_input_buffer(rol)["qkv"].shape[1] == 3 * w and P > 3 * w
    assert _bits(got, want)
    assert m.decoding_positions(rol).tolist() == n == m.decoding_positions(sta).tolist()
    rb, sb = m._get_input_buffer(rol), m._get_input_buffer(sta)
    for b in range(B):
        c = n[b] // m.chunk_size
        assert _bits(rb["rf_k_bar"][b, :, :c], sb["rf_k_bar"][b, :, :c]) and _bits(rb["beta"][b, :, :c], sb["beta"][b, :, :c])


# ---- 9. overflow per row ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_overflow_is_per_row(dtype, kind):
    """By replay, row 1 passes cap: its flag is set, its output rows are NaN, its count and every byte of its state rows stay;
    the other rows' outputs equal, bit for bit, a run in which row 1 stops at cap."""
    _skip_f32(dtype)
    m, C = _small()
    w, B = m.window_size, 3
    cap = 4 * w
    p, extra = [w + 1, cap - 3, 7], 4                            # row 1: three more tokens fit, then `extra` do not
    K = 3 + extra + 2
    torch.manual_seed(67)
    seqs = [torch.randn(cap + 8, C, device="cuda") for _ in range(B)]
    snap = {}
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        ref = _Session(m, kind, dtype, B, C, cap)
        ref.prefill(seqs, p)
        want = ref.run([(0, 0, seqs[0][p[0]:p[0] + K]), (1, 0, seqs[1][p[1]:cap]), (2, 0, seqs[2][p[2]:p[2] + K])], K=K)
        ses = _Session(m, kind, dtype, B, C, cap)
        ses.prefill(seqs, p)
        got = ses.run([(0, 0, seqs[0][p[0]:p[0] + K]), (1, 0, seqs[1][p[1]:cap + extra]), (2, 0, seqs[2][p[2]:p[2] + K])], K=K,
                      hooks={3: lambda s: snap.update(_state_rows(s.buf(), 1))})
    assert _bits(got[:, 0], want[:, 0]) and _bits(got[:, 2], want[:, 2]) and _bits(got[:3, 1], want[:3, 1])
    assert torch.isnan(got[3:3 + extra, 1]).all() and torch.isfinite(got[3 + extra:, 1]).all()
    assert m.static_decoding_overflowed(ses.state) and m.static_decoding_overflowed_rows(ses.state).tolist() == [False, True, False]
    assert not m.static_decoding_overflowed(ref.state)
    assert m.decoding_positions(ses.state).tolist() == [p[0] + K, cap, p[2] + K] == m.decoding_positions(ref.state).tolist()
    assert not _same_rows(snap, _state_rows(ses.buf(), 1)) and not _same_rows(snap, _state_rows(ref.buf(), 1))


# ---- 10. beam reorder ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_reorder_permutes_the_counts_with_the_rows(dtype, kind):
    """reorder_incremental_state between replays == a run started in the permuted order."""
    _skip_f32(dtype)
    m, C = _small()
    w, B = m.window_size, 4
    p, L = [w + 5, 3, 2 * w, 17], [3 * w + 9, 2 * w + 30, 4 * w, 80]
    order = [2, 2, 0, 3]                                        # beams: row 2 survives twice, row 1 dies
    k1, K = 25, 70
    torch.manual_seed(71)
    seqs = [torch.randn(Lb + K, C, device="cuda") for Lb in L]
    tails = [torch.randn(K, C, device="cuda") for _ in range(B)]            # what each NEW row says after the reorder
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        a = _Session(m, kind, dtype, B, C, 8 * w)
        a.prefill(seqs, p)
        idx = torch.tensor(order, device="cuda")
        feeds = [(b, 0, seqs[b][p[b]:p[b] + k1]) for b in range(B)] + [(b, k1, tails[b][:K - k1]) for b in range(B)]
        got = a.run(feeds, K=K, hooks={k1: lambda s: m.reorder_incremental_state(s.state, idx)})
        b_ = _Session(m, kind, dtype, B, C, 8 * w)
        b_.prefill([seqs[o] for o in order], [p[o] for o in order])
        feeds = [(b, 0, seqs[o][p[o]:p[o] + k1]) for b, o in enumerate(order)] + [(b, k1, tails[b][:K - k1]) for b in range(B)]
        want = b_.run(feeds, K=K)
    assert _bits(got[k1:], want[k1:])
    assert _bits(got[:k1][:, order], want[:k1])
    assert m.decoding_positions(a.state).tolist() == m.decoding_positions(b_.state).tolist() == [p[o] + K for o in order]
    ab, bb = a.buf(), b_.buf()
    for k in ("pos", "status", "ntok"):
        assert torch.equal(ab[k], bb[k]), k


# ---- 11. launches -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_a_per_sequence_step_is_the_same_four_launches(kind):
    m, C = _small()
    B, dtype = 3, torch.bfloat16
    torch.manual_seed(73)
    x = torch.randn(9, B, C, device="cuda")
    mask = torch.zeros(B, 9, dtype=torch.bool, device="cuda")
    mask[1, 4:] = True
    mask[2] = True
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        _quiet()
        st = _init(m, kind, B, 64, dtype)
        with _Calls() as calls:
            for kpm in (None, mask, mask[:, :1]):
                calls.step()
                n = 9 if kpm is None or kpm.shape[1] == 9 else 1
                m(x[:n], x[:n], x[:n], key_padding_mask=kpm, incremental_state=st)
    for step in calls.steps:
        # (as tests/test_gpu_ceva_static_decode.py counts a step: the projections around the attention core set aside)
        assert [c for c in step if not (c.startswith("ea_linear") or c == "ea_multi_cast")] == list(STATIC), step
    assert m.decoding_positions(st).tolist() == [19, 14, 9]
