"""Per-token latency of CausalEVAttention decoding at the wikitext-103 LM geometry (embed 1024, h 8, d 128, w 128, chunks of 8,
T5 bias, adaptive 'qk'), 16 stacked residual attention layers (x + attn(x), no FFN), bf16 autocast, in eighteen modes:
 - dynamic:       the incremental state of `_decode` (host token count, two decode launches per layer step);
 - static:        `init_static_decoding`, the same step run eagerly (four decode launches per layer step);
 - graph:         that static step over all 16 layers captured once with torch.cuda.graph and replayed;
 - rolling:       `init_rolling_decoding`, the static step on a state whose token rows live in a ring, eager;
 - rolling-graph: that step captured and replayed;
 - per-seq, per-seq-graph, per-seq-rolling-graph: static, graph and rolling-graph on a state with per-sequence token counts
   (`per_sequence=True`), every row at the same count and no mask, so that the rows compare bitwise with the other modes.
 - split-graph, split-rolling-graph, per-seq-split-graph, per-seq-split-rolling-graph: graph, rolling-graph and their
   per-sequence twins on a state made with `landmark_splits=P` (`--splits P`, default 256 / (B h)): the 1-token step runs attn
   as attn_split + merge, P workgroups per (b, h).  Their rows differ from the unsplit modes' in rounding (another order of
   the partial sums) and equal each other bitwise; the printed comparison reports the largest difference where rows differ.
 - held-graph, held-rolling-graph, held-split-rolling-graph: graph, rolling-graph and split-rolling-graph on a state made with
   `hold_projections=True`: the 1-token step runs its two projections on ea_ceva_sdecode_linear over the 16-bit weights the
   state holds, and no framework kernel touches a weight.  Their rows differ from the other modes' in rounding (the query is
   rounded before the products, another order of the sums).
 - compact-graph, compact-rolling-graph, compact-split-rolling-graph: graph, rolling-graph and split-rolling-graph on a state
   made with `compact_landmarks=True`: rf_k_bar and beta are bf16, and the step runs close, attn and attn_split on the `_l16`
   entry points.  Their rows differ from the plain modes' by the one rounding of the landmark rows: for these modes the
   "rows equal" column always reports the distance to the first mode's rows, never bitwise equality.
   python tools/ceva_decode_latency.py [--context 512|4096|32768] [--steps 64] [--splits P] [--modes dynamic,static,graph,...]   (GPU)
   python tools/ceva_decode_latency.py --ragged [--context 512] [--steps 64]     (GPU)
`--ragged`: batch 8 on per-sequence states, row b prefilled to (b + 1) / 8 of `context` by right-padded steps, then the
captured 1-token step replayed with every row live -- rows at eight different counts in one replay -- next to the same
modes with all rows at `context`; prints the replay time of both and the bytes the per-sequence tensors add to a state.
A 1-token step after a prefill of `context` tokens, fed in pieces of one window (the largest step of a rolling state) in
every mode, so that all modes run one sequence of step sizes; a warm-up, then the median over 5 blocks of `steps` tokens,
each block timed by the host clock around its steps and a device synchronise.  The rows of the modes are compared (bitwise)
with those of the first mode, and the bytes of one layer's decoding state at `context` tokens are printed for the static and
the rolling state (`decoding_state_nbytes`: allocation sizes); `--state-bytes 512,4096,32768` prints only those."""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd")]
import torch  # noqa: E402
import efficient_attention as ea  # noqa: E402

warnings.simplefilter("ignore")
EMBED, HEADS, LAYERS = 1024, 8, 16
RECIPE = dict(window_size=128, chunk_size=8, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
              overlap_window=False)


def build():
    torch.manual_seed(0)
    return [ea.AttentionFactory.build_attention(
        "causal_eva", dict(embed_dim=EMBED, num_heads=HEADS, self_attention=True, dropout=0.0,
                           attn_args=argparse.Namespace(**RECIPE))).cuda().eval() for _ in range(LAYERS)]


def step(mods, states, x, mask=None):
    for m, st in zip(mods, states):
        x = x + m(x, x, x, key_padding_mask=mask, incremental_state=st)[0]
    return x


def default_splits(B):
    """About 256 / (B h) workgroups per (b, h) fill the device."""
    return max(2, min(64, 256 // (B * HEADS)))


def run(mods, mode, B, context, steps, blocks=5, warmup=4, lengths=None, splits=None):
    """-> (median ms per token, the rows of every timed step).  lengths (per-seq modes): row b is prefilled to lengths[b] <=
    context tokens instead of `context`.  splits (split modes): landmark_splits of the states, default_splits(B) when None."""
    n_tok = context + warmup + 1 + blocks * steps
    torch.manual_seed(1)
    x = 0.5 * torch.randn(n_tok, B, EMBED, device="cuda")
    states = []
    opt = dict(per_sequence=True) if mode.startswith("per-seq") else {}
    if "split" in mode:
        opt["landmark_splits"] = splits or default_splits(B)
    if mode.startswith("held-"):
        opt["hold_projections"] = True
    if mode.startswith("compact-"):
        opt["compact_landmarks"] = True
    for m in mods:
        st = {}
        m.init_incremental_state()
        if mode != "dynamic":
            init = m.init_rolling_decoding if "rolling" in mode else m.init_static_decoding
            init(st, B, n_tok, torch.bfloat16, "cuda", **opt)
        states.append(st)
    ends = None if lengths is None else torch.tensor(lengths, device="cuda").unsqueeze(1)
    rows, times = [], []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        for a in range(0, context, RECIPE["window_size"]):
            b = min(a + RECIPE["window_size"], context)
            step(mods, states, x[a:b], None if ends is None else torch.arange(a, b, device="cuda").unsqueeze(0) >= ends)
        t = context
        xin = x[t:t + 1].clone()
        if mode.endswith("graph"):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step(mods, states, xin)                       # the token at `context`, eager on a side stream
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                yout = step(mods, states, xin)

            def one(tok):
                xin.copy_(x[tok:tok + 1])
                g.replay()
                return yout.clone()
        else:
            step(mods, states, xin)

            def one(tok):
                return step(mods, states, x[tok:tok + 1])
        t += 1
        for _ in range(warmup):
            one(t)
            t += 1
        torch.cuda.synchronize()
        for _ in range(blocks):
            t0 = time.perf_counter()
            for _ in range(steps):
                rows.append(one(t))
                t += 1
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / steps)
    return sorted(times)[len(times) // 2], torch.cat(rows, 0)


MODES = ("dynamic", "static", "graph", "rolling", "rolling-graph", "per-seq", "per-seq-graph", "per-seq-rolling-graph",
         "split-graph", "split-rolling-graph", "per-seq-split-graph", "per-seq-split-rolling-graph",
         "held-graph", "held-rolling-graph", "held-split-rolling-graph",
         "compact-graph", "compact-rolling-graph", "compact-split-rolling-graph")
CONTEXTS = (512, 4096, 32768)


def ragged(mods, context, steps):
    B = 8
    lengths = [max(1, context * (b + 1) // B) for b in range(B)]
    print("ms per token, %d layers, bf16, batch %d, per-sequence counts: rows at %s tokens against all rows at %d"
          % (LAYERS, B, lengths, context))
    for mode in ("per-seq-graph", "per-seq-rolling-graph"):
        even, rag = run(mods, mode, B, context, steps)[0], run(mods, mode, B, context, steps, lengths=lengths)[0]
        print("%22s  uniform %.3f  ragged %.3f" % (mode, even, rag), flush=True)
    m = mods[0]
    for name, init in (("static", m.init_static_decoding), ("rolling", m.init_rolling_decoding)):
        one, per = {}, {}
        init(one, B, context, torch.bfloat16, "cuda")
        init(per, B, context, torch.bfloat16, "cuda", per_sequence=True)
        print("    decoding_state_nbytes per layer, %d tokens, batch %d, %s: shared count %d, per-sequence %d (+%d)"
              % (context, B, name, m.decoding_state_nbytes(one), m.decoding_state_nbytes(per),
                 m.decoding_state_nbytes(per) - m.decoding_state_nbytes(one)), flush=True)


def state_bytes(m, B, context, **opt):
    """decoding_state_nbytes of one layer with room for `context` tokens -> (static, rolling)."""
    out = []
    for init in (m.init_static_decoding, m.init_rolling_decoding):
        st = {}
        init(st, B, context, torch.bfloat16, "cuda", **opt)
        out.append(m.decoding_state_nbytes(st))
    return tuple(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=512, help="tokens before the timed steps; DESIGN.md 4a uses %s" % (CONTEXTS,))
    ap.add_argument("--splits", type=int, default=None, metavar="P",
                    help="landmark_splits of the split modes (default: 256 / (B h), i.e. 32 at batch 1 and 4 at batch 8)")
    ap.add_argument("--batches", default="1,8", help="comma-separated batch sizes")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--state-bytes", default=None, metavar="CONTEXTS",
                    help="only print the state sizes at these comma-separated contexts (batch 1), no timing")
    ap.add_argument("--ragged", action="store_true", help="replay time with the rows of a batch of 8 at different counts")
    a = ap.parse_args()
    if a.ragged:
        ragged(build(), a.context, a.steps)
        return
    if a.state_bytes:
        m = build()[0]
        for ctx in [int(c) for c in a.state_bytes.split(",")]:
            sb, rb = state_bytes(m, 1, ctx)
            print("decoding_state_nbytes per layer, %d tokens, batch 1: static %d, rolling %d" % (ctx, sb, rb), flush=True)
            cs, cr = state_bytes(m, 1, ctx, compact_landmarks=True)
            print("    compact_landmarks: static %d, rolling %d" % (cs, cr), flush=True)
        return
    modes = [m for m in a.modes.split(",") if m]
    if [m for m in modes if m not in MODES]:
        ap.error("--modes: a comma-separated subset of %s" % (MODES,))
    mods = build()
    print("ms per token, %d layers, bf16, context %d" % (LAYERS, a.context))
    print("%3s " % "B" + " ".join("%13s" % m for m in modes) + "  rows equal (%s vs %s)" % (", ".join(modes[1:]), modes[0]))
    for B in [int(b) for b in a.batches.split(",")]:
        res = {mode: run(mods, mode, B, a.context, a.steps, splits=a.splits) for mode in modes}
        ref = res[modes[0]][1]
        def dist(mode):                                       # (compact modes: the distance, also where it is 0)
            return "max |d| %.2e" % (res[mode][1].float() - ref.float()).abs().max().item()
        same = [dist(mode) if mode.startswith("compact-") else torch.equal(res[mode][1], ref) or dist(mode) for mode in modes[1:]]
        print("%3d " % B + " ".join("%13.3f" % res[m][0] for m in modes) + "  %s" % same, flush=True)
        sb, rb = state_bytes(mods[0], B, a.context)
        print("    decoding_state_nbytes per layer, %d tokens, batch %d: static %d, rolling %d" % (a.context, B, sb, rb),
              flush=True)
        if [m for m in modes if m.startswith("held-")]:
            hs, hr = state_bytes(mods[0], B, a.context, hold_projections=True)
            print("    hold_projections: static %d, rolling %d (+ %d bytes per layer: the 16-bit projections and the staging rows)"
                  % (hs, hr, hs - sb), flush=True)
        if [m for m in modes if m.startswith("compact-")]:
            cs, cr = state_bytes(mods[0], B, a.context, compact_landmarks=True)
            print("    compact_landmarks: static %d, rolling %d (- %d bytes per layer: rf_k_bar and beta in bf16)"
                  % (cs, cr, sb - cs), flush=True)
        if [m for m in modes if "split" in m]:
            P = a.splits or default_splits(B)
            print("    landmark_splits %d: + %d bytes of workspace per layer" % (P, B * HEADS * 8 * P * (EMBED // HEADS + 4) * 4),
                  flush=True)


if __name__ == "__main__":
    main()
