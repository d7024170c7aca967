"""What the GPU tests of causal EVA's incremental decoding share (test_gpu_ceva_decode.py, test_gpu_ceva_static_decode.py,
test_gpu_ceva_rolling_decode.py): the entry-point names of each family, the tolerances, the geometries, a recorder of the
C-ABI calls of each step, and the drivers that decode a sequence on a state of a given kind, eagerly or by capture and
replay.  A plain module, not collected."""
import pytest
import torch

from test_gpu_causal_eva import RECIPE

F32_TOL = (2e-4, 1e-4)                                   # max |d| / max |ref|, rms(d) / rms(ref)
DECODE = ("ea_ceva_decode_close", "ea_ceva_decode_attn")
OLD = ("ea_window_attn_fwd", "ea_f32_attn_fwd")


def _err(got, ref, live=None):
    d = (got.double() - ref.double())
    r = ref.double()
    if live is not None:
        d, r = d * live, r * live
    return (d.abs().max() / r.abs().max().clamp_min(1e-30)).item(), (d.pow(2).mean().sqrt() / r.pow(2).mean().sqrt().clamp_min(1e-30)).item()


class _Calls:
    """Every C-ABI entry point called inside the block, one list per decoding step (nv.call patched as in test_gpu_f32_cores.py)."""

    def __enter__(self):
        from efficient_attention import _native as nv
        self.nv, self.real, self.steps = nv, nv.call, []
        nv.call = lambda nm, *a: (self.steps[-1].append(nm) if self.steps else None, self.real(nm, *a))[1]
        return self

    def step(self):
        self.steps.append([])

    def __exit__(self, *exc):
        self.nv.call = self.real

    def all(self):
        return [c for s in self.steps for c in s]


STATIC = ("ea_ceva_sdecode_append", "ea_ceva_sdecode_close", "ea_ceva_sdecode_attn", "ea_ceva_sdecode_advance")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "fp32"]

def _geometry(variant):
    aa = dict(RECIPE)
    embed, heads, T, B = 512, 8, 300, 2
    if variant == "recipe_d128":
        embed, heads, T = 1024, 8, 200
    elif variant == "overlap_d64":
        aa.update(overlap_window=True, window_size=32)
        T = 150
    elif variant == "no_rpe_noln":
        aa.update(use_t5_rpe=False, adaptive_proj="no-ln", window_size=64, chunk_size=16)
        T = 200
    elif variant == "many_chunks":
        aa.update(overlap_window=True, window_size=32, chunk_size=4)
        embed, heads, T = 256, 4, 300
    return aa, embed, heads, T, B


def _skip_f32(dtype):
    from efficient_attention import _f32
    if dtype == torch.float32 and not _f32.ENABLED:
        pytest.skip("the fp32 cores are switched off (EA_F32_CORES=0)")


def _ctx(dtype):
    """16-bit: autocast (without its weight-cast cache, which a capture may not use); fp32: the fp32 path outside autocast."""
    if dtype == torch.float32:
        return torch.autocast("cuda", enabled=False)
    return torch.autocast("cuda", dtype=dtype, cache_enabled=False)


def _init(m, kind, B, T, dtype, S=None):
    """A fresh incremental state of `kind`.  (The module keeps the key it was built with: states made here stay readable
    side by side.)"""
    st = {}
    if kind == "static":
        m.init_static_decoding(st, B, T, dtype, "cuda")
    elif kind == "rolling":
        m.init_rolling_decoding(st, B, T, dtype, "cuda", max_step_tokens=S)
    return st


def _decode(m, x, steps, kind, dtype, pad=None, S=None, calls=None, before=None):
    """Decode x [T, B, C] in steps of the given sizes, then single tokens, on a state of `kind` ("static" | "rolling" |
    "dynamic"); before(state, t): called ahead of every step with the tokens decoded so far.  -> per-step outputs, state."""
    T, B = x.shape[:2]
    state, rows, t = _init(m, kind, B, T, dtype, S), [], 0
    for i, step in enumerate(list(steps) + [1] * T):
        if t >= T:
            break
        n = min(step, T - t)
        kpm = None if pad is None else (pad[:, t:t + n] if i % 2 == 0 else pad[:, :t + n])
        if before is not None:
            before(state, t)
        if calls is not None:
            calls.step()
        rows.append(m(x[t:t + n], x[t:t + n], x[t:t + n], key_padding_mask=kpm, incremental_state=state)[0])
        t += n
    return rows, state


def _check_full(got, full, dtype, live=None):
    """The project's bounds against the full forward: F32_TOL for fp32, 2e-2 of max |ref| for 16-bit rows."""
    if dtype == torch.float32:
        e = _err(got, full, live)
        print("fp32 (max, rms) error vs full forward:", e)
        assert e[0] <= F32_TOL[0] and e[1] <= F32_TOL[1], e
    else:
        d = (got.float() - full.float()).abs()
        if live is not None:
            d = d * live
        print("16-bit max |d|, bound:", d.max().item(), 2e-2 * full.float().abs().max().item())
        assert d.max().item() <= 2e-2 * full.float().abs().max().item()


def _stack_step(mods, states, x):
    """Residual layers y = h + attn(h), one incremental state per layer."""
    h = x
    for m, st in zip(mods, states):
        h = h + m(h, h, h, incremental_state=st)[0]
    return h


def _captured_run(mods, x, P, dtype, kind="rolling", S=None, reorder=None, order=None, graph_reorder=False):
    """Decoding of x [T, B, C] through the residual stack on states of `kind`: P tokens eagerly (in pieces of at most the
    step bound), a warm-up step on a side stream, the capture of one 1-token step whose input is a static tensor, and replays
    for the remaining tokens.  reorder: before the replay of token `reorder` the states are permuted by `order` (in a captured
    graph when graph_reorder) and the inputs from there on are x[:, order].  -> [T - P, B, C] rows, states."""
    T, B = x.shape[:2]
    states = [_init(m, kind, B, T, dtype, S) for m in mods]
    xr = x if order is None else x[:, order]
    rows = []
    _stack_step(mods, states, x[:P])
    xin = x[P:P + 1].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rows.append(_stack_step(mods, states, xin).clone())             # warm-up: token P, eager
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yout = _stack_step(mods, states, xin)
    greo = None
    if reorder is not None and graph_reorder:
        static_order = order.clone()
        greo = torch.cuda.CUDAGraph()
        with torch.cuda.graph(greo):
            for m, st in zip(mods, states):
                m.reorder_incremental_state(st, static_order)
    for t in range(P + 1, T):
        if reorder is not None and t == reorder:
            if greo is not None:
                greo.replay()
            else:
                for m, st in zip(mods, states):
                    m.reorder_incremental_state(st, order)
        src = xr if (reorder is not None and t >= reorder) else x
        xin.copy_(src[t:t + 1])
        g.replay()
        rows.append(yout.clone())
    torch.cuda.synchronize()
    return torch.cat(rows, 0), states
