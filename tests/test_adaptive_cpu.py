"""-m "not gpu": adaptive input and adaptive softmax (ea_harness/adaptive.py, DecoderStack(adaptive=...)) and the C ABI 33
entries (ea_adaptive_route, ea_vocab_score_rows, ea_adaptive_score): keys and shapes against the reference's tables
(tests/golden/adaptive_keys.json), values against its arrays (tests/golden/adaptive_small.npz), the routing reference against
a plain loop, and the header, the binding table and the workspace queries, which run without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import adaptive_score_reference as aref
import vocab_score_reference as vref
from test_cabi import HEADER, declared_symbols

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = json.load(open(os.path.join(GOLDEN, "adaptive_keys.json")))
ATTN = dict(window_size=4, chunk_size=2, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
NEW = {"ea_adaptive_route": 8, "ea_vocab_score_rows_ws": 2, "ea_vocab_score_rows": 23, "ea_adaptive_score_ws": 4,
       "ea_adaptive_score": 18}


def _modules(entry):
    from ea_harness.adaptive import AdaptiveInput, AdaptiveSoftmax
    g = entry["geometry"]
    inp = AdaptiveInput(g["V"], g["pad"], g["C"], g["factor"], g["C"], list(g["cutoff"]))
    out = AdaptiveSoftmax(g["V"], g["C"], list(g["cutoff"]), 0.0, factor=g["factor"],
                          adaptive_inputs=inp if entry["tie_weights"] else None, tie_proj=entry["tie_proj"])
    return inp, out


def _shapes(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def _small_state():
    """The fixture's state dict under the stack's names, the tied entries filled in from the input's."""
    d = np.load(os.path.join(GOLDEN, "adaptive_small.npz"))
    sd = {k: torch.from_numpy(d[k]) for k in d.files if k.startswith(("embed_tokens.", "adaptive_softmax."))}
    sd["adaptive_softmax.head.word_proj.weight"] = sd["embed_tokens.embeddings.0.0.weight"]
    for i in range(2):
        sd["adaptive_softmax.tail.%d.0.weight" % i] = sd["embed_tokens.embeddings.%d.1.weight" % (i + 1)]
        sd["adaptive_softmax.tail.%d.2.weight" % i] = sd["embed_tokens.embeddings.%d.0.weight" % (i + 1)]
    return d, sd


# ---- C1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_tied", "small_untied_proj", "small_untied"])
def test_c1_modules_have_the_references_keys_and_shapes(name):
    entry = KEYS[name]
    inp, out = _modules(entry)
    assert _shapes(inp) == entry["input"] and _shapes(out) == entry["output"]
    inp.load_state_dict({k: torch.zeros(s) for k, s in entry["input"].items()}, strict=True)
    out.load_state_dict({k: torch.zeros(s, dtype=torch.long if k == "version" else torch.float32)
                         for k, s in entry["output"].items()}, strict=True)
    if entry["tie_weights"]:
        assert out.head.word_proj.weight is inp.embeddings[0][0].weight
        assert all(out.tail[i][2].weight is inp.embeddings[i + 1][0].weight for i in range(2))
        assert all((out.tail[i][0].weight is inp.embeddings[i + 1][1].weight) == entry["tie_proj"] for i in range(2))


def test_c1_the_recipes_geometry_on_the_meta_device():
    entry = KEYS["recipe"]
    assert entry["geometry"]["cutoff"] == [20000, 60000] and entry["geometry"]["V"] == 267744
    with torch.device("meta"):
        inp, out = _modules(entry)
    assert _shapes(inp) == entry["input"] and _shapes(out) == entry["output"]
    assert out.band_dims() == [256, 64]


def test_c1_the_stack_takes_a_reference_checkpoints_decoder_keys():
    from ea_harness import sequence as sq
    entry = KEYS["small_tied"]
    g = entry["geometry"]
    adaptive = dict(cutoff=g["cutoff"], factor=g["factor"])
    stack = sq.DecoderStack(g["V"], g["C"], 256, 2, 2, ATTN, pad_idx=g["pad"], adaptive=adaptive)
    plain = sq.DecoderStack(g["V"], g["C"], 256, 2, 2, ATTN, pad_idx=g["pad"])
    got = {k: list(v.shape) for k, v in stack.state_dict().items()}
    want = {"embed_tokens." + k: s for k, s in entry["input"].items()}
    want.update({"adaptive_softmax." + k: s for k, s in entry["output"].items()})
    assert {k: s for k, s in got.items() if k.startswith(("embed_tokens.", "adaptive_softmax."))} == want
    assert "embed_tokens.weight" not in got
    # without the option: today's members and keys
    mine = set(plain.state_dict())
    assert "embed_tokens.weight" in mine and not any(k.startswith("adaptive_softmax.") for k in mine)
    assert mine - {"embed_tokens.weight"} == set(got) - set(want)
    assert not plain.is_adaptive and not hasattr(plain, "adaptive_softmax")
    # a state dict with those keys loads strictly, and the tied entries share storage
    _, sd = _small_state()
    full = dict(stack.state_dict())
    full.update(sd)
    stack.load_state_dict(full, strict=True)
    sm, emb = stack.adaptive_softmax, stack.embed_tokens
    assert sm.head.word_proj.weight.data_ptr() == emb.embeddings[0][0].weight.data_ptr()
    for i in range(2):
        assert sm.tail[i][0].weight.data_ptr() == emb.embeddings[i + 1][1].weight.data_ptr()
        assert sm.tail[i][2].weight.data_ptr() == emb.embeddings[i + 1][0].weight.data_ptr()
    assert torch.equal(emb.embeddings[2][0].weight, sd["embed_tokens.embeddings.2.0.weight"])


def test_c1_the_recipe_builder_hands_the_recipes_values_on(monkeypatch):
    from ea_harness import sequence as sq
    seen = {}

    class Probe:
        def __init__(self, *a, **kw):
            seen["a"], seen["kw"] = a, kw
    monkeypatch.setattr(sq, "DecoderStack", Probe)
    sq.wikitext103_decoder(adaptive=True, vocab=267744)
    assert seen["a"][0] == 267744
    assert seen["kw"]["adaptive"] == dict(cutoff=[20000, 60000], factor=4, dropout=0.2, tie_weights=True, tie_proj=True)


def test_c1_q_noise_and_hold_vocab_are_refused():
    from ea_harness import sequence as sq
    from ea_harness.adaptive import AdaptiveInput
    with pytest.raises(NotImplementedError, match="q_noise"):
        AdaptiveInput(333, 1, 128, 2, 128, [96, 200], q_noise=0.1)
    stack = sq.DecoderStack(333, 128, 256, 2, 1, ATTN, adaptive=dict(cutoff=[96, 200], factor=2)).eval()
    with pytest.raises(NotImplementedError, match="adaptive"):
        stack.init_decoding(2, 16, torch.bfloat16, "cpu", hold_vocab=True)
    with pytest.raises(ValueError, match="cutoff"):
        sq.DecoderStack(333, 128, 256, 2, 1, ATTN, adaptive=dict(factor=2))
    with pytest.raises(RuntimeError, match="adaptive="):
        sq.DecoderStack(333, 128, 256, 2, 1, ATTN).adaptive_tables()


# ---- C2 ---------------------------------------------------------------------------------------------------------------------
def test_c2_values_match_the_references_arrays():
    d, sd = _small_state()
    inp, out = _modules(KEYS["small_tied"])
    inp.load_state_dict({k[len("embed_tokens."):]: v for k, v in sd.items() if k.startswith("embed_tokens.")}, strict=True)
    out.load_state_dict({k[len("adaptive_softmax."):]: v for k, v in sd.items() if k.startswith("adaptive_softmax.")},
                        strict=True)
    inp.eval(), out.eval()
    tol = dict(rtol=1e-5, atol=1e-6)
    tokens, targets, x = (torch.from_numpy(d[k]) for k in ("tokens", "targets", "x"))
    cut = inp.cutoff
    assert all(any(int(t) == e for t in tokens.reshape(-1)) for c in cut[:-1] for e in (c - 1, c)) and cut[-1] - 1 in tokens
    with torch.no_grad():
        torch.testing.assert_close(inp(tokens), torch.from_numpy(d["embedded"]), **tol)
        full = out.get_log_prob(x)
        torch.testing.assert_close(full, torch.from_numpy(d["logp_full"]), **tol)
        torch.testing.assert_close(full.exp().sum(-1), torch.ones(2, 24), **tol)
        at = out.get_log_prob(x, targets)
        assert at.shape == targets.shape
        torch.testing.assert_close(at, torch.from_numpy(d["logp_targets"]), **tol)
        torch.testing.assert_close(at, full.gather(-1, targets.unsqueeze(-1)).squeeze(-1), **tol)
        bad = targets.clone()
        bad[0, 0], bad[1, 3] = -1, cut[-1]
        got = out.get_log_prob(x, bad)
        assert torch.isnan(got[0, 0]) and torch.isnan(got[1, 3]) and torch.isnan(got).sum() == 2
    # the fp64 reference agrees too: it is what the GPU tests hold the kernels against
    head = torch.cat([sd["embed_tokens.embeddings.0.0.weight"], sd["adaptive_softmax.head.class_proj.weight"]]).numpy()
    projs = [sd["embed_tokens.embeddings.%d.1.weight" % i].numpy().T for i in (1, 2)]
    tabs = [sd["embed_tokens.embeddings.%d.0.weight" % i].numpy() for i in (1, 2)]
    ref = aref.score(d["x"].reshape(48, 128), head, projs, tabs, cut, d["targets"].reshape(-1))
    np.testing.assert_allclose(ref["logp"], d["logp_targets"].reshape(-1), rtol=1e-5, atol=1e-6)


# ---- C3 ---------------------------------------------------------------------------------------------------------------------
def _route_loop(targets, cutoffs):
    c0, V, n = cutoffs[0], cutoffs[-1], len(cutoffs) - 1
    head, rows = [], [[] for _ in range(n)]
    for m, t in enumerate(targets):
        if not 0 <= t < V:
            head.append(-1)
        elif t < c0:
            head.append(t)
        else:
            i = max(k for k in range(n) if t >= cutoffs[k])
            head.append(c0 + i)
            rows[i].append(m)
    return head, rows


def edge_targets(cutoffs):
    V = cutoffs[-1]
    return [e for c in cutoffs[:-1] for e in (c - 1, c)] + [V - 1, -1, V, 2 ** 40, -2 ** 40, 0]


@pytest.mark.parametrize("cutoffs", [[96, 200, 333], [40, 2140, 2190], [5, 6, 7, 8, 9]])
def test_c3_route_against_a_plain_loop(cutoffs):
    g = np.random.RandomState(3)
    V, n = cutoffs[-1], len(cutoffs) - 1
    cases = {"edges": edge_targets(cutoffs),
             "random": edge_targets(cutoffs) + list(g.randint(-3, V + 3, size=500)),
             "empty band": [t for t in g.randint(0, V, size=300) if not cutoffs[0] <= t < cutoffs[1]],
             "one band": list(g.randint(cutoffs[n - 1], V, size=64))}
    for name, targets in cases.items():
        head, rows, count = aref.route(targets, cutoffs)
        want_head, want_rows = _route_loop([int(t) for t in targets], cutoffs)
        assert head.dtype == np.int64 and head.tolist() == want_head, name
        assert [r.tolist() for r in rows] == want_rows and count.tolist() == [len(r) for r in want_rows], name
        assert all(r.dtype == np.int32 and (np.diff(r) > 0).all() for r in rows), name
    assert aref.route(cases["empty band"], cutoffs)[2][0] == 0
    assert aref.route(cases["one band"], cutoffs)[2].tolist() == [0] * (n - 1) + [64]


# ---- C4 ---------------------------------------------------------------------------------------------------------------------
def test_c4_header_binding_and_version():
    from efficient_attention import _native
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counts = {m.group(1): m.group(2).count(",") + 1
              for m in re.finditer(r"\b(ea_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    for name, n in NEW.items():
        assert name in declared_symbols() and counts[name] == n and len(_native.SIGNATURES[name]) == n, name
        assert hasattr(_native.lib(), name)
    assert _native.lib().ea_abi_version() == _native.ABI_VERSION >= 33
    assert int(re.search(r"#define EA_ADAPTIVE_MAX_TAILS (\d+)", text).group(1)) >= 4
    assert set(_native.SIGNATURES) | {"ea_version", "ea_abi_version"} == set(declared_symbols())
    assert _native.lib().ea_vocab_score_rows_ws.restype is ctypes.c_int64
    assert _native.lib().ea_adaptive_score_ws.restype is ctypes.c_int64


def r16(n):
    return (n + 15) // 16 * 16


def adaptive_ws_layout(M, cutoffs, dims, vs_ws):
    """The documented layout (include/ea_hip.h) -> dict of byte offsets, `total`; vs_ws(M, V) is ea_vocab_score_ws."""
    n, at, lay = len(dims), 0, {}

    def take(name, nbytes):
        nonlocal at
        lay[name] = at
        at += r16(nbytes)
    take("head_target", 8 * M), take("rows", 4 * n * M), take("count", 16)
    take("token_head", 8 * M), take("lse_head", 4 * M), take("logp_head", 4 * M)
    inner = vs_ws(M, cutoffs[0] + n)
    for i, d in enumerate(dims):
        take("h%d" % i, 2 * M * d), take("token%d" % i, 8 * M), take("lse%d" % i, 4 * M), take("logp%d" % i, 4 * M)
        inner = max(inner, vs_ws(M, d), vs_ws(M, cutoffs[i + 1] - cutoffs[i]))
    lay["inner"], lay["total"] = at, at + inner
    return lay


def test_c4_workspace_queries_run_on_the_cpu():
    from efficient_attention import _native as nv
    lib = nv.lib()
    BM, BN, SL = vref.constants()
    for M, V in ((1, 1), (300, 333), (9216, 207744)):
        assert lib.ea_vocab_score_rows_ws(M, V) == lib.ea_vocab_score_ws(M, V) == r16(12 * M * (-(-V // SL)) + 4 * M)
    assert lib.ea_vocab_score_rows_ws(0, 5) < 0 and lib.ea_vocab_score_rows_ws(5, 0) < 0

    def ws(M, cutoffs, dims):
        return lib.ea_adaptive_score_ws(M, len(dims), nv.host_array(ctypes.c_int64, cutoffs), nv.host_array(ctypes.c_int32, dims))
    for M, cutoffs, dims in ((300, [96, 200, 333], [64, 32]), (1, [1, 2], [32]), (9216, [20000, 60000, 267744], [256, 64]),
                             (77, [5, 6, 7, 8, 9], [64, 32, 32, 32])):
        lay = adaptive_ws_layout(M, cutoffs, dims, lib.ea_vocab_score_ws)
        assert ws(M, cutoffs, dims) == lay["total"], (M, cutoffs, dims)
        n = len(dims)
        formula = 16 + r16(4 * n * M) + 2 * r16(8 * M) + 2 * r16(4 * M) \
            + sum(r16(2 * M * d) + r16(8 * M) + 2 * r16(4 * M) for d in dims) + (lay["total"] - lay["inner"])
        assert lay["total"] == formula
    assert ws(0, [96, 200, 333], [64, 32]) < 0                       # M < 1
    assert ws(300, [96, 96, 333], [64, 32]) < 0                      # not increasing
    assert ws(300, [0, 200, 333], [64, 32]) < 0                      # c0 < 1
    assert ws(300, [96, 200, 333], [64, 0]) < 0                      # d_i < 1
    assert ws(300, [96, 200, 2 ** 31], [64, 32]) < 0                 # V >= 2^31
    assert ws(300, [1, 2, 3, 4, 5, 6], [32] * 5) < 0                 # more tails than EA_ADAPTIVE_MAX_TAILS
    assert lib.ea_adaptive_score_ws(300, 0, nv.host_array(ctypes.c_int64, [5]), nv.host_array(ctypes.c_int32, [32])) < 0


def test_c4_argument_errors_are_decided_before_any_launch():
    """NULL operands, bad cutoffs and widths that are no multiple of 32 are refused on the host (no GPU here: a launch would
    fail differently)."""
    from efficient_attention import _native as nv
    lib = nv.lib()
    cut, dims = nv.host_array(ctypes.c_int64, [96, 200, 333]), nv.host_array(ctypes.c_int32, [64, 32])
    null2 = nv.host_array(ctypes.c_void_p, [None, None])
    assert lib.ea_adaptive_route(10, 2, cut, None, None, None, None, None) == -1
    assert lib.ea_adaptive_route(10, 2, None, None, None, None, None, None) == -1
    assert lib.ea_adaptive_score(10, 128, 2, cut, dims, None, 2, 128, None, None, 0, null2, null2, None, 0, None, None, None) == -1
    fake = ctypes.c_void_p(4096)                                      # (aligned, never dereferenced: the call stops before)
    ptrs = nv.host_array(ctypes.c_void_p, [4096, 4096])
    odd = nv.host_array(ctypes.c_int32, [64, 40])
    big = 1 << 40
    assert lib.ea_adaptive_score(10, 128, 2, cut, odd, fake, 2, 128, fake, fake, 0, ptrs, ptrs, fake, big, fake, None, None) == -2
    assert lib.ea_adaptive_score(10, 144, 2, cut, dims, fake, 2, 144, fake, fake, 0, ptrs, ptrs, fake, big, fake, None, None) == -2
    assert lib.ea_adaptive_score(10, 128, 2, cut, dims, fake, 2, 128, fake, fake, 0, ptrs, ptrs, fake, 64, fake, None, None) == -1
    assert lib.ea_vocab_score_rows(10, 32, 16, fake, 2, 32, fake, 0, None, None, 0, 0, fake, big, fake, None, fake, fake, None,
                                   None, -1, 0, None) == -1
    assert lib.ea_vocab_score_rows(10, 32, 16, fake, 2, 32, fake, 0, None, None, 0, 0, fake, big, None, None, None, None, None,
                                   None, 0, 1, None) == -1                # logits_only without logits
    assert lib.ea_vocab_score_rows(10, 48, 16, fake, 2, 48, fake, 0, None, None, 0, 0, fake, big, fake, None, fake, fake, None,
                                   None, 0, 0, None) == -2
