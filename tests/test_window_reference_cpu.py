"""CPU checks of the same-operand window / landmark reference (tests/window_reference.py) that tests/test_gpu_window_core.py
holds the 16-bit kernels to:
  a. the reference equals the oracle (oracle/attention.py) in fp64 to 1e-12, outputs and gradients;
  b. every case of tests/window_cases.py still gets the plan it was written for (host queries; no GPU needed);
  c. the model-relative bound rejects a reference with ONE deliberate defect, and accepts the unmutated model."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import window_cases as wc               # noqa: E402
import window_reference as wr           # noqa: E402
from oracle import attention as oa      # noqa: E402

F64 = torch.float64


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-300))


def _qkv(B, h, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, h, n, d, dtype=F64, generator=g).requires_grad_(True) for _ in range(3)] + [g]


def _tail_mask(B, n, w):
    m = torch.zeros(B, n, dtype=torch.bool)
    m[B - 1, n - (3 * w) // 2:] = True
    return m


# ------------------------------------------------------------------------------------------------------------------------
# a. reference against oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn_2d,shape,w,e,masked", [(False, (64,), 16, 0, False), (False, (50,), 8, 4, True), (False, (44,), 8, 8, True),
                                                       (True, (8, 8), 4, 0, False), (True, (12, 12), 4, 2, True)])
def test_window_core_equals_local_core(attn_2d, shape, w, e, masked):
    B, h, d = 2, 2, 16
    n = int(math.prod(shape))
    q, k, v, g = _qkv(B, h, n, d, 1 + n + e)
    Wq, Wk = (w * w, (w + 2 * e) ** 2) if attn_2d else (w, w + 2 * e)
    bias = (0.5 * torch.randn(h, Wq, Wk, dtype=F64, generator=g)).requires_grad_(True)
    mask = _tail_mask(B, n, Wq) if masked else None
    gy = torch.randn(B, h, n, d, dtype=F64, generator=g)
    ref = oa.local_core(q, k, v, mask, attn_2d, w, e, bias)
    gr = torch.autograd.grad(ref, [q, k, v, bias], gy)
    out, lse = wr.window_core(q, k, v, bias=bias, mask=mask, attn_2d=attn_2d, seq_shape=shape, w=w, e=e)
    go = torch.autograd.grad(out, [q, k, v, bias], gy)
    assert _rel(out, ref) <= 1e-12
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(go, gr))
    assert lse.shape == (B, h, n) and bool(torch.isfinite(lse).all())


def _mu_fn(d, g, seen=None):
    A, Bm = torch.randn(d, d, dtype=F64, generator=g) / math.sqrt(d), torch.randn(d, d, dtype=F64, generator=g) / math.sqrt(d)

    def mu_fn(mq, mk):
        if seen is not None:
            seen["qmean"], seen["kmean"] = mq, mk
        rk = mk @ A
        return rk, 0.5 * (mq @ Bm + rk)
    return mu_fn


@pytest.mark.parametrize("attn_2d,shape,w,e,L,masked", [(False, (64,), 16, 0, 4, False), (False, (64,), 16, 8, 8, True),
                                                         (True, (8, 8), 4, 0, 4, False), (True, (12, 12), 4, 2, 9, True)])
def test_window_beta_and_chunk_mean_cores_equal_eva_core(attn_2d, shape, w, e, L, masked):
    B, h, d = 2, 2, 16
    n = int(math.prod(shape))
    q, k, v, g = _qkv(B, h, n, d, 7 + n + e)
    Wq, Wk = (w * w, (w + 2 * e) ** 2) if attn_2d else (w, w + 2 * e)
    bias = (0.5 * torch.randn(h, Wq, Wk, dtype=F64, generator=g)).requires_grad_(True)
    mask = _tail_mask(B, n, Wq) if masked else None
    gy = torch.randn(B, h, n, d, dtype=F64, generator=g)
    seen = {}
    r = int(math.sqrt(n // L)) if attn_2d else n // L
    noise = torch.randn(B, h, L, d, dtype=F64, generator=g)
    ref, aux = oa.eva_core(q, k, v, mask, attn_2d, shape, w, e, L, _mu_fn(d, g, seen), noise, bias, return_aux=True)
    gr = torch.autograd.grad(ref, [q, k, v, bias], gy, retain_graph=True)
    # the landmarks as OPERANDS of the window core, still attached to the oracle's graph: the total gradients must agree
    out, _ = wr.window_core(q, k, v, aux["rf_k_bar"], aux["beta"], bias=bias, mask=mask, attn_2d=attn_2d, seq_shape=shape, w=w, e=e)
    go = torch.autograd.grad(out, [q, k, v, bias], gy, retain_graph=True)
    assert _rel(out, ref) <= 1e-12
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(go, gr))
    geo = dict(r=r, e=e, attn_2d=attn_2d, seq_shape=shape)
    beta = wr.beta_core(k, v, aux["omega"], mask, **geo)
    assert _rel(beta, aux["beta"]) <= 1e-12
    gb = torch.randn(B, h, L, d, dtype=F64, generator=g)
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(torch.autograd.grad(beta, [k, v], gb, retain_graph=True),
                                                    torch.autograd.grad(aux["beta"], [k, v], gb, retain_graph=True)))
    qm, km = wr.chunk_mean_core(q, k, mask, **geo)
    assert _rel(qm, seen["qmean"]) <= 1e-12 and _rel(km, seen["kmean"]) <= 1e-12


@pytest.mark.parametrize("w,e,r,causal,masked,drop", [(16, 0, 8, True, False, False), (16, 16, 4, True, True, False),
                                                       (8, 8, 16, False, True, False), (16, 0, 8, True, True, True)])
def test_window_core_equals_causal_eva_core(w, e, r, causal, masked, drop):
    B, h, n, d = 2, 2, 64, 16
    q, k, v, g = _qkv(B, h, n, d, 11 + w + e + r)
    bias = (0.5 * torch.randn(w, w + e, dtype=F64, generator=g)).requires_grad_(True)
    mask = None
    if masked:
        mask = _tail_mask(B, n, w)
        mask[B - 1, :3] = True                                # left padding: queries of chunk 0 that see no landmark either
    L = n // r
    keep = (torch.rand(B, h, n, w + e + L, generator=g) < 0.8).to(F64) if drop else None
    gy = torch.randn(B, h, n, d, dtype=F64, generator=g)
    noise = torch.randn(B, h, L, d, dtype=F64, generator=g)
    seen = {}
    ref, aux = oa.causal_eva_core(q, k, v, mask, w, e, r, _mu_fn(d, g, seen), noise, bias, causal, None, keep, 0.2, return_aux=True)
    gr = torch.autograd.grad(ref, [q, k, v, bias], gy, retain_graph=True)
    out, _ = wr.window_core(q, k, v, aux["rf_k_bar"], aux["beta"], bias=bias.expand(h, w, w + e), mask=mask, w=w, e=e,
                            causal=2 if causal else 1, chunk=r, keep=keep, keep_scale=1.0 / 0.8)
    go = torch.autograd.grad(out, [q, k, v, bias], gy, retain_graph=True)
    assert _rel(out, ref) <= 1e-12
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(go, gr))
    # the chunks of the causal geometry are never extended, whatever e
    beta = wr.beta_core(k, v, aux["omega"], mask, r=r, e=e, causal=1)
    assert _rel(beta, aux["beta"]) <= 1e-12
    gb = torch.randn(B, h, L, d, dtype=F64, generator=g)
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(torch.autograd.grad(beta, [k, v], gb, retain_graph=True),
                                                    torch.autograd.grad(aux["beta"], [k, v], gb, retain_graph=True)))
    qm, km = wr.chunk_mean_core(q, k, mask, r=r, e=e, causal=1)
    assert _rel(qm, seen["qmean"]) <= 1e-12 and _rel(km, seen["kmean"]) <= 1e-12


def test_lse_is_the_natural_log_normaliser():
    B, h, n, d, w = 1, 2, 32, 16, 8
    q, k, v, g = _qkv(B, h, n, d, 3)
    out, lse = wr.window_core(q, k, v, w=w)
    s = d ** -0.5 * torch.einsum("bhid,bhjd->bhij", q[:, :, :w], k[:, :, :w])
    assert _rel(lse[:, :, :w], torch.logsumexp(s, -1)) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------
# b. plan pins
# ------------------------------------------------------------------------------------------------------------------------
_QUERY = dict(parts="ea_window_bwd_parts", qb="ea_window_bwd_query_blocks", slices="ea_window_bwd_acc_slices",
              bias_t="ea_window_bwd_needs_bias_t", bias_parts="ea_window_bwd_bias_parts", bias_ld="ea_window_bias_ld",
              keep_ld="ea_window_keep_ld")


@pytest.mark.parametrize("name", sorted(wc.WINDOW_CASES))
@pytest.mark.parametrize("io", [0, 1])
def test_plan_pins(name, io):
    from efficient_attention import _native as nv
    c = wc.WINDOW_CASES[name]
    geom = nv.make_geom(c["B"], c["h"], c["N"], c["d"], io, c["attn_2d"], c["seq_shape"], c["w"], c["e"], c["chunk"], c["L"], c["causal"])
    got = tuple(int(nv.query(_QUERY[k], geom)) for k in wc.PIN_QUERIES)
    assert got == wc.PINS[name], (name, dict(zip(wc.PIN_QUERIES, got)))


def test_pins_say_what_the_case_table_claims():
    """The plan every case names, read off its pins (ea_window.h: win_bwd_single / _merged / _colour_slices, cdirect, dbd)."""
    P = {n_: dict(zip(wc.PIN_QUERIES, v)) for n_, v in wc.PINS.items()}
    C = wc.WINDOW_CASES
    for n_ in ("W1", "W2", "W5a", "W5b", "W5c", "W6a", "W6b", "W6c", "W7", "W12a", "W12b", "C1", "M1", "M2"):      # single launch
        assert C[n_]["e"] == 0 and P[n_]["slices"] == 0 and P[n_]["qb"] == 1
    assert P["W3"]["slices"] == 0 and C["W3"]["e"] * 2 == C["W3"]["w"] and C["W3"]["N"] % C["W3"]["w"] == 0              # cdirect
    assert P["W4"]["slices"] == 2 and P["W9a"]["slices"] == 3 and P["W9b"]["slices"] == 2 and P["C2"]["slices"] == 2     # colour slices
    assert P["C7"]["slices"] == 2
    assert P["W8"]["slices"] == 1 and P["W8"]["parts"] == 9 and P["W10a"]["slices"] == 1 and P["W11"]["slices"] == 1     # RMW + finish
    assert P["W10a"]["bias_t"] == 1 and P["W10b"]["bias_t"] == 1 and P["W8"]["bias_t"] == 0                               # bias from global
    assert P["C3"]["qb"] == 1 and P["C3"]["slices"] == 0 and P["C3"]["bias_t"] == 1                                       # dbd, one block
    assert P["C4"]["qb"] == 2 and P["C4"]["slices"] == 2 and P["C4"]["bias_parts"] < P["C4"]["parts"]                     # merged
    assert P["C5"]["qb"] == 2 and P["C5"]["slices"] == 1 and C["C5"]["e"] > 0 and P["C6"]["qb"] > 4 and P["C6"]["slices"] == 1   # ordered
    assert P["M1"]["parts"] == 2 and P["M2"]["parts"] == 3 and P["W1"]["parts"] == 2
    assert P["W3"]["keep_ld"] == 48 and P["W7"]["bias_ld"] == 64 and P["W8"]["bias_ld"] == 176 and P["W10a"]["bias_ld"] == 256
    assert C["W10a"]["d"] == 64 and C["W10b"]["d"] == 128


# ------------------------------------------------------------------------------------------------------------------------
# c. sensitivity of the model-relative bound
# ------------------------------------------------------------------------------------------------------------------------
def _drop_last_ext_slot(idx_k, ctx):
    idx_k = idx_k.clone()
    g = idx_k.shape[0] // 2
    j = ctx["e"] - 1 if ctx["causal"] else idx_k.shape[1] - 1          # (the causal extension lies on the left only)
    assert idx_k[g, j] >= 0
    idx_k[g, j] = -1
    return idx_k


def _bias_column_off(bias, ctx):
    return torch.roll(bias, 1, -1)


def _masked_as_absent(dots, ctx):
    # padded TOKENS get -inf instead of -5e4 (slots outside the sequence keep -5e4), in the rows where every local key is blocked
    tok_masked = (oa._gather_mask(ctx["mask"], ctx["idx_k"]) & (ctx["idx_k"] >= 0)[None])[:, None, :, None, :]
    all_blocked = (dots <= oa.MASK_VAL).all(-1, keepdim=True)
    assert bool((all_blocked & tok_masked).any()), "no row with every local key masked: the mutant would be vacuous"
    return dots.masked_fill(all_blocked & tok_masked, float("-inf"))


def _landmarks_one_chunk_late(cv, ctx):
    q_chunk = torch.div(ctx["idx_q"], ctx["chunk"], rounding_mode="floor").unsqueeze(-1)
    L = cv.shape[-1]
    return ctx["cv_raw"].masked_fill((torch.arange(L).view(1, 1, -1) > q_chunk)[None, None], oa.MASK_VAL)


def _local_limit_one_short(dots, ctx):
    i = torch.arange(ctx["Wq"]).view(-1, 1)
    j = torch.arange(ctx["Wk"]).view(1, -1)
    return dots.masked_fill((j - i == ctx["e"])[None, None, None], oa.MASK_VAL)


def _detach_window(pair, g):
    return tuple(torch.cat([t[:, :, :g], t[:, :, g:g + 1].detach(), t[:, :, g + 1:]], 2) for t in pair)


def _skip_window_dkdv(pair, ctx):
    return _detach_window(pair, 1)


def _skip_window_dlkdlv(pair, ctx):
    return _detach_window(pair, 2)


def _no_keep_scale_on_landmarks(keepmul, ctx):
    keepmul = keepmul.clone()
    keepmul[..., ctx["Wk"]:] /= ctx["keep_scale"]
    return keepmul


MUTANTS = {
    "ext_slot_dropped": ("idx_k", _drop_last_ext_slot),
    "bias_column_off": ("bias", _bias_column_off),
    "masked_as_absent": ("local_logits", _masked_as_absent),
    "landmarks_one_chunk_late": ("lm_logits", _landmarks_one_chunk_late),
    "local_limit_one_short": ("local_logits", _local_limit_one_short),
    "window_dkdv_skipped": ("local_kv", _skip_window_dkdv),
    "keep_scale_not_on_landmarks": ("keepmul", _no_keep_scale_on_landmarks),
    "window_dlkdlv_dropped": ("lm_kv", _skip_window_dlkdlv),
}
SENS_CASES = {
    "1d_ext_lm": dict(N=64, w=16, e=8, L=8, mutants=("ext_slot_dropped", "bias_column_off", "window_dkdv_skipped", "window_dlkdlv_dropped")),
    # no landmarks, and batch row 1 pads a corner window with its halo: rows whose every local key is masked
    "2d_ext": dict(grid=(12, 12), w=4, e=2, L=0, mutants=("ext_slot_dropped", "bias_column_off", "masked_as_absent", "window_dkdv_skipped")),
    "causal": dict(N=64, w=16, e=16, causal=2, chunk=8, keep=True,
                   mutants=("ext_slot_dropped", "bias_column_off", "masked_as_absent", "landmarks_one_chunk_late", "local_limit_one_short",
                            "window_dkdv_skipped", "keep_scale_not_on_landmarks", "window_dlkdlv_dropped")),
}
_SENS = {}


def _sens_setup(case, round_to):
    """Operands as in the GPU test, R and the unmutated M of one sensitivity case (computed once)."""
    key = (case, round_to)
    if key in _SENS:
        return _SENS[key]
    c = SENS_CASES[case]
    B, h, d, w, e = 2, 2, 32, c["w"], c["e"]
    grid, causal, chunk = c.get("grid"), c.get("causal", 0), c.get("chunk", 0)
    n = grid[0] * grid[1] if grid else c["N"]
    L = n // chunk if causal else c["L"]
    g = torch.Generator().manual_seed(17)

    def io(t):
        return t.to(round_to).float()
    q, k = io(1.5 * torch.randn(B, h, n, d, generator=g)), io(1.5 * torch.randn(B, h, n, d, generator=g))
    v, dout = io(torch.randn(B, h, n, d, generator=g)), io(torch.randn(B, h, n, d, generator=g))
    lk = io(torch.randn(B, h, L, d, generator=g)) if L else None
    lv = io(torch.randn(B, h, L, d, generator=g)) if L else None
    Wq, Wk = (w * w, (w + 2 * e) ** 2) if grid else (w, w + (e if causal else 2 * e))
    bias = 0.5 * torch.randn(h, Wq, Wk, generator=g)
    mask = torch.zeros(B, n, dtype=torch.bool)
    if grid:
        mask.view(B, *grid)[1, :w + e, :w + e] = True
    else:
        mask[1, n - (3 * w) // 2:] = True
        if causal:
            mask[1, :4] = True
    kw = dict(bias=bias, mask=mask, attn_2d=bool(grid), seq_shape=grid or (n,), w=w, e=e, causal=causal, chunk=chunk)
    if c.get("keep"):
        kw.update(keep=(torch.rand(B, h, n, Wk + L, generator=g) < 0.8).float(), keep_scale=1.25)
    ops = (q, k, v, lk, lv, dout)
    R = wr.window_grads(*ops, dtype=F64, **kw)
    M = wr.window_grads(*ops, dtype=torch.float32, round_to=round_to, **kw)
    _SENS[key] = (ops, kw, R, M)
    return _SENS[key]


def _verdicts(X, M, R, round_to):
    return {n_: wr.bound_report(n_, X[n_], M[n_], R[n_], round_to) for n_ in R}


@pytest.mark.parametrize("round_to", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(SENS_CASES))
def test_unmutated_model_passes_at_ratio_one(case, round_to):
    ops, kw, R, M = _sens_setup(case, round_to)
    for n_, (ok, txt, ratio) in _verdicts(M, M, R, round_to).items():
        assert ok and ratio == 1.0, txt
        # and the model is a rounding-level perturbation of the reference, not a different function
        assert wr.a_err(M[n_], R[n_]) <= (0.05 if round_to == torch.bfloat16 else 0.01), txt


@pytest.mark.parametrize("round_to", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case,mutant", [(c, m) for c in sorted(SENS_CASES) for m in SENS_CASES[c]["mutants"]])
def test_bound_rejects_single_defect(case, mutant, round_to):
    ops, kw, R, M = _sens_setup(case, round_to)
    where, fn = MUTANTS[mutant]
    X = wr.window_grads(*ops, dtype=torch.float32, round_to=round_to, hooks={where: fn}, **kw)
    res = _verdicts(X, M, R, round_to)
    assert not all(ok for ok, _, _ in res.values()), "the bound accepts mutant %s:\n%s" % (mutant, "\n".join(t for _, t, _ in res.values()))
