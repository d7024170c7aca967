"""-m gpu: CausalSoftmaxAttention under bf16 autocast against an fp64 restatement of fairseq's module (three Linears, the scaled
causal softmax with the padding mask, out_proj) -- output, input gradient and the gradients of all eight parameters within
gpu_checks.MODULE_TOL -- and a 2-layer DecoderStack(attn_name="softmax"): finite loss / evaluate, causal rows, no decoding."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-attention_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import gpu_checks                       # noqa: E402

T, B = 80, 2


def _fp64_module(m, x, pad, h):
    """fairseq's MultiheadAttention forward under the future mask, in fp64, on clones of m's parameters."""
    ps = {n: p.detach().double().requires_grad_(True) for n, p in m.named_parameters()}
    x = x.detach().double().requires_grad_(True)
    C = x.shape[-1]
    d = C // h
    lin = lambda t, n: torch.nn.functional.linear(t, ps[n + ".weight"], ps[n + ".bias"])      # noqa: E731
    rows = [lin(x, n) for n in ("q_proj", "k_proj", "v_proj")]
    rows[1].retain_grad()
    q, k, v = [r.view(T, B, h, d).permute(1, 2, 0, 3) for r in rows]
    logits = d ** -0.5 * q @ k.transpose(-1, -2)
    dead = torch.ones(T, T, dtype=torch.bool, device=x.device).triu(1)[None, None] | pad[:, None, None, :]
    out = torch.softmax(logits.masked_fill(dead, float("-inf")), -1) @ v
    return lin(out.permute(2, 0, 1, 3).reshape(T, B, C), "out_proj"), x, ps, rows[1]


def _close(got, ref, what, scale=None, rms_scale=None):
    mx, rms = gpu_checks.MODULE_TOL
    err = (got.detach().double() - ref).abs()
    scale = ref.abs().max() if scale is None else scale
    rms_scale = ref.pow(2).mean().sqrt() if rms_scale is None else rms_scale
    figures = (float(err.max() / scale), float(err.pow(2).mean().sqrt() / rms_scale))
    print("%-16s max %.2e rms %.2e" % ((what,) + figures))
    assert figures[0] <= mx and figures[1] <= rms, (what, figures)


@pytest.mark.gpu
@pytest.mark.parametrize("C,h", [(128, 2), (256, 2)])
def test_module_matches_fp64_fairseq_restatement(C, h):
    import efficient_attention as ea
    torch.manual_seed(C)
    m = ea.CausalSoftmaxAttention(C, h).cuda()
    x = torch.randn(T, B, C, device="cuda", requires_grad=True)
    pad = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    pad[1, T - 11:] = True                                # right padding on one row
    w = torch.randn(T, B, C, device="cuda")
    w[-11:, 1] = 0                                        # (padded positions carry no loss)
    future = torch.full((T, T), float("-inf"), device="cuda").triu(1)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y, none = m(x, x, x, key_padding_mask=pad, attn_mask=future)
    assert none is None and y.shape == (T, B, C)
    (y.float() * w).sum().backward()
    yr, xr, ps, krows = _fp64_module(m, x, pad, h)
    (yr * w.double()).sum().backward()
    keep = ~pad.t()[:, :, None].expand(T, B, C)
    _close(y.float()[keep], yr.detach()[keep], "out")
    _close(x.grad, xr.grad, "dx")
    for n, p in m.named_parameters():
        if n == "k_proj.bias":
            # softmax is invariant to a shift of every key, so this gradient is exactly 0: the column sum of dk.  What the
            # module returns is the sum of dk's rounding errors, measured against the sum it cancels in, sum_rows |dk|.
            col = krows.grad.abs().sum((0, 1))
            _close(p.grad, ps[n].grad, n, scale=col.max(), rms_scale=col.pow(2).mean().sqrt())
        else:
            _close(p.grad, ps[n].grad, n)
    with pytest.raises(ValueError):
        m(x, x, x, attn_mask=torch.zeros(T, T, device="cuda"))
    with pytest.raises(NotImplementedError, match="incremental"):
        m(x, x, x, incremental_state={})
    with pytest.raises(NotImplementedError, match="fp32"):
        m(x, x, x)


@pytest.mark.gpu
def test_softmax_decoder_stack():
    from ea_harness import sequence as sq
    torch.manual_seed(3)
    stack = sq.DecoderStack(97, 128, 256, 2, 2, None, dropout=0.0, attn_name="softmax").cuda()
    tokens = torch.randint(2, 97, (2, 41), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = stack.loss(tokens)
        loss.backward()
        stack.eval()
        logp = stack.evaluate(tokens)
        rows = stack(tokens)
        other = tokens.clone()
        t = 17
        other[:, t + 1:] = torch.randint(2, 97, (2, 41 - t - 1), device="cuda")
        rows2 = stack(other)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(logp).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in stack.parameters() if p.grad is not None)
    assert bool((rows[:t + 1] == rows2[:t + 1]).all()) and not bool((rows[t + 1:] == rows2[t + 1:]).all())
    with pytest.raises(NotImplementedError, match="softmax decoding is not built"):
        stack.init_decoding(2, 64, torch.bfloat16, "cuda")
