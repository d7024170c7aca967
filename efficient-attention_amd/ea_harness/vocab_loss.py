"""The vocabulary cross-entropy of a plain (tied) [V, C] table as a training loss: `vocab_nll(rows, weight, targets) -> logp`,
differentiable, without a [rows, V] tensor in either direction.

Forward: ONE ea_vocab_score call (include/ea_hip.h, ABI 30) -- the scorer of `DecoderStack.rows_logprobs`, so logp has its bits:
logp[t, b] = logit[targets[t, b]] - lse, the log-sum-exp taken over fp32 sums that were never rounded to 16 bits.
Backward (ABI 38, csrc/ea_vocab_nll.hip): the table is walked in column chunks; per chunk one ea_vocab_nll_grad launch forms the
logit tiles again and writes G = d ((v == target) - exp(logit - lse)) in 16 bits, row-major and transposed, and two
ea_gemm_nt16 launches take dX += G W_c and dW[chunk] = G^T X.  What the backward holds beyond its outputs is
ea_vocab_nll_ws(M, C, V, chunk_cols) bytes, which do not grow with rows x V.  Launches and framework copies only: no host
synchronisation, nothing read back, so a training step that contains it can be captured the way trainer.capture_step does
(gradients that keep their storage, .backward(); the pattern the tests cover -- DESIGN.md 4a has what is not known).  No framework GEMM, softmax or
cross-entropy runs; a missing device or library is an error, never a fall-back."""
import torch

from . import token_pick as tp

_SCORE, _GRAD, _GEMM = "ea_vocab_score", "ea_vocab_nll_grad", "ea_gemm_nt16"


def _up64(n):
    return (n + 63) // 64 * 64


def _table_dtype(rows, weight):
    if weight.dtype != torch.float32:
        return weight.dtype
    if rows.dtype in (torch.bfloat16, torch.float16):
        return rows.dtype
    return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else torch.bfloat16


def backward_chunks(x2, table, targets, lse, d, chunk_cols, need_dx, need_dw):
    """The chunk loop: x2 [M, C] fp32 or the table's type, table [V, C] 16-bit, targets int64 [M], lse and d fp32 [M] ->
    (dX fp32 [M, C] or None, dW fp32 [V, C] or None).  chunk_cols: a multiple of the scorer's slice width, or None: the
    library's default (ea_vocab_nll_chunk)."""
    from efficient_attention import _native as nv
    M, C = x2.shape
    V, dev, E = table.shape[0], x2.device, table.dtype
    lib = nv.lib()
    cc = lib.ea_vocab_nll_chunk(M, V) if chunk_cols is None else int(chunk_cols)
    if max(M, V, C) >= 2 ** 31 or cc < 1 or lib.ea_vocab_nll_ws(M, C, V, cc) < 0:
        raise ValueError("%d rows of %d channels against %d table rows in chunks of %r columns are outside "
                         "ea_vocab_nll_grad's envelope (chunk_cols: a positive multiple of %d)"
                         % (M, C, V, chunk_cols, nv.vocab_score_tiles()[2]))
    ldm, width = _up64(M), _up64(min(cc, V))
    code, st = nv.io_dtype(table), nv.stream()
    g = torch.empty(M * width, dtype=E, device=dev)
    gt = torch.empty(min(cc, V) * ldm, dtype=E, device=dev)
    dx = dw = wct = xt = None
    if need_dx:
        wct = torch.empty(C * width, dtype=E, device=dev)
        dx = torch.empty((M, C), dtype=torch.float32, device=dev)
    if need_dw:
        xt = torch.empty((C, ldm), dtype=E, device=dev)
        xt[:, :M].copy_(x2.t())                                             # (fp32 rows: rounded to nearest even, as the kernel does)
        xt[:, M:].zero_()
        dw = torch.empty((V, C), dtype=torch.float32, device=dev)
    for v0 in range(0, V, cc):
        Vc = min(cc, V - v0)
        ldg = _up64(Vc)
        nv.call(_GRAD, M, C, V, nv.ptr(x2), tp.type_code(x2), C, nv.ptr(table), code, nv.ptr(targets), nv.ptr(lse), nv.ptr(d),
                v0, Vc, nv.ptr(g), ldg, nv.ptr(gt), ldm, st)
        if need_dx:
            wc = wct[:C * ldg].view(C, ldg)
            wc[:, :Vc].copy_(table[v0:v0 + Vc].t())
            wc[:, Vc:].zero_()
            nv.call(_GEMM, M, C, ldg, nv.ptr(g), ldg, nv.ptr(wc), ldg, code, nv.ptr(dx), C, 1 if v0 else 0, st)
        if need_dw:
            nv.call(_GEMM, Vc, C, ldm, nv.ptr(gt), ldm, nv.ptr(xt), ldm, code, nv.ptr(dw[v0:]), C, 0, st)
    return dx, dw


class _VocabNll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, weight, targets, chunk_cols):
        from efficient_attention import _native as nv
        if not isinstance(weight, torch.Tensor) or weight.dim() != 2 or \
                weight.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("weight must be the [V, C] table: the fp32 master or a 16-bit copy")
        table = weight.detach().to(_table_dtype(rows, weight)).contiguous()
        x2 = tp.score_operand(table, rows)
        T, B, C = rows.shape
        V, dev = table.shape[0], x2.device
        t1 = tp.checked_targets(targets, T, B, dev)
        if t1 is None:
            raise ValueError("vocab_nll scores targets: pass an int64 [T, B] tensor")
        nv.require_cuda(x2, "rows")
        nbytes = nv.lib().ea_vocab_score_ws(T * B, V) if max(T * B, V, C) < 2 ** 31 else -1
        if nbytes < 0:
            raise ValueError("%d rows against %d table rows are outside ea_vocab_score's envelope" % (T * B, V))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        token = torch.empty(T * B, dtype=torch.long, device=dev)
        logp = torch.empty((T, B), dtype=torch.float32, device=dev)
        lse = torch.empty(T * B, dtype=torch.float32, device=dev)
        nv.call(_SCORE, T * B, C, V, nv.ptr(x2), tp.type_code(x2), C, nv.ptr(table), nv.io_dtype(table), nv.ptr(t1), None,
                nv.EA_F32, V, nv.ptr(ws), ws.numel(), nv.ptr(token), None, nv.ptr(lse), nv.ptr(logp), nv.stream())
        ctx.save_for_backward(x2, table, t1, lse)
        ctx.chunk_cols = chunk_cols
        ctx.rows_dtype, ctx.weight_dtype = rows.dtype, weight.dtype
        return logp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogp):
        x2, table, t1, lse = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_dx or need_dw):
            return None, None, None, None
        T, B = dlogp.shape
        d = dlogp.detach().to(torch.float32).contiguous().view(T * B)
        dx, dw = backward_chunks(x2, table, t1, lse, d, ctx.chunk_cols, need_dx, need_dw)
        if dx is not None:
            dx = dx.view(T, B, -1).to(ctx.rows_dtype)
        if dw is not None:
            dw = dw.to(ctx.weight_dtype)
        return dx, dw, None, None


def vocab_nll(rows, weight, targets, *, chunk_cols=None):
    """rows [T, B, C] (16-bit or fp32), weight [V, C] (the fp32 master parameter -- cast here to the autocast dtype, bfloat16
    outside autocast, or to the rows' 16-bit type -- or a 16-bit table), targets int64 [T, B] -> logp fp32 [T, B], the targets'
    log-probabilities with `rows_logprobs`' bits (a target outside [0, V): NaN, and no gradient through the target's logit).
    Differentiable in rows and weight: the gradients come back in their dtypes, for the fp32 master the chunk results as
    the kernels stored them.  An entry of dlogp that is exactly 0 (a pad target) adds exact zeros to both gradients, whatever
    its row holds.  chunk_cols: the columns of the table one backward chunk covers, a multiple of the scorer's slice width
    (default: ea_vocab_nll_chunk).  d weight has the same bits at every chunk width; d rows sums the chunks in fp32, in
    table order."""
    return _VocabNll.apply(rows, weight, targets, chunk_cols)
