"""fairseq's adaptive-softmax criterion as a training loss: `adaptive_nll(rows, softmax, targets) -> logp`, differentiable in the
rows and in every parameter of the AdaptiveSoftmax, without a [rows, V], [rows, c0 + n] or [rows_i, V_i] tensor in either
direction and without a host read-back.

Forward: ONE ea_adaptive_score call (include/ea_hip.h, ABI 33; ea_adaptive_score_masked with tail masks) -- the scorer of
`DecoderStack.rows_logprobs` on adaptive tables, so logp has its bits.  Its workspace is kept: head_target, the per-tail row
lists and their device counts, lse_head, h_i and lse_i are views into it.
Backward (csrc/ea_adaptive_nll.hip): the head is `vocab_loss.backward_chunks` on the head table with head_target and lse_head;
each tail runs the chunk loop over its device-counted list (ea_vocab_nll_grad_rows), dE_i = G^T h_i and dQ_i = dh_i^T x[rows_i]
on ea_gemm_nt16 against gathered, zero-padded transposes (ea_rows_transpose16), dh_i and dX[rows_i] += dh_i Q_i on
ea_gemm_nt16_rows.  Everything is sized for all M positions per tail; what the backward holds beyond its outputs and the saved
workspace is ea_adaptive_nll_ws bytes.  Launches and framework copies only, so a training step that contains it can be captured
in trainer.capture_step's pattern.  No framework GEMM, softmax or cross-entropy runs; a missing device or library is an error,
never a fall-back."""
import ctypes

import torch

from . import token_pick as tp
from .vocab_loss import _up64, backward_chunks

_SCORE, _MASKED = "ea_adaptive_score", "ea_adaptive_score_masked"
_GRAD, _GEMM, _GEMM_ROWS, _TRANSPOSE = "ea_vocab_nll_grad_rows", "ea_gemm_nt16", "ea_gemm_nt16_rows", "ea_rows_transpose16"


def _r16(n):
    return (n + 15) // 16 * 16


def workspace_plan(M, dims):
    """Byte offsets of the parts of ea_adaptive_score's workspace the backward reads (the layout of include/ea_hip.h):
    dict(head_target, rows, count, lse_head, h=[..], lse=[..], end) -- `end` is where the inner workspace starts."""
    at, plan = 0, dict(h=[], lse=[])

    def take(nbytes):
        nonlocal at
        here, at = at, at + _r16(nbytes)
        return here
    plan["head_target"] = take(8 * M)
    plan["rows"] = take(4 * len(dims) * M)
    plan["count"] = take(16)
    take(8 * M)                                                              # token_head
    plan["lse_head"] = take(4 * M)
    take(4 * M)                                                              # logp_head
    for d in dims:
        plan["h"].append(take(2 * M * d))
        take(8 * M)                                                          # token_i
        plan["lse"].append(take(4 * M))
        take(4 * M)                                                          # logp_i
    plan["end"] = at
    return plan


def _view(ws, at, n, dtype):
    return ws[at:at + n * {torch.int64: 8, torch.float32: 4, torch.int32: 4}[dtype]].view(dtype)


def operand_dtype(rows, softmax):
    """The 16-bit type `adaptive_nll` runs its operands in (what `tail_masks` must have)."""
    return _operand_dtype(rows, [p for p in softmax.parameters()])


def _operand_dtype(rows, params):
    for p in params:
        if p.dtype != torch.float32:
            return p.dtype
    if rows.dtype in (torch.bfloat16, torch.float16):
        return rows.dtype
    return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else torch.bfloat16


class _AdaptiveNll(torch.autograd.Function):
    """apply(rows, targets, meta, head_a, head_b, proj_0, table_0, ..) with meta = (cutoff, tied_proj, chunk_cols, masks);
    head_a is band 0's table [c0, C] and head_b the class rows [n, C], or head_a is `head.weight` [c0 + n, C] and head_b None."""

    @staticmethod
    def forward(ctx, rows, targets, meta, head_a, head_b, *tails):
        from efficient_attention import _native as nv
        cutoff, tied, chunk_cols, masks = meta
        n = len(cutoff) - 1
        params = [head_a] + ([] if head_b is None else [head_b]) + list(tails)
        E = _operand_dtype(rows, params)
        head = (head_a if head_b is None else torch.cat([head_a.detach(), head_b.detach()], 0)).detach().to(E).contiguous()
        proj = [(tails[2 * i].detach().t() if tied else tails[2 * i].detach()).to(E).contiguous() for i in range(n)]
        tabs = [tails[2 * i + 1].detach().to(E).contiguous() for i in range(n)]
        dims = [t.shape[1] for t in tabs]
        x2 = tp.score_operand(head, rows)
        T, B, C = rows.shape
        M, dev = T * B, x2.device
        t1 = tp.checked_targets(targets, T, B, dev)
        if t1 is None:
            raise ValueError("adaptive_nll scores targets: pass an int64 [T, B] tensor")
        nv.require_cuda(x2, "rows")
        if masks is not None:
            if len(masks) != n:
                raise ValueError("tail_masks takes one entry (a tensor or None) per tail: %d, got %d" % (n, len(masks)))
            for i, m in enumerate(masks):
                if m is not None and (m.dtype != E or tuple(m.shape) != (M, dims[i]) or m.device != dev or not m.is_contiguous()):
                    raise ValueError("tail_masks[%d] must be a contiguous %s [%d, %d] tensor on the rows' device"
                                     % (i, str(E).replace("torch.", ""), M, dims[i]))
            if all(m is None for m in masks):
                masks = None
        cut, hd = nv.host_array(ctypes.c_int64, cutoff), nv.host_array(ctypes.c_int32, dims)
        nbytes = nv.lib().ea_adaptive_score_ws(M, n, cut, hd) if max(M, C) < 2 ** 31 else -1
        if nbytes < 0 or nv.lib().ea_adaptive_nll_ws(M, C, n, cut, hd, 0 if chunk_cols is None else int(chunk_cols)) < 0:
            raise ValueError("%d rows against cutoffs %s at widths %s in chunks of %r columns are outside the adaptive loss's "
                             "envelope (chunk_cols: a positive multiple of %d)"
                             % (M, cutoff, dims, chunk_cols, nv.vocab_score_tiles()[2]))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        logp = torch.empty((T, B), dtype=torch.float32, device=dev)
        hp = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in proj])
        ht = nv.host_array(ctypes.c_void_p, [t.data_ptr() for t in tabs])
        args = [M, C, n, cut, hd, nv.ptr(x2), tp.type_code(x2), C, nv.ptr(t1), nv.ptr(head), nv.io_dtype(head), hp, ht]
        if masks is None:
            nv.call(_SCORE, *args, nv.ptr(ws), ws.numel(), nv.ptr(logp), None, nv.stream())
        else:
            hm = nv.host_array(ctypes.c_void_p, [None if m is None else m.data_ptr() for m in masks])
            nv.call(_MASKED, *args, hm, nv.ptr(ws), ws.numel(), nv.ptr(logp), None, nv.stream())
        ctx.save_for_backward(x2, t1, ws, head, *proj, *tabs, *[m for m in (masks or ()) if m is not None])
        ctx.meta = (list(cutoff), dims, tied, chunk_cols, None if masks is None else [m is not None for m in masks])
        ctx.dtypes = (rows.dtype, [None if p is None else p.dtype for p in (head_a, head_b) + tuple(tails)])
        return logp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogp):
        from efficient_attention import _native as nv
        cutoff, dims, tied, chunk_cols, masked = ctx.meta
        n = len(dims)
        saved = ctx.saved_tensors
        x2, t1, ws, head = saved[:4]
        proj, tabs, rest = saved[4:4 + n], saved[4 + n:4 + 2 * n], list(saved[4 + 2 * n:])
        masks = [rest.pop(0) if masked and masked[i] else None for i in range(n)]
        need = ctx.needs_input_grad
        need_dx, need_head, need_tail = need[0], need[3] or need[4], any(need[5:])
        M, C = x2.shape
        dev, E = x2.device, head.dtype
        d = dlogp.detach().to(torch.float32).contiguous().view(M)
        plan = workspace_plan(M, dims)
        head_target = _view(ws, plan["head_target"], M, torch.int64)
        lse_head = _view(ws, plan["lse_head"], M, torch.float32)
        lib, code, st = nv.lib(), nv.io_dtype(head), nv.stream()
        ldm = _up64(M)

        # the head: today's chunk loop; dX starts here (the tails add to it, so it exists whenever they need it)
        dx, dhead = backward_chunks(x2, head, head_target, lse_head, d, chunk_cols, need_dx, need_head)
        grads = [None] * (2 * n)
        for i in range(n if (need_dx or need_tail) else 0):
            di, Vi = dims[i], cutoff[i + 1] - cutoff[i]
            list_i = ctypes.c_void_p(ws.data_ptr() + plan["rows"] + 4 * i * M)
            count_i = ctypes.c_void_p(ws.data_ptr() + plan["count"] + 4 * i)
            h_i = ctypes.c_void_p(ws.data_ptr() + plan["h"][i])
            lse_i = ctypes.c_void_p(ws.data_ptr() + plan["lse"][i])
            need_de, need_dq = need[6 + 2 * i], need[5 + 2 * i]
            cc = lib.ea_vocab_nll_chunk(M, Vi) if chunk_cols is None else int(chunk_cols)
            width = _up64(min(cc, Vi))
            g = torch.empty(M * width, dtype=E, device=dev)
            gt = torch.empty(min(cc, Vi) * ldm, dtype=E, device=dev)
            ht = de = None
            if need_de:                                                      # h_i^T, zeros beyond the count (h_i is uninitialised there)
                ht = torch.empty((di, ldm), dtype=E, device=dev)
                nv.call(_TRANSPOSE, M, di, h_i, code, di, None, count_i, nv.ptr(ht), code, ldm, st)
                de = torch.empty((Vi, di), dtype=torch.float32, device=dev)
            wct = torch.empty(di * width, dtype=E, device=dev)
            dh = torch.zeros((M, di), dtype=torch.float32, device=dev)      # (rows beyond the count are never written: zeros)
            for v0 in range(0, Vi, cc):
                Vc = min(cc, Vi - v0)
                ldg = _up64(Vc)
                nv.call(_GRAD, M, di, Vi, h_i, code, di, nv.ptr(tabs[i]), code, nv.ptr(t1), lse_i, nv.ptr(d), v0, Vc, nv.ptr(g),
                        ldg, nv.ptr(gt), ldm, list_i, count_i, cutoff[i], st)
                wc = wct[:di * ldg].view(di, ldg)
                wc[:, :Vc].copy_(tabs[i][v0:v0 + Vc].t())
                wc[:, Vc:].zero_()
                nv.call(_GEMM_ROWS, M, di, ldg, nv.ptr(g), ldg, nv.ptr(wc), ldg, code, nv.ptr(dh), di, 1 if v0 else 0, None,
                        count_i, st)
                if need_de:
                    nv.call(_GEMM, Vc, di, ldm, nv.ptr(gt), ldm, nv.ptr(ht), ldm, code, nv.ptr(de[v0:]), di, 0, st)
            del g, gt, wct, ht
            if masks[i] is not None:
                dh.mul_(masks[i])                                            # (the Dropout's backward; dead rows stay zeros)
            dh16 = dh.to(E)
            if need_dq:
                xt = torch.empty((C, ldm), dtype=E, device=dev)              # x[rows_i]^T, zeros beyond the count
                nv.call(_TRANSPOSE, M, C, nv.ptr(x2), tp.type_code(x2), C, list_i, count_i, nv.ptr(xt), code, ldm, st)
                dht = torch.empty((di, ldm), dtype=E, device=dev)
                dht[:, :M].copy_(dh16.t())
                dht[:, M:].zero_()
                dq = torch.empty((di, C), dtype=torch.float32, device=dev)
                nv.call(_GEMM, di, C, ldm, nv.ptr(dht), ldm, nv.ptr(xt), ldm, code, nv.ptr(dq), C, 0, st)
                grads[2 * i] = dq.t() if tied else dq
                del xt, dht
            if need_dx:
                qt = proj[i].t().contiguous()                                # Q_i^T [C, d_i]
                nv.call(_GEMM_ROWS, M, C, di, nv.ptr(dh16), di, nv.ptr(qt), di, code, nv.ptr(dx), C, 1, list_i, count_i, st)
            grads[2 * i + 1] = de
        rows_dtype, param_dtypes = ctx.dtypes
        split = param_dtypes[1] is not None
        if dx is not None:
            dx = dx.view(dlogp.shape[0], dlogp.shape[1], C).to(rows_dtype)
        c0 = cutoff[0]
        ga = gb = None
        if dhead is not None:
            ga, gb = (dhead[:c0], dhead[c0:]) if split else (dhead, None)
        out = [ga, gb] + grads
        out = [g.to(param_dtypes[k]) if g is not None and need[3 + k] else None for k, g in enumerate(out)]
        return (dx if need_dx else None, None, None) + tuple(out)


def adaptive_nll(rows, softmax, targets, *, chunk_cols=None, tail_masks=None):
    """rows [T, B, C] (16-bit or fp32), softmax an ea_harness.adaptive.AdaptiveSoftmax (fp32 master parameters -- cast here to
    the autocast dtype, bfloat16 outside autocast, or to the rows' 16-bit type -- or 16-bit ones), targets int64 [T, B] -> logp
    fp32 [T, B], the targets' log-probabilities under the adaptive softmax with the bits of `rows_logprobs(rows,
    adaptive_tables, targets)` (a target outside [0, V): NaN, and no target term in the gradient).  Differentiable in rows and
    in band 0's table, the class rows (or `head.weight`), and each tail's projection and table; the gradients come back in
    their dtypes, a tied projection's (stored [C, d_i]) transposed, and autograd adds the tied input-side gradients by
    itself.  An entry of dlogp that is exactly 0 adds exact zeros everywhere, whatever its row holds.
    chunk_cols: the table columns one backward chunk covers in every pass, a multiple of the scorer's slice width (default:
    ea_vocab_nll_chunk per pass).  Table gradients have the same bits at every chunk width.
    tail_masks: per tail None or 16-bit multipliers [T B, d_i] in the operands' dtype, indexed by the POSITION in the tail's
    row list (the j-th row whose target lies in tail i, in row order): h_i = round(h_i mask), fairseq's Dropout inside
    tail[i]; the backward multiplies dh_i by the same mask.  `softmax.dropout` itself is NOT applied here (see
    DecoderStack.adaptive_loss)."""
    from .adaptive import AdaptiveSoftmax, _TiedHead
    if not isinstance(softmax, AdaptiveSoftmax):
        raise ValueError("softmax must be an ea_harness.adaptive.AdaptiveSoftmax, got %s" % type(softmax).__name__)
    if isinstance(softmax.head, _TiedHead):
        head_a, head_b = softmax.head.word_proj.weight, softmax.head.class_proj.weight
    else:
        head_a, head_b = softmax.head.weight, None
    tails = []
    for i in range(len(softmax.tail)):
        tails += [softmax.tail[i][0].weight, softmax.tail[i][2].weight]
    for p in [head_a] + tails:
        if p.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("the adaptive softmax's parameters must be fp32 masters or 16-bit, got %s" % p.dtype)
    meta = (list(softmax.cutoff), softmax.tie_proj, chunk_cols, None if tail_masks is None else list(tail_masks))
    return _AdaptiveNll.apply(rows, targets, meta, head_a, head_b, *tails)
