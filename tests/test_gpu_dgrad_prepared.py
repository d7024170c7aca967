"""The qkv input-gradient kernels fed by the PREPARED W^T image (ea_linear_w192_prepare_t, ABI 25): the image holds the bits of
w16q in the lane order of the kernels' registers, and ea_linear_dgrad / ea_linear_dgrad_finish on it are BIT-identical to the
same kernels staging the 16-bit weight through LDS (same MFMA operands, same order of accumulation)."""
import pytest


def _td(dtype):
    import torch
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def _weights(td, seed):
    import torch
    from efficient_attention import _ops
    g = torch.Generator(device="cuda").manual_seed(seed)
    wq = torch.randn(576, 192, device="cuda", generator=g) * 0.05
    wp = torch.randn(192, 192, device="cuda", generator=g) * 0.05
    return wq, wp, _ops.prepare_w192_t(wq, wp, td)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_prepared_wt_image_is_w16q_in_lane_order(dtype):
    """piece (wave, ks, lane = 16 g + li) = w16q[32 ks + 8 g .. + 7, 16 wave + li], compared on the host; the other four images
    are what ea_linear_w192_prepare writes."""
    import torch
    from efficient_attention import _ops
    td = _td(dtype)
    wq, wp, (w16q, wsw, w16p, w16pT, wt) = _weights(td, 3)
    four = _ops.prepare_w192(wq, wp, td)
    assert len(four) == 4
    for a, b in zip(four, (w16q, wsw, w16p, w16pT)):
        assert torch.equal(a, b)
    assert torch.equal(w16q, wq.to(td))
    assert wt.dtype == td and wt.numel() == 576 * 192
    img = wt.view(torch.int16).cpu().view(12, 18, 4, 16, 8)              # [wave, ks, g, li, j]
    w = w16q.view(torch.int16).cpu()                                     # [576, 192]
    assert torch.equal(torch.sort(img.flatten())[0], torch.sort(w.flatten())[0])
    # w[32 ks + 8 g + j, 16 wave + li] as [ks, g, j, wave, li] -> [wave, ks, g, li, j]
    want = w.view(18, 4, 8, 12, 16).permute(3, 0, 1, 4, 2).contiguous()
    assert torch.equal(img, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("rows,wide,dx_f32", [(1, 0, 1), (33, 1, 1), (1000, 1, 0)])
def test_linear_dgrad_from_prepared_image_is_bit_identical(rows, wide, dx_f32, dtype):
    """one row, one partial tile, 1000 rows of a strided 640-wide buffer"""
    import torch
    from efficient_attention import _ops, _native as nv
    td = _td(dtype)
    wq, _, (w16q, _, _, _, wt) = _weights(td, 5)
    g = torch.Generator(device="cuda").manual_seed(rows)
    buf = (0.5 * torch.randn(rows, 576 + (64 if wide else 0), device="cuda", generator=g)).to(td)
    dy = buf[:, :576]
    xd = torch.float32 if dx_f32 else td
    old = _ops.DGRAD_RS_MIN_ROWS
    _ops.DGRAD_RS_MIN_ROWS = 1
    try:
        kinds = []
        real = nv.call_as
        nv.call_as = lambda label, name, *a: (kinds.append((name, a[7])), real(label, name, *a))[1]
        try:
            dx0 = _ops.qkv_dgrad(dy, wq, w16q, xd)
            dx1 = _ops.qkv_dgrad(dy, wq, w16q, xd, wt)
        finally:
            nv.call_as = real
    finally:
        _ops.DGRAD_RS_MIN_ROWS = old
    assert kinds == [("ea_linear_dgrad", 0), ("ea_linear_dgrad", 2)], kinds
    assert dx1.dtype == xd and tuple(dx1.shape) == (rows, 192)
    assert torch.equal(dx0, dx1), float((dx0.float() - dx1.float()).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W,r,C,has_t", [(3, 28, 28, 4, 49, 1),
                                             (6, 14, 14, 2, 49, 1),          # half-filled tiles, duplicate slots
                                             (9, 14, 14, 2, 49, 0)])
def test_linear_dgrad_finish_from_prepared_image_is_bit_identical(B, H, W, r, C, has_t, dtype):
    """dx and the rewritten dq / dk rows"""
    import torch
    from efficient_attention import _ops
    td = _td(dtype)
    wq, _, (w16q, _, _, _, wt) = _weights(td, 7)
    g = torch.Generator(device="cuda").manual_seed(B * 31 + H + C)
    N, h, d = H * W, 3, 64
    L = (H // r) * (W // r)
    rn = lambda *shape, s=1.0: s * torch.randn(*shape, device="cuda", generator=g)   # noqa: E731
    qkv = rn(B, N, 3, h, d, s=0.5).to(td)
    dqkv = rn(B, N, 3, h, d, s=0.5).to(td)
    scale = d ** -0.5
    qbar = rn(B * h, C, d)
    uq = rn(B * h, C, d) if has_t else None
    q = qkv[:, :, 0].permute(0, 2, 1, 3).float()
    lse_t = torch.logsumexp(scale * torch.einsum("bhnd,bhcd->bhcn", q, qbar.view(B, h, C, d)), -1).reshape(B * h, C).contiguous()
    dpq, dpk = rn(B * h, L, d), rn(B * h, L, d)
    fin = dict(B=B, gh=H, gw=W, r=r, C=C, scale=scale, qbar=qbar if has_t else None, uq=uq, lse_t=lse_t if has_t else None,
               dpq=dpq, dpk=dpk)
    out = []
    for xd in (torch.float32, td):
        for image in (None, wt):
            dq = dqkv.clone()
            dx = _ops.qkv_dgrad_finish(dq.view(-1, 576), qkv.view(-1, 576), wq, w16q, xd, fin, image)
            out.append((dx, dq))
        (dx0, dq0), (dx1, dq1) = out[-2:]
        assert not torch.equal(dq0, dqkv)                                 # the rows were corrected
        assert torch.equal(dq0, dq1), float((dq0.float() - dq1.float()).abs().max())
        assert dx1.dtype == xd and torch.equal(dx0, dx1), float((dx0.float() - dx1.float()).abs().max())
