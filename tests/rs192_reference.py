"""The weight image of ea_linear_rs192 rebuilt from a [192, 192] weight with torch indexing, shared by
tests/test_linear_rs192_cpu.py (which holds it to the documented map computed in numpy) and tests/test_gpu_linear_rs192.py
(which holds the prepare kernel to it)."""


def rs192_image(w16):
    """w16 [192, 192] (any device) in ea_linear_rs192's register order, flat: the map of include/ea_hip.h, piece
    ((pair * 2 + j) * 6 + ks) * 64 + 16 g + li = w16[32 pair + 8 (li >> 2) + (li & 3) + 4 j, 32 ks + 8 g .. + 7]."""
    import torch
    pair = torch.arange(6, device=w16.device).view(6, 1, 1)
    j = torch.arange(2, device=w16.device).view(1, 2, 1)
    li = torch.arange(16, device=w16.device).view(1, 1, 16)
    rows = 32 * pair + 8 * (li >> 2) + (li & 3) + 4 * j                                   # [pair, j, li]
    pieces = w16.contiguous().view(192, 6, 4, 8)[rows]                                    # [pair, j, li, ks, g, 8]
    return pieces.permute(0, 1, 3, 4, 2, 5).contiguous().view(-1)
