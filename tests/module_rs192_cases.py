"""The runner of tests/test_gpu_module_rs192.py, shared with the child processes it starts (one per setting of EA_LIN_RS192, which
efficient_attention reads once per process): one LARA and one EVA module step at [2, 14, 14, 192], 3 heads, bf16 autocast,
forward + backward, from fixed seeds.  -> {attn: {"calls": [C-ABI entries in launch order], "y", "dx", "grad.<parameter>"}}."""
import sys
import warnings

ATTN_ARGS = {
    "lara": dict(num_landmarks=49, proposal_gen="pool-mixed", mis_type="mis-opt", alpha_coeff=2.0),
    "eva": dict(window_size=7, attn_2d=True, use_rpe=True, num_landmarks=49, adaptive_proj="default"),
}
B, GRID, C, HEADS = 2, (14, 14), 192, 3


def run(attn):
    import torch
    import efficient_attention as ea
    from efficient_attention import _native as nv
    torch.manual_seed(20 + len(attn))
    args = dict(dim=C, num_heads=HEADS, qkv_bias=True, attn_drop=0.0, proj_drop=0.0, **ATTN_ARGS[attn])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        layer = ea.AttentionFactory.build_attention(attn, args).to("cuda")
    layer.train()
    x = torch.randn(B, *GRID, C, device="cuda", requires_grad=True)
    g = (torch.randn(B, *GRID, C, device="cuda") / (B * GRID[0] * GRID[1])).to(torch.bfloat16)
    calls, plain = [], nv.call

    def recording(name, *a):
        calls.append(name)
        return plain(name, *a)
    nv.call = recording
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = layer(x)
        y.backward(g)
        torch.cuda.synchronize()
    finally:
        nv.call = plain
    res = {"calls": calls, "y": y.detach().cpu(), "dx": x.grad.cpu()}
    for n_, p in layer.named_parameters():
        if p.grad is not None:
            res["grad." + n_] = p.grad.cpu()
    return res


if __name__ == "__main__":        # child process: <package directory> <output file>
    sys.path.insert(0, sys.argv[1])
    import torch
    torch.save({attn: run(attn) for attn in ATTN_ARGS}, sys.argv[2])
