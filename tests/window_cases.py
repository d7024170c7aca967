"""Case tables of the 16-bit window / landmark core tests (tests/test_window_reference_cpu.py pins the plans on the CPU,
tests/test_gpu_window_core.py runs the kernels).  Every case is tied to the host-selected plan it is there for; PINS holds what
the planner answers for it (ea_window_bwd_* / ea_window_*_ld queries; 256 CUs, which is also the no-device fallback), so that a
planner change cannot silently move a case off its plan."""


def _w(B=2, h=2, N=None, d=64, w=None, e=0, L=0, grid=None, causal=0, chunk=0, bias=False, tail=False, keep=False, dlse=False,
       time_first=False, mult=1, store="single"):
    if grid is not None:
        N = grid[0] * grid[1]
    if causal:
        L = N // chunk
    return dict(B=B, h=h, N=N, d=d, w=w, e=e, L=L, attn_2d=grid is not None, seq_shape=grid if grid is not None else (N,),
                causal=causal, chunk=chunk, bias=bias, tail=tail, keep=keep, dlse=dlse, time_first=time_first, mult=mult, store=store)


WINDOW_CASES = {
    # SGs<1,1,0,4> hand-small, `plain`, ragged last iteration (4 + 1 windows)
    "W1": _w(N=80, w=16, bias=True),
    # same kernel, not plain, incomplete last window
    "W2": _w(N=72, w=16, bias=True, tail=True),
    # SGs<1,2,1,4> + half-window direct accumulation (cdirect)
    "W3": _w(N=80, w=16, e=8, L=16, bias=True, store="cdirect"),
    # colour-class slices (2)
    "W4": _w(N=72, w=16, e=8, L=16, bias=True, tail=True),
    # static SGs<4,4,{0,3,4},1,HO,PW>
    "W5a": _w(N=256, w=64, L=0, bias=True),
    "W5b": _w(N=256, w=64, L=48, bias=True),
    "W5c": _w(N=256, w=64, L=64, bias=True),
    # the same three without PW
    "W6a": _w(N=256, w=64, L=0, bias=True, tail=True),
    "W6b": _w(N=200, w=64, L=48, bias=True),
    "W6c": _w(N=200, w=64, L=64, bias=True, tail=True),
    # the cfg2 geometry, static via 2-D
    "W7": _w(grid=(14, 14), w=7, L=49, bias=True),
    # four colour classes of 4/2/2/1 windows, acc_mode 1 + memset + finish
    "W8": _w(grid=(21, 21), w=7, e=3, L=9, bias=True),
    # three slices / two slices with 2e != w, N not a multiple of w
    "W9a": _w(N=100, w=8, e=8, L=4, d=32),
    "W9b": _w(N=100, w=8, e=2, L=4, d=32),
    # bias table read from global memory (at D = 128 the 256 keys of e = 4 do not fit the backward's LDS image -- REFUSED below;
    # with e = 1 the keys fit and two copies of the [64, 113] table do not)
    "W10a": _w(grid=(16, 16), w=8, e=4, L=4, d=64, bias=True),
    "W10b": _w(grid=(16, 16), w=8, e=1, L=4, d=128, bias=True),
    # SGdyn, D = 128, wpi = 4
    "W11": _w(grid=(16, 16), w=4, e=2, L=16, d=128, bias=True),
    # SGdyn, wpi = 2; wpi = 1 with partial tiles
    "W12a": _w(N=128, w=32, L=8, d=64),
    "W12b": _w(N=130, w=48, L=6, d=32),
    # causal kernel
    "C1": _w(N=128, w=16, causal=2, chunk=8, bias=True),
    # causal + left extension
    "C2": _w(N=128, w=16, e=16, causal=2, chunk=2),
    # direct bias-gradient stores (dbd) in one query block
    "C3": _w(N=256, w=128, causal=2, chunk=8, d=128, bias=True, tail=True),
    # dbd + 2 merged query blocks (acc_mode 2)
    "C4": _w(N=256, w=128, causal=2, chunk=4, d=128, bias=True),
    # ordered query blocks with extension (2 blocks x 2 colour classes).  With e = 128 the planner answers 4 blocks, but the 256
    # keys of a block at D = 128 exceed the 160 KB LDS image and the launch refuses the geometry (REFUSED below): e = 64 is the
    # largest extension of this window that runs
    "C5": _w(N=256, w=128, e=64, causal=2, chunk=8, d=128),
    # 16 ordered blocks (more than 4, so not merged).  N = w = 256 at D = 128 is refused for the same reason; at D = 64 a window
    # needs 512 tokens before it is split at all
    "C6": _w(N=512, w=512, causal=2, chunk=16, d=64),
    # causal geometry, non-causal masks
    "C7": _w(N=256, w=64, e=64, causal=1, chunk=16, d=64),
    # dropout kernels, bias in LDS and from global memory
    "C8a": _w(N=128, w=16, causal=2, chunk=8, bias=True, keep=True),
    "C8b": _w(N=256, w=128, causal=2, chunk=4, d=128, bias=True, keep=True),
    # the LocalAttnLseFn input: a gradient of lse
    "X1a": _w(N=80, w=16, bias=True, dlse=True),
    "X1b": _w(grid=(21, 21), w=7, e=3, L=9, bias=True, dlse=True),
    # the strided output path: time-first qkv
    "X2": _w(N=80, w=16, e=8, L=16, bias=True, store="cdirect", time_first=True),
    # magnitudes of the existing cdirect test: inputs x 4, dout x 8
    "X3a": _w(N=80, w=16, e=8, L=16, bias=True, store="cdirect", mult=4),
    "X3b": _w(N=128, w=16, causal=2, chunk=8, bias=True, mult=4),
    # workgroups of 3 + 2 iterations (5 iterations per (b,h))
    "M1": _w(B=64, h=4, N=320, w=16, L=16, bias=True),
    # 3 workgroups x 3 windows, landmark-gradient accumulators kept across windows
    "M2": _w(B=80, h=4, grid=(21, 21), w=7, L=49, bias=True),
}

# ea_window_bwd_parts, _query_blocks, _acc_slices, _needs_bias_t, _bias_parts, ea_window_bias_ld, ea_window_keep_ld
PIN_QUERIES = ("parts", "qb", "slices", "bias_t", "bias_parts", "bias_ld", "keep_ld")
PINS = {
    "W1": (2, 1, 0, 0, 2, 16, 16),
    "W2": (2, 1, 0, 0, 2, 16, 16),
    "W3": (2, 1, 0, 0, 2, 32, 48),
    "W4": (2, 1, 2, 0, 2, 32, 48),
    "W5a": (4, 1, 0, 0, 4, 64, 64),
    "W5b": (4, 1, 0, 0, 4, 64, 112),
    "W5c": (4, 1, 0, 0, 4, 64, 128),
    "W6a": (4, 1, 0, 0, 4, 64, 64),
    "W6b": (4, 1, 0, 0, 4, 64, 112),
    "W6c": (4, 1, 0, 0, 4, 64, 128),
    "W7": (4, 1, 0, 0, 4, 64, 128),
    "W8": (9, 1, 1, 0, 9, 176, 192),
    "W9a": (4, 1, 3, 0, 4, 32, 48),
    "W9b": (4, 1, 2, 0, 4, 16, 32),
    "W10a": (4, 1, 1, 1, 4, 256, 272),
    "W10b": (4, 1, 1, 1, 4, 112, 128),
    "W11": (8, 1, 1, 0, 8, 64, 80),
    "W12a": (2, 1, 0, 0, 2, 32, 48),
    "W12b": (3, 1, 0, 0, 3, 48, 64),
    "C1": (2, 1, 0, 0, 2, 16, 32),
    "C2": (2, 1, 2, 0, 2, 32, 96),
    "C3": (2, 1, 0, 1, 2, 128, 160),
    "C4": (4, 2, 2, 1, 2, 128, 192),
    "C5": (4, 2, 1, 1, 4, 192, 224),
    "C6": (16, 16, 1, 1, 16, 512, 544),
    "C7": (4, 1, 2, 0, 4, 128, 144),
    "C8a": (2, 1, 0, 0, 2, 16, 32),
    "C8b": (4, 2, 2, 1, 2, 128, 192),
    "X1a": (2, 1, 0, 0, 2, 16, 16),
    "X1b": (9, 1, 1, 0, 9, 176, 192),
    "X2": (2, 1, 0, 0, 2, 32, 48),
    "X3a": (2, 1, 0, 0, 2, 32, 48),
    "X3b": (2, 1, 0, 0, 2, 16, 32),
    "M1": (2, 1, 0, 0, 2, 16, 32),
    "M2": (3, 1, 0, 0, 3, 64, 128),
}

BATCH_INDEPENDENCE = ("W3", "W8", "C4", "M1")

# geometries the planner tiles (its queries answer) but whose backward does not fit one LDS image: ea_window_attn_bwd must
# refuse them with EA_E_UNSUPPORTED before it launches anything
REFUSED = {
    "w128_e128_d128": _w(N=256, w=128, e=128, causal=2, chunk=8, d=128),
    "w256_d128": _w(N=256, w=256, causal=2, chunk=16, d=128),
    "2d_w8_e4_d128": _w(grid=(16, 16), w=8, e=4, L=4, d=128),
}


def _l(grid=None, N=None, r=None, w=None, e=0, d=64):
    attn_2d = grid is not None
    if attn_2d:
        N = grid[0] * grid[1]
    L = (grid[0] // r) * (grid[1] // r) if attn_2d else N // r
    return dict(B=2, h=2, N=N, d=d, attn_2d=attn_2d, seq_shape=grid if attn_2d else (N,), r=r, w=w if w is not None else r, e=e, L=L)


LANDMARK_CASES = {
    "L1": _l(N=64, r=8),                          # register-resident NI = 1
    "L2": _l(grid=(16, 16), r=4),                 # NI = 2
    "L3": _l(grid=(20, 20), r=5, w=5),            # NI = 4
    "L4a": _l(grid=(14, 14), r=7),                # NI = 8
    "L4b": _l(grid=(14, 14), r=7, d=32),          # NI = 4
    "L5": _l(grid=(16, 16), r=4, d=128),          # looping, WPC = 1
    "L6a": _l(N=256, r=64),                       # cooperative, WPC = 4
    "L6b": _l(N=512, r=128),
    "L7": _l(grid=(16, 16), r=4, w=4, e=1),       # 4 colour classes; chunk-mean backward by the gather kernel
    "L8": _l(grid=(14, 14), r=7, w=7, e=3),       # cooperative + colours
}
