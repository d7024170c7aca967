"""-m gpu: the causal-EVA decoder stack of ea_harness/sequence.py and the fused few-row linear behind the feed-forward of
its held decoding step (csrc/ea_ceva_decode_linear.hip, ea_ceva_sdecode_linear_fused, C ABI 24).

Kernel, with u = 2^-24 (fp32 unit roundoff), u_w the unit roundoff of the weight's type (2^-8 bf16, 2^-11 fp16: round to
nearest, |fl(a) - a| <= u_w |a|) and ulp_y one unit in the last place of y (2^-7 bf16, 2^-10 fp16, 2^-23 fp32, the constant
of tests/test_gpu_ceva_held_decode.py):

 1. no LayerNorm, no activation, no residual: the bits of ea_ceva_sdecode_linear.
 2. the LayerNorm prologue alone (w = the 16-bit identity, fp32 y: the operand as the kernel rounded it) against
    z = (x - mu) r gamma + beta in fp64, mu and var = mean((x - mu)^2) exact, r = (var + eps)^-1/2.  The kernel's fp32
    arithmetic, element k of a row, A = mean |x|, d_k = x_k - mu, n_k = |d_k| r |gamma_k|:
      mean      sum of K terms in any order and one product with fl(1 / K):     |dmu| <= (K + 2) u A
      variance  sum of K squares of fl(x - mu^) and the same product; shifting the mean by dmu adds dmu^2 exactly:
                var^ = var (1 + t),  |t| <= (K + 4) u + dmu^2 / (var + eps)  (relative to var + eps)
      rstd      fl(var^ + eps) (u), rsqrt to 2 ulp (4 u):  r^ = r (1 + rho),  |rho| <= |t| / 2 + u / 2 + 4 u
      operand   fl(x_k - mu^) (u |d_k| + |dmu|), two products (2 u), the sum with beta (u on the products, u |z| on the result;
                fewer roundings where the compiler contracts to fma)
      e32_k = |gamma_k| r |dmu| + n_k (rho + 4 u) + u |z_k|, times 1.01 for the products of these terms among themselves
    and then ONE rounding to the weight's type:  |got - z| <= u_w (|z| + e32) + e32  (+ 2^-25, the fp16 subnormal spacing
    / 2: the all-zero row returns beta, and a beta below 2^-14 is rounded absolutely).  u_w is the half-ulp bound of a
    correct rounding, so the worst ratio sits just below 1 wherever some element lands near a tie: that is the bound being
    sharp, not slack lost.
 3. the whole entry against fp64 relu(x^ w^T + bias) + res on the same operands (x^ from 2, or x rounded without LayerNorm):
      |got - ref| <= ulp_y |ref| + 2 K u (|x^| |w|^T + |bias| + |res|)
    -- the bound of test_gpu_ceva_held_decode._excess with |res| joining |bias|; relu is 1-Lipschitz, so it holds unchanged.
 4. res == y (in place) gives the bits of the out-of-place call.

Stack (embed 128, 2 heads of 64, ffn 256, 2 layers, window 16, chunks of 4, T5 bias, adaptive 'qk'; B = 3; 45 tokens as a
17-token prompt -- 51 rows: the fused feed-forward, while a rolling state's attention cuts it into pieces of a window -- and
steps of 1 and 3): 5. fp32 decode rows = forward rows at F32_TOL; 6. 16-bit held decoding is as close to forward as plain
decoding, within a factor 2 (the same fp32 algebra rounded at other points); 7. the launches of a held step with the
framework's GEMMs banned; 8. generate by capture and replay = generate eagerly, bit for bit; 9. refresh_decoding_weights
reaches a captured step, and without it the step keeps the weights it was made with; 10. the bytes of a held state."""
import functools
import os
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-attention_amd"), os.path.join(ROOT, "tests")]

from ceva_decoding import F32_TOL, STATIC, _Calls, _ctx, _err, _skip_f32            # noqa: E402

LINEAR, FUSED = "ea_ceva_sdecode_linear", "ea_ceva_sdecode_linear_fused"
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
W_DTYPES = [torch.bfloat16, torch.float16]
W_IDS = ["bf16", "fp16"]
EPS = 1e-5
# (M, K, N, strided): one k-step and one live wave; 9 steps over 8 waves, idle waves; exactly one row tile; a second row tile
# holding one row, strided x / res / y; 33 steps: a second pass with one live step; the row bound at fc2's K; the LM shapes
SHAPES = [(1, 32, 16, False), (3, 288, 48, False), (16, 256, 64, False), (17, 256, 64, True), (33, 1056, 32, False),
          (64, 4096, 16, False), (8, 1024, 4096, False), (8, 4096, 1024, False)]
SMALL, LM = SHAPES[:6], SHAPES[6:]
_ids = lambda shapes: ["%dx%dx%d" % s[:3] for s in shapes]                          # noqa: E731


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _code(t):
    from efficient_attention import _native as nv
    return nv.EA_F32 if t.dtype == torch.float32 else nv.io_dtype(t)


def _fused(M, K, N, x, gamma, beta, w, bias, act, res, y):
    """x, res, y: 2-D buffers whose row stride is the leading dimension."""
    from efficient_attention import _native as nv
    nv.call(FUSED, M, K, N, nv.ptr(x), _code(x), x.stride(0), nv.ptr(gamma), nv.ptr(beta), EPS, nv.ptr(w), nv.io_dtype(w),
            nv.ptr(bias), act, nv.ptr(res), 0 if res is None else _code(res), 0 if res is None else res.stride(0),
            nv.ptr(y), _code(y), y.stride(0), nv.stream())
    return y


def _rows(M, K, ld, dtype, values):
    """[M + 1, ld] of NaN with `values` [M, K] in front: what lies beside and below the operand is not read."""
    buf = torch.full((M + 1, ld), float("nan"), dtype=dtype, device="cuda")
    buf[:M, :K] = values
    return buf


@functools.lru_cache(maxsize=None)
def _identity(K, wdtype):
    return torch.eye(K, dtype=wdtype, device="cuda")


def _operands(shape, wdtype, ln_rows=False):
    """x32 [M, K] fp32, xh (rounded to the weight's type), w, bias, gamma, beta, res32 [M, N] -- seeded by the shape."""
    M, K, N, _ = shape
    g = torch.Generator().manual_seed(M * 1000 + K + N)
    if ln_rows:                                      # rows s (3 + 2 randn), s log-uniform over four decades
        s = 10.0 ** (4.0 * torch.rand(M, 1, generator=g) - 2.0)
        x32 = s * (3.0 + 2.0 * torch.randn(M, K, generator=g))
    else:
        x32 = torch.randn(M, K, generator=g)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(wdtype).cuda()
    b = torch.randn(N, generator=g).to(wdtype).cuda()
    gamma = (1.0 + 0.5 * torch.randn(K, generator=g)).cuda()
    beta = torch.randn(K, generator=g).cuda()
    res32 = torch.randn(M, N, generator=g).cuda()
    x32 = x32.cuda()
    return x32, x32.to(wdtype), w, b, gamma, beta, res32


def _ln_operand(xin, gamma, beta, wdtype):
    """The operand rows the kernel forms from xin [M, K] (fp32 or the weight's type): the identity product, fp32 y."""
    M, K = xin.shape
    y = torch.empty((M, K), dtype=torch.float32, device="cuda")
    return _fused(M, K, K, xin.contiguous(), gamma, beta, _identity(K, wdtype), None, 0, None, y)


# ---- 1. bitwise: the plain entry point ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_fused_entry_without_prologue_and_epilogue_is_the_plain_kernel(wdtype, shape):
    from efficient_attention import _native as nv
    M, K, N, strided = shape
    x32, xh, w, b, _, _, _ = _operands(shape, wdtype)
    ldx, ldy = (K + 8, N + 8) if strided else (K, N)
    for xdtype in (torch.float32, wdtype):
        xbuf = _rows(M, K, ldx, xdtype, x32 if xdtype == torch.float32 else xh)
        for ydtype in (wdtype, torch.float32):
            for bias in (b, None):
                want = torch.full((M + 3, ldy), 7.0, dtype=ydtype, device="cuda")
                nv.call(LINEAR, M, K, N, nv.ptr(xbuf), _code(xbuf), ldx, nv.ptr(w), nv.io_dtype(w), nv.ptr(bias), nv.ptr(want),
                        _code(want), ldy, nv.stream())
                got = _fused(M, K, N, xbuf, None, None, w, bias, 0, None, torch.full_like(want, 7.0))
                torch.cuda.synchronize()
                assert torch.isfinite(got[:M, :N]).all() and _bits(got, want), (shape, wdtype, xdtype, ydtype, bias is not None)


# ---- 2. the LayerNorm prologue alone --------------------------------------------------------------------------------------------
def _ln_ref_and_bound(xin, gamma, beta, wdtype):
    """z in fp64 and the element-wise bound of the module docstring, from the operand rows as the kernel reads them."""
    u, K = 2.0 ** -24, xin.shape[1]
    xd, g, b = xin.double(), gamma.double(), beta.double()
    mu = xd.mean(1, keepdim=True)
    d = xd - mu
    var = (d * d).mean(1, keepdim=True)
    r = (var + EPS).rsqrt()
    z = d * r * g + b
    dmu = (K + 2) * u * xd.abs().mean(1, keepdim=True)
    rho = 0.5 * ((K + 4) * u + dmu * dmu / (var + EPS)) + 4.5 * u
    e32 = 1.01 * (g.abs() * r * dmu + d.abs() * r * g.abs() * (rho + 4 * u) + u * z.abs())
    return z, UNIT[wdtype] * (z.abs() + e32) + e32 + (2.0 ** -25 if wdtype == torch.float16 else 0.0)


LN_SHAPES = [s for s in SHAPES if s[1] <= 1056]


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", LN_SHAPES, ids=_ids(LN_SHAPES))
def test_layernorm_prologue_against_fp64(wdtype, shape):
    M, K, _, strided = shape
    x32, _, _, _, gamma, beta, _ = _operands(shape, wdtype, ln_rows=True)
    inputs = [x32]
    if M > 1:
        x32[M - 1] = 0.0                             # the all-zero row: variance 0, the result is beta
    else:
        inputs.append(torch.zeros_like(x32))
    ld = K + 8 if strided else K
    worst = 0.0
    for xv in inputs:
        for xdtype in (torch.float32, wdtype):
            xin = xv.to(xdtype)
            y = torch.full((M + 3, ld), 7.0, dtype=torch.float32, device="cuda")
            _fused(M, K, K, _rows(M, K, ld, xdtype, xin), gamma, beta, _identity(K, wdtype), None, 0, None, y)
            torch.cuda.synchronize()
            assert (y[M:] == 7.0).all() and (y[:, K:] == 7.0).all()
            got = y[:M, :K]
            assert torch.isfinite(got).all() and _bits(got, got.to(wdtype).float())         # values of the weight's type
            z, bound = _ln_ref_and_bound(xin, gamma, beta, wdtype)
            e = ((got.double() - z).abs() / bound).max().item()
            print(shape, wdtype, "x", xdtype, "LayerNorm operand |d| / bound: %.3f" % e)
            worst = max(worst, e)
            zero = xin.abs().sum(1) == 0
            assert zero.any() == (M > 1 or xv is not x32)
            assert _bits(got[zero], beta.to(wdtype).float().expand(M, K)[zero])
    print(shape, wdtype, "worst LayerNorm operand |d| / bound: %.3f" % worst)
    assert worst <= 1.0, (shape, wdtype, worst)


# ---- 3. the whole entry against fp64 --------------------------------------------------------------------------------------------
def _excess(got, xh, w, bias, act, res, ulp_y):
    """max |got - ref| / bound, ref = relu(x^ w^T + bias) + res in fp64 (test_gpu_ceva_held_decode._excess with the
    activation, and |res| joining |bias| in the magnitude)."""
    xd, wd = xh.double(), w.double()
    ref, mag = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if act:
        ref = ref.clamp_min(0.0)
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    bound = ulp_y * ref.abs() + 2.0 * xh.shape[1] * 2.0 ** -24 * mag
    assert torch.isfinite(got).all()
    return ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


def _check_combos(shape, wdtype, combos):
    """combos: (LayerNorm, act, res: None | "w" | "f32").  x and y in {fp32, the weight's type}, with and without bias."""
    M, K, N, strided = shape
    x32, xh, w, b, gamma, beta, res32 = _operands(shape, wdtype)
    ldx, ldy = (K + 8, N + 8) if strided else (K, N)
    worst = 0.0
    for xdtype in (torch.float32, wdtype):
        xin = x32 if xdtype == torch.float32 else xh
        xbuf = _rows(M, K, ldx, xdtype, xin)
        operand = {False: xh, True: _ln_operand(xin, gamma, beta, wdtype)}
        for ln, act, rkind in combos:
            res = None if rkind is None else _rows(M, N, ldy, wdtype if rkind == "w" else torch.float32, res32)
            for ydtype in (wdtype, torch.float32):
                for bias in (b, None) if shape in SMALL else (b,):
                    y = torch.full((M + 3, ldy), 7.0, dtype=ydtype, device="cuda")
                    _fused(M, K, N, xbuf, gamma if ln else None, beta if ln else None, w, bias, act, res, y)
                    torch.cuda.synchronize()
                    assert (y[M:] == 7.0).all() and (y[:, N:] == 7.0).all()
                    e = _excess(y[:M, :N], operand[ln], w, bias, act, None if res is None else res[:M, :N], ULP[ydtype])
                    assert e <= 1.0, (shape, wdtype, xdtype, ydtype, ln, act, rkind, bias is not None, e)
                    worst = max(worst, e)
    print(shape, wdtype, "worst |d| / bound over %d combinations: %.3f" % (len(combos), worst))


EVERY = [(ln, act, res) for ln in (False, True) for act in (0, 1) for res in (None, "w", "f32")]
# what a layer launches: fc1 with the LayerNorm of a pre-norm layer or without (post-norm), ReLU, no residual; fc2 with the
# residual stream (fp32 under autocast, 16-bit in a converted model)
LAYERS_OWN = {1024: [(True, 1, None), (False, 1, None)], 4096: [(False, 0, "f32"), (False, 0, "w")]}


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SMALL, ids=_ids(SMALL))
def test_fused_linear_against_fp64_every_combination(wdtype, shape):
    _check_combos(shape, wdtype, EVERY)


@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", LM, ids=_ids(LM))
def test_fused_linear_against_fp64_lm_shapes(wdtype, shape):
    _check_combos(shape, wdtype, LAYERS_OWN[shape[1]])


# ---- 4. the residual in place -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wdtype", W_DTYPES, ids=W_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_residual_in_place_equals_out_of_place(wdtype, shape):
    M, K, N, strided = shape
    x32, xh, w, b, gamma, beta, res32 = _operands(shape, wdtype)
    ldx, ldy = (K + 8, N + 8) if strided else (K, N)
    for xdtype in (torch.float32, wdtype):
        xbuf = _rows(M, K, ldx, xdtype, x32 if xdtype == torch.float32 else xh)
        for ydtype in (wdtype, torch.float32):
            for ln, act in ((False, 0), (True, 1)):
                res = torch.full((M + 3, ldy), 7.0, dtype=ydtype, device="cuda")
                res[:M, :N] = res32
                gb = (gamma, beta) if ln else (None, None)
                want = _fused(M, K, N, xbuf, *gb, w, b, act, res, torch.full_like(res, 7.0))
                before = res.clone()
                got = _fused(M, K, N, xbuf, *gb, w, b, act, res, res)
                torch.cuda.synchronize()
                assert not _bits(got[:M, :N], before[:M, :N]) and _bits(got, want), (shape, wdtype, xdtype, ydtype, ln)


# ---- the stack ------------------------------------------------------------------------------------------------------------------
ATTN = dict(window_size=16, chunk_size=4, causal=True, adaptive_proj="qk", use_t5_rpe=True, num_chunks=None,
            overlap_window=False)
C, FFN, HEADS, LAYERS, VOCAB, B, T, P0 = 128, 256, 2, 2, 96, 3, 45, 17
STEPS = (P0,) + (1, 3) * 7
NORMS = ["pre_norm", "post_norm"]
KINDS = ["rolling", "static"]


@functools.lru_cache(maxsize=None)
def _stack(norm):
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(5)
    m = DecoderStack(VOCAB, C, FFN, HEADS, LAYERS, ATTN, normalize_before=norm == "pre_norm").cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        for layer in m.layers:
            layer.self_attn.rel_pos_bias.relative_attention_bias.weight.mul_(20.0)
    return m.eval()


@functools.lru_cache(maxsize=None)
def _tokens():
    g = torch.Generator().manual_seed(11)
    return torch.randint(2, VOCAB, (B, T), generator=g).cuda()             # [B, T], no pad token


@functools.lru_cache(maxsize=None)
def _forward(norm, dtype):
    """The full path's rows [T, B, C], computed once per (norm, dtype) and shared."""
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _stack(norm)(_tokens())


def _decode_all(m, kind, dtype, steps=STEPS, calls=None, **opt):
    tokens = _tokens().t()
    st = m.init_decoding(B, T, dtype, "cuda", rolling=kind == "rolling", **opt)
    rows, t = [], 0
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in steps:
            if calls is not None:
                calls.step()
            rows.append(m.decode(tokens[t:t + n], st))
            t += n
    assert t == T
    return torch.cat(rows, 0), st


# ---- 5. fp32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_decode_rows_equal_forward_rows(kind, norm):
    _skip_f32(torch.float32)
    m = _stack(norm)
    full = _forward(norm, torch.float32)
    got, st = _decode_all(m, kind, torch.float32, hold_weights=False)
    assert got.dtype == full.dtype == torch.float32 and got.shape == full.shape
    e = _err(got, full)
    print(kind, norm, "fp32 (max, rms) error vs forward:", e)
    assert e[0] <= F32_TOL[0] and e[1] <= F32_TOL[1], e
    assert m.layers[0].self_attn.decoding_positions(st.incremental).tolist() == [T] * B and not m.decoding_overflowed(st)


# ---- 6. 16-bit: held against plain ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", W_DTYPES, ids=W_IDS)
def test_held_decoding_is_as_close_to_forward_as_plain_decoding(dtype, kind, norm):
    m = _stack(norm)
    full = _forward(norm, dtype)
    plain, _ = _decode_all(m, kind, dtype, hold_weights=False)             # (no new kernel runs in it)
    held, st = _decode_all(m, kind, dtype, hold_weights=True)
    assert held.dtype == plain.dtype == full.dtype and held.shape == full.shape
    d_plain = (plain.double() - full.double()).abs().max().item()
    d_held = (held.double() - full.double()).abs().max().item()
    floor = UNIT[dtype] * full.double().abs().max().item()
    print(kind, norm, dtype, "max |plain - forward| %.4e  max |held - forward| %.4e  u max |forward| %.4e" % (d_plain, d_held, floor))
    assert torch.isfinite(held).all()
    assert d_held <= 2.0 * max(d_plain, floor), (d_held, d_plain, floor)
    assert not m.decoding_overflowed(st)


# ---- 7. launches ------------------------------------------------------------------------------------------------------------------
def _ban(monkeypatch):
    def banned(name):
        def f(*a, **k):
            raise AssertionError("%s reached in a held step of at most 64 rows" % name)
        return f
    for mod, name in ((F, "linear"), (torch, "addmm"), (torch, "matmul")):
        monkeypatch.setattr(mod, name, banned(name))


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_held_step_launches(kind, norm, monkeypatch):
    """A prompt of 23 tokens (69 rows) may use the library GEMM and launches neither linear kernel; steps of 1 and 3 tokens
    (3 and 9 rows) launch, per layer, linear, the attention's four, linear, fused, fused -- eagerly and under capture -- with
    F.linear, torch.addmm and torch.matmul replaced by functions that raise."""
    dtype = torch.bfloat16
    m = _stack(norm)
    tokens = _tokens().t()
    per_layer = [LINEAR] + list(STATIC) + [LINEAR, FUSED, FUSED]
    st = m.init_decoding(B, T, dtype, "cuda", rolling=kind == "rolling")
    pos = m.layers[0].self_attn.decoding_positions_tensor(st.incremental)
    assert pos.is_cuda and pos.dtype == torch.int32 and tuple(pos.shape) == (1,)
    assert pos.data_ptr() == m.layers[0].self_attn._get_input_buffer(st.incremental)["pos"].data_ptr()
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with _Calls() as calls:
            calls.step()
            m.decode(tokens[:23], st)
            assert LINEAR not in calls.steps[-1] and FUSED not in calls.steps[-1]
            with monkeypatch.context() as mp:
                _ban(mp)
                for a, n in ((23, 1), (24, 3), (27, 1)):
                    calls.step()
                    m.decode(tokens[a:a + n], st)
                xin = tokens[28:29].clone()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                calls.step()
                with torch.cuda.stream(s):
                    m.decode(xin, st)
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                calls.step()
                with torch.cuda.graph(g):
                    m.decode(xin, st)
            assert calls.steps[1:] == [per_layer * LAYERS] * 5, calls.steps[1:]
        g.replay()
        torch.cuda.synchronize()
    assert pos.tolist() == [30]                                          # 23 + 1 + 3 + 1, the warm-up, one replay


# ---- 8. capture and replay --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lively_stack():
    """The pre-norm stack with its embedding rows scaled by 1 / 32.  With rows of the initial size a token's own embedding
    outweighs everything else in the tied logits (sqrt(C) |e|^2 against terms of order |e|), so greedy decoding repeats one
    token for ever and would not notice a step that is fed a stale token; with small rows the positions and the layers
    decide, and the tokens move."""
    from ea_harness.sequence import DecoderStack
    torch.manual_seed(7)
    m = DecoderStack(VOCAB, C, FFN, HEADS, LAYERS, ATTN).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))
        for layer in m.layers:
            layer.self_attn.rel_pos_bias.relative_attention_bias.weight.mul_(20.0)
        m.embed_tokens.weight.mul_(1.0 / 32)
    return m.eval()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rolling", "static", "per_sequence_ragged"])
def test_generate_by_replay_equals_generate_eagerly(case):
    dtype = torch.bfloat16
    m = _lively_stack()
    prompt = _tokens()[:, :P0].clone()
    opt = dict(rolling=case != "static")
    lengths = [P0] * B
    if case == "per_sequence_ragged":
        opt["per_sequence"] = True
        lengths = [17, 9, 1]
        for b, n in enumerate(lengths):
            prompt[b, n:] = m.pad_idx
    n_new = T - P0
    out = {}
    with _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for graph in (False, True):
            st = m.init_decoding(B, T, dtype, "cuda", **opt)
            out[graph] = m.generate(prompt, n_new, st, graph=graph, return_rows=True) + (st,)
        (tok_e, rows_e, st_e), (tok_g, rows_g, st_g) = out[False], out[True]
        assert tuple(tok_g.shape) == (B, n_new) and tok_g.dtype == torch.long and tuple(rows_g.shape) == (n_new, B, C)
        assert torch.equal(tok_g, tok_e) and _bits(rows_g, rows_e)
        print(case, "tokens", tok_g.tolist())
        assert (tok_g[:, 1:] != tok_g[:, :-1]).any()                      # (a stale input token would show)
        attn = m.layers[0].self_attn
        want = [n + n_new - 1 for n in lengths]
        assert attn.decoding_positions(st_g.incremental).tolist() == attn.decoding_positions(st_e.incremental).tolist() == want
        if case != "per_sequence_ragged":
            # ... and both are greedy decoding: the same loop written out with decode, logits and argmax, on a fresh state
            with torch.no_grad():
                st = m.init_decoding(B, T, dtype, "cuda", **opt)
                y = m.decode(prompt.t(), st)[-1:]
                for i in range(n_new):
                    tok = m.logits(y).argmax(-1)
                    assert torch.equal(tok[0], tok_g[:, i]) and _bits(y[0], rows_g[i]), i
                    if i + 1 < n_new:
                        y = m.decode(tok, st)


@pytest.mark.gpu
def test_a_ragged_prompt_gives_every_row_its_own_positions():
    """Per-sequence state, right-padded prompt of lengths 17, 9, 1: each row's decoded rows -- the prompt's and those of two
    further single tokens -- equal forward on that row alone (the project's 16-bit bound: 2e-2 of the largest value)."""
    dtype = torch.bfloat16
    m = _stack("pre_norm")
    tokens, lengths = _tokens(), [17, 9, 1]
    prompt = tokens[:, :P0].clone()
    for b, n in enumerate(lengths):
        prompt[b, n:] = m.pad_idx
    nxt = tokens[:, P0:P0 + 2]                                            # two more tokens for every row
    with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = m.init_decoding(B, T, dtype, "cuda", per_sequence=True)
        x = m.decode(prompt.t(), st, prompt.eq(m.pad_idx))
        more = torch.cat([m.decode(nxt[:, i:i + 1].t(), st) for i in range(2)], 0)
        for b, n in enumerate(lengths):
            seq = torch.cat([prompt[b, :n], nxt[b]]).unsqueeze(0)
            full = m(seq)[:, 0]                                           # [n + 2, C]
            got = torch.cat([x[:n, b], more[:, b]], 0)
            d = (got.float() - full.float()).abs().max().item()
            print("row", b, "length", n, "max |d| %.3e, bound %.3e" % (d, 2e-2 * full.float().abs().max().item()))
            assert d <= 2e-2 * full.float().abs().max().item()
    assert m.layers[0].self_attn.decoding_positions(st.incremental).tolist() == [n + 2 for n in lengths]


# ---- 9. the weights are the state's -------------------------------------------------------------------------------------------------
def _replayed(m, dtype, change=None, refresh=False, how="replay"):
    """The prompt eagerly, then single tokens P0 .. T - 1 through one captured step (a warm-up token first) or eagerly; ahead
    of token `change` one fc1 and one q_proj weight are scaled in place (and restored at the end) -> rows [T - P0, B, C]."""
    tokens = _tokens().t()
    fc1, q = m.layers[0].fc1.weight, m.layers[1].self_attn.q_proj.weight
    saved = (fc1.detach().clone(), q.detach().clone())
    st = m.init_decoding(B, T, dtype, "cuda")
    rows = []
    try:
        with torch.no_grad(), _ctx(dtype), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.decode(tokens[:P0], st)
            xin = tokens[P0:P0 + 1].clone()
            g = None
            if how == "replay":
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    rows.append(m.decode(xin, st).clone())
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    yout = m.decode(xin, st)
            else:
                rows.append(m.decode(xin, st).clone())
            ptrs = [t.data_ptr() for held in st.ffn for t in held]
            for t in range(P0 + 1, T):
                if t == change:
                    fc1.mul_(1.5)
                    q.mul_(1.5)
                    if refresh:
                        assert m.refresh_decoding_weights(st) is st
                xin.copy_(tokens[t:t + 1])
                if g is None:
                    rows.append(m.decode(xin, st).clone())
                else:
                    g.replay()
                    rows.append(yout.clone())
            torch.cuda.synchronize()
            assert ptrs == [t.data_ptr() for held in st.ffn for t in held]
            if refresh:
                assert torch.equal(st.ffn[0][0], fc1.detach().to(dtype))
    finally:
        with torch.no_grad():
            fc1.copy_(saved[0])
            q.copy_(saved[1])
    return torch.cat(rows, 0)


@pytest.mark.gpu
def test_refresh_decoding_weights_reaches_a_captured_step():
    dtype = torch.bfloat16
    m = _stack("pre_norm")
    change = 30
    old = _replayed(m, dtype)
    kept = _replayed(m, dtype, change=change)                            # no refresh: the step keeps the old weights
    new = _replayed(m, dtype, change=change, refresh=True)
    eager = _replayed(m, dtype, change=change, refresh=True, how="eager")
    assert _bits(kept, old)
    k = change - P0
    assert _bits(new[:k], old[:k]) and not _bits(new[k:k + 1], old[k:k + 1])
    assert _bits(new, eager)


# ---- 10. bytes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("opt", [{}, dict(per_sequence=True, landmark_splits=3, compact_landmarks=True)], ids=["plain", "options"])
def test_a_held_state_is_the_plain_state_plus_the_held_weights(kind, opt):
    m = _stack("pre_norm")
    dtype = torch.float16
    plain = m.init_decoding(B, 500, dtype, "cuda", rolling=kind == "rolling", hold_weights=False, **opt)
    held = m.init_decoding(B, 500, dtype, "cuda", rolling=kind == "rolling", hold_weights=True, **opt)
    assert plain.ffn is None and not plain.hold_weights and held.hold_weights and len(held.ffn) == LAYERS
    attention = 2 * (3 * C * C + 3 * C + C * C + C) + 2 * 64 * 3 * C       # hold_projections: the weights and the staging rows
    ffn = 2 * (C * FFN + FFN + FFN * C + C)
    assert m.decoding_state_nbytes(held) - m.decoding_state_nbytes(plain) == LAYERS * (attention + ffn)
    for layer, (w1, b1, w2, b2) in zip(m.layers, held.ffn):
        for t, p in ((w1, layer.fc1.weight), (b1, layer.fc1.bias), (w2, layer.fc2.weight), (b2, layer.fc2.bias)):
            assert t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 16 == 0 and not t.requires_grad
            assert torch.equal(t, p.detach().to(dtype))
    # a beam reorder and a row reset forward to every layer and leave the held weights alone
    kept = [t.clone() for layer in held.ffn for t in layer]
    m.reorder_decoding_state(held, torch.tensor([2, 0, 0], device="cuda"))
    if opt:
        m.reset_decoding_rows(held, [1])
    else:
        with pytest.raises(RuntimeError, match="per-sequence"):
            m.reset_decoding_rows(held, [1])
    assert all(torch.equal(a, b) for a, b in zip(kept, [t for layer in held.ffn for t in layer]))
