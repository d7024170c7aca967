"""Case table of the kernelized-attention core tests (tests/test_kz_reference_cpu.py holds the reference, the model, the plan and
the input conditions on the CPU; tests/test_gpu_kz_core.py runs the kernels of csrc/ea_kernelized.hip): one small case per branch
of the dispatcher and of the kernels.  d = 64 throughout; every case runs in fp32 I/O, the cases in BOTH16 also in bf16 and fp16.

The slice plan (plan_slices, csrc/ea_f32_tile.h) is S = min(ceil(1024 / BH), tiles, 64), tps = ceil(tiles / S) * 64; the feature
block (kz_dispatch, csrc/ea_kernelized.hip) is 32 columns when Fb % 32 == 0 (fourier: and m % 32 == 0), else 16.  Each case
RECORDS the S, tps and fb it must get; the CPU file compares them with `plan` / `feature_block` below and with the library's own
ea_kernelized_parts, so a planner change cannot move a case off its branch silently.

The base geometry is B = 2, h = 2, N = 200 with 37 padded keys at the end of the last batch row: S = 4, one tile per slice, a last
tile of 8 rows.

Operands come from a per-case seeded CPU generator: q, k ~ xs N(0, 1), v, dout ~ N(0, 1), W ~ N(0, 1), drawn in fp32 and then
rounded to the I/O dtype.  `operands` then enforces the input conditions by REDRAWING the offending tokens from the same generator
(no element is ever skipped by a test):
  relu maps   every query and key logit has |l| >= RELU_MARGIN (the branch relu(r l) must be the same in fp32 and fp64)
  all maps    every query has |den - 1e-2| >= DEN_MARGIN (the clamp branch likewise)
  fourier     no query has 1e-2 <= den < DEN_GAP.  Fourier features are signed, so den = phi(q) . ksum is a sum with cancellation
              (sum |terms| is about 1): an unclamped query with den = 0.013 amplifies the fp32 error of its logits 80-fold into
              out and 1 / den^2-fold into dq.  With a handful of such queries in a case the figure a(.) is the error of ONE of
              them, and two equally legitimate fp32 evaluations of the model (another order of additions in the logits) gave
              a(.) figures up to 31 times apart -- no fixed factor can hold a correct kernel to that.  With the gap the two stay
              within a factor 3 (asserted on the CPU for every W-map case and tensor).  Clamped queries (den < 1e-2, as close to
              it as DEN_MARGIN) stay, and the favorp cases keep unclamped queries from den = 0.0101 on: a wrong clamp threshold
              still shows from both sides.
and returns how many tokens it redrew."""
import torch

import kz_contract as kc

RELU_MARGIN = 4e-4          # 64 times the fp32 logit error of the model (up to 3.4e-6 at these scales) with room to spare
DEN_MARGIN = 1e-5
DEN_GAP = 0.1                # fourier: no unclamped query with den below this (see `operands`)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def plan(BH, N):
    """(S, tps): the slice plan of plan_slices."""
    tiles = -(-N // 64)
    S = max(1, min(-(-1024 // BH), tiles, 64))
    return S, -(-tiles // S) * 64


def base_features(mp, m):
    return {"favorp": m, "relu": m, "fourier": 2 * m, "relu-only": 64, "sigmoid-only": 64}.get(mp) or 128 * ((m // 64) // 2)


def feature_block(mp, m):
    """The dispatcher's rule for p.fb."""
    Fb = base_features(mp, m)
    return 32 if (Fb % 32 == 0 and (mp != "fourier" or m % 32 == 0)) else 16


def _c(mp, m, cos, fb, B=2, h=2, N=200, S=4, tps=64, pad="tail37", xs=0.7, need_dw=None, like=None, build=None, gap=0.0):
    has_w = mp in ("favorp", "relu", "fourier")
    gap = DEN_GAP if (mp == "fourier" and not gap) else gap
    return dict(map=mp, m=m, cos=bool(cos), fb=fb, B=B, h=h, N=N, S=S, tps=tps, pad=pad, xs=xs, like=like, build=build, gap=gap,
                need_dw=has_w if need_dw is None else need_dw, F=base_features(mp, m) * (2 if cos else 1))


CASES = {
    # ---- every (map, cos) pair at fb = 32: the 48 instantiations of kv / out / bwd_q / bwd_k
    "favorp_m64": _c("favorp", 64, 0, 32, xs=0.5),
    "favorp_m64_cos": _c("favorp", 64, 1, 32, xs=0.5),
    "relu_m64": _c("relu", 64, 0, 32),
    "relu_m64_cos": _c("relu", 64, 1, 32),
    "fourier_m32": _c("fourier", 32, 0, 32),
    "fourier_m32_cos": _c("fourier", 32, 1, 32),
    "reluonly": _c("relu-only", 0, 0, 32),
    "reluonly_cos": _c("relu-only", 0, 1, 32),
    "sigmoid": _c("sigmoid-only", 0, 0, 32),
    "sigmoid_cos": _c("sigmoid-only", 0, 1, 32),
    "dpfp_nu1": _c("dpfp", 128, 0, 32),
    "dpfp_nu1_cos": _c("dpfp", 128, 1, 32),                 # (also a widest image: F = 256, the cos halves at f0 >= Fb)
    # ---- fb = 16: acc_in_block, acc_feat_times<16>, w = 2, the wave gate; fourier's sin / cos split inside a 32-column span
    "favorp_m16": _c("favorp", 16, 0, 16, xs=0.5),
    "favorp_m48_cos": _c("favorp", 48, 1, 16, xs=0.5),
    "relu_m16": _c("relu", 16, 0, 16),
    "relu_m112_cos": _c("relu", 112, 1, 16),
    "fourier_m16": _c("fourier", 16, 0, 16),
    "fourier_m48_cos": _c("fourier", 48, 1, 16),
    "relu_m80": _c("relu", 80, 0, 16),
    # ---- widest images: all 8 accumulator tiles per wave, a dpfp roll of j = 2
    "favorp_m128_cos": _c("favorp", 128, 1, 32, xs=0.5),
    "fourier_m128": _c("fourier", 128, 0, 32),              # (F = 256 and the largest LDS image, 157 KB)
    "fourier_m64_cos": _c("fourier", 64, 1, 32),
    "dpfp_nu2": _c("dpfp", 256, 0, 32),
    # ---- slices
    # L1: S = 64, tps = 128: 32 two-tile slices (tokens 0 .. 4095), one slice of 34 tokens, 31 empty slices
    "L1_fourier_m32": _c("fourier", 32, 0, 32, B=1, h=2, N=4130, S=64, tps=128, pad=None),
    # L2: S = 4, tps = 128: slices of 128, 128, 44 tokens and an empty fourth; bh / H indexing at BH = 258; masks in several rows
    # (xs = 0.35: den of the live rows stays near 40, so its fp32 error is well below 1e-2 / 64 -- the fully padded row has den = 0)
    "L2_relu_m48_cos": _c("relu", 48, 1, 16, B=43, h=6, N=300, S=4, tps=128, pad="rows", xs=0.35),
    # L3: one full tile; one token
    "L3_favorp_m64_n64": _c("favorp", 64, 0, 32, B=1, h=1, N=64, S=1, tps=64, pad=None, xs=0.5),
    "L3_favorp_m64_n1": _c("favorp", 64, 0, 32, B=1, h=1, N=1, S=1, tps=64, pad=None, xs=0.5),
    # ---- dW: every W-map case above asks for it; this one does not (p_dw NULL), on relu_m64's operands
    "relu_m64_nodw": _c("relu", 64, 0, 32, need_dw=False, like="relu_m64"),
    # ---- masks: B = 3: row 0 padded in the middle of tiles, row 1 fully padded (den = 0: clamped everywhere), row 2 the tail.
    # favorp: one padded key of rows 0 and 2 is scaled by 3, so the key stabiliser sits on a PADDED key (asserted on the CPU)
    "mask_favorp_m64": _c("favorp", 64, 0, 32, B=3, pad="mixed", xs=0.5, S=4, build="padded_max"),
    "mask_dpfp_nu1": _c("dpfp", 128, 0, 32, B=3, pad="mixed", S=4),
    # ---- clamp: queries on both sides of den = 1e-2 (fourier: between 5 % and 95 % clamped; favorp: favorp_m64 above)
    "clamp_fourier_m32": _c("fourier", 32, 0, 32, xs=0.8, pad=None),
    # ---- statistics edge: every key logit negative (W k = -t solved exactly, m < d), N = 70: the 58 zero rows of the ragged tile
    # would win the key maximum
    "stat_favorp_m16_n70": _c("favorp", 16, 0, 16, B=1, h=2, N=70, S=2, tps=64, pad=None, xs=0.5, build="neg_logits"),
}
NAMES = sorted(CASES)
BOTH16 = ("favorp_m64", "fourier_m32", "reluonly", "dpfp_nu1", "favorp_m16", "fourier_m16")
RUNS = [(n_, "fp32") for n_ in NAMES] + [(n_, dt) for n_ in BOTH16 for dt in ("bf16", "fp16")]
CLAMP = {"clamp_fourier_m32": (0.05, 0.95), "favorp_m64": None}
# the Performer's exact-fp32 unit (csrc/ea_performer_f32.hip) blocks the feature dimension differently: the no-cos favorp cases
# with m <= 96 run through it too, on the same R; m = 48 and 80 exist for it alone
PERFORMER_ONLY = {
    "pf_favorp_m48": _c("favorp", 48, 0, 16, xs=0.5),
    "pf_favorp_m80": _c("favorp", 80, 0, 16, xs=0.5),
}
PERFORMER = ("favorp_m16", "favorp_m64", "pf_favorp_m48", "pf_favorp_m80", "mask_favorp_m64", "stat_favorp_m16_n70")


def case(name):
    return CASES[name] if name in CASES else PERFORMER_ONLY[name]


def seed(name):
    return 9000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _mask(c):
    B, N, pad = c["B"], c["N"], c["pad"]
    if pad is None:
        return None
    mask = torch.zeros(B, N, dtype=torch.bool)
    if pad == "tail37":
        mask[-1, N - 37:] = True
    elif pad == "mixed":
        mask[0, 70:96] = True
        mask[0, 130] = True
        mask[0, 191:193] = True
        mask[1, :] = True
        mask[2, N - 37:] = True
    elif pad == "rows":
        mask[0, N - 37:] = True
        mask[7, 100:140] = True
        mask[20, :] = True
        mask[42, 250:] = True
        mask[42, 3] = True
    return mask


def _conditions(c, q, k, v, W, mask):
    """(bad_q [B,N], bad_k [B,N]) tokens that miss an input condition, on the fp64 evaluation of the current operands."""
    F64 = torch.float64
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    Wd = None if W is None else W.to(F64)
    stats = {}
    kc.core(q, k, v, mask, Wd, c["map"], c["m"], c["cos"], stats)
    den = stats["den"]
    bad_q = (((den - 1e-2).abs() < DEN_MARGIN) | ((den >= 1e-2) & (den < c["gap"]))).any(1)
    bad_k = torch.zeros_like(bad_q)
    if c["map"] == "relu":
        cc = 64 ** -0.25
        lq = cc * torch.einsum("bhnd,hjd->bhnj", q, Wd)
        lk = cc * torch.einsum("bhnd,hjd->bhnj", k, Wd)
        bad_q = bad_q | (lq.abs().amin(-1) < RELU_MARGIN).any(1)
        bad_k = (lk.abs().amin(-1) < RELU_MARGIN).any(1)
    return bad_q, bad_k


def operands(name, dt="fp32", same_rows=False):
    """(c, o, redrawn): the case, its CPU operands q, k, v, dout [B,h,N,64] in the I/O dtype, W [h,m,64] fp32 or None, mask [B,N]
    bool or None, and the number of tokens redrawn to meet the input conditions.  same_rows: every batch row gets the data of row
    0 and the mask of the last row."""
    c = case(name)
    io = DTYPES[dt]
    B, h, N = c["B"], c["h"], c["N"]
    g = torch.Generator().manual_seed(seed(c["like"] or name))

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    q, k = (c["xs"] * rn(B, h, N, 64)).to(io), (c["xs"] * rn(B, h, N, 64)).to(io)
    v, dout = rn(B, h, N, 64).to(io), rn(B, h, N, 64).to(io)
    W = rn(h, c["m"], 64) if c["map"] in ("favorp", "relu", "fourier") else None
    mask = _mask(c)
    if c["build"] == "neg_logits":
        t = 0.5 + rn(B, h, N, c["m"]).abs()
        Wd, kd = W.double(), k.double()
        resid = torch.einsum("bhnd,hjd->bhnj", kd, Wd) + t.double()
        k = (kd - torch.einsum("hdj,bhnj->bhnd", torch.linalg.pinv(Wd), resid)).to(io)
    if c["build"] == "padded_max":
        for b, n in ((0, 80), (2, N - 5)):
            assert bool(mask[b, n])
            k[b, :, n] = (3.0 * k[b, :, n].float()).to(io)
    redrawn = 0
    for _ in range(20):
        bad_q, bad_k = _conditions(c, q, k, v, W, mask)
        nq, nk = int(bad_q.sum()), int(bad_k.sum())
        if nq + nk == 0:
            break
        redrawn += nq + nk
        for x, bad, n_ in ((q, bad_q, nq), (k, bad_k, nk)):
            if n_:
                sel = bad[:, None, :].expand(B, h, N)
                x[sel] = (c["xs"] * rn(n_ * h, 64)).to(io)
    else:
        raise AssertionError("%s: the input conditions were not met after 20 rounds of redrawing" % name)
    if same_rows:
        q, k, v, dout = [x[:1].expand(B, h, N, 64).contiguous() for x in (q, k, v, dout)]
        if mask is not None:
            mask = mask[-1:].expand(B, N).contiguous()
    return c, dict(q=q, k=k, v=v, dout=dout, W=W, mask=mask), redrawn
