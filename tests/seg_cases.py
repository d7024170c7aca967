"""Case table of the LARA segment-kernel core tests (tests/test_seg_reference_cpu.py checks the reference, the model and the input
conditions on the CPU; tests/test_gpu_seg_core.py runs lara_segment_kernel<E, D, BWD>, pool2d_*_kernel of csrc/ea_lara_segment.hip
and seglin_col_kernel<E, BWD, NCT>, seglin_dg_kernel<E> of csrc/ea_lara_seglin.hip through the C ABI): the smallest shapes that reach
each branch.  Splits are written N / L -> lengths (count short + count long).  Operands are drawn from a per-case seed on the CPU;
every 16-bit operand (rows, gradient base) is rounded to the I/O dtype and handed out as fp32, so R and the kernel see the same
values.  Generator weights G are rounded too (G = G.to(td).float()), except in H7.

Input conditions (properties of R alone, asserted by tests/test_seg_reference_cpu.py): every LayerNorm case has per-row variance
>= 0.05 before the LayerNorm, H8 keeps it in [1e-3, 1e-2]; the prefilled dq / dk / dx base has rms <= the rms of the expected
gradient; max_n t[c,n] < 0.5 in the F cases."""
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _g(D, B, h, N, L, ln=True, bias=True, mask=None, mbias=False, part=True, like=None, what=""):
    return dict(fam="G", D=D, B=B, h=h, N=N, L=L, ln=ln, bias=bias, mask=mask, mbias=mbias, part=part, like=like, what=what)


def _h(B, h, N, L, like=None, raw_G=False, sx=1.0, sgb=0.1, C=0, what=""):
    return dict(fam="F" if C else "H", D=64, B=B, h=h, N=N, L=L, like=like, raw_G=raw_G, sx=sx, sgb=sgb, C=C, scale=64 ** -0.5, what=what)


def _p(gh, gw, side, D, what=""):
    return dict(fam="P", B=2, h=2, gh=gh, gw=gw, N=gh * gw, side=side, D=D, like=None, what=what)


# mask of G1 / G6 (130 / 16: segments 0 .. 13 hold 8 tokens each): batch row 0 masks tokens 20 .. 31 = the second half of segment 2
# and all of segment 3; the last batch row masks 100 .. 103 = half of segment 12
_M1 = ((0, 20, 32), (-1, 100, 104))

CASES = {
    "G1": _g(64, 2, 3, 130, 16, mask=_M1, mbias=True,
             what="130 / 16 -> 8, 9 (14 + 2): LayerNorm, bias, a mask over part of one segment and all of another, mbias; 9 > 8 rows per iteration"),
    "G2": _g(32, 1, 1, 100, 7, ln=False, bias=False,
             what="100 / 7 -> 14, 15 (5 + 2): plain means, no bias, no mask; fewer rows than one 16-row iteration; 14 units = a workgroup with two idle waves"),
    "G3": _g(64, 1, 2, 17, 16, what="17 / 16 -> 1, 2 (15 + 1): one- and two-token segments, LayerNorm"),
    "G4": _g(64, 1, 2, 341, 4, what="341 / 4 -> 85, 86 (3 + 1): 11 iterations, the second row of the last trip invalid"),
    "G5": _g(32, 1, 2, 1000, 16, mask=((0, 490, 530),),
             what="1000 / 16 -> 62, 63 (8 + 8): D 32 with LayerNorm, bias, mask without mbias (NULL)"),
    "G6": _g(64, 2, 3, 130, 16, ln=False, mask=_M1, mbias=True, part=False, like="G1",
             what="G1's geometry, plain means with bias: gq == NULL with a bias; the backward's part is NULL"),
    "H1": _h(1, 2, 130, 16, what="130 / 16 -> 8, 9: one partial step per segment in all three passes"),
    "H2": _h(1, 1, 17, 16, what="17 / 16 -> 1, 2: tiny segments; queue deeper than a segment"),
    "H3": _h(2, 3, 333, 7, what="333 / 7 -> 47, 48 (3 + 4): 2 steps + 15 and exactly 3 full 16-steps; dG: one 32-step + 15 / 16"),
    "H4": _h(8, 8, 150, 49, what="150 / 49 -> 3, 4 (46 + 3): several segments per wave in all three passes, a shorter last group, prefetch "
                                 "across segment boundaries and past the group's end"),
    "H5": _h(1, 1, 1101, 4, what="1101 / 4 -> 275, 276 (3 + 1): 18 column steps with tails 3 / 4; 9 dG steps with tails 19 / 20"),
    "H6": _h(1, 2, 130, 64, what="130 / 64 -> 2, 3 (62 + 2): L = 64"),
    "H7": _h(1, 2, 130, 16, like="H1", raw_G=True, what="H1 with G not representable in the I/O dtype: the staging's rounding of G"),
    "H8": _h(1, 2, 130, 16, sx=0.06, sgb=0.02, what="H1's geometry, per-row variance of G x + g_b in [1e-3, 1e-2]: eps visible"),
    "F1": _h(2, 3, 333, 7, like="H3", C=49, what="_bwd_fin, C = 49: NCT 4, 15 padded landmark rows"),
    "F2": _h(2, 3, 333, 7, like="H3", C=16, what="_bwd_fin, C = 16: NCT 2, 16 of 32 slots padded"),
    "F3": _h(2, 3, 333, 7, like="H3", C=32, what="_bwd_fin, C = 32: NCT 2, no padding, the last C of NCT 2"),
    "F4": _h(2, 3, 333, 7, like="H3", C=33, what="_bwd_fin, C = 33: NCT 4, the first C of NCT 4, 31 padded rows"),
    "F5": _h(2, 3, 333, 7, like="H3", C=64, what="_bwd_fin, C = 64: NCT 4, no padding"),
    "P1": _p(28, 28, 6, 64, what="28 x 28, side 6: bins that share rows / columns"),
    "P2": _p(14, 10, 3, 128, what="14 x 10, side 3, D 128: a non-square grid; two channels per thread"),
    "P3": _p(5, 9, 2, 32, what="5 x 9, side 2, D 32: half of the threads idle"),
    "P4": _p(7, 7, 7, 64, what="7 x 7, side 7: bins of one cell"),
}

NAMES = sorted(CASES)
G_NAMES = [n_ for n_ in NAMES if CASES[n_]["fam"] == "G"]
H_NAMES = [n_ for n_ in NAMES if CASES[n_]["fam"] == "H"]
F_NAMES = [n_ for n_ in NAMES if CASES[n_]["fam"] == "F"]
P_NAMES = [n_ for n_ in NAMES if CASES[n_]["fam"] == "P"]
SAME_B = ("G1", "H3", "H4", "F1")


def seed(name):
    return 9000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def nct(C):
    """Landmark tiles of the fused finish (seglin_dispatch: C <= 32 -> 2, else 4)."""
    return 2 if C <= 32 else 4


def steps(length, rows):
    return (length + rows - 1) // rows


def mask_of(c, B=None):
    if c["fam"] != "G" or not c["mask"]:
        return None
    B = c["B"] if B is None else B
    m = torch.zeros(B, c["N"], dtype=torch.bool)
    for b, lo, hi in c["mask"]:
        m[b % B, lo:hi] = True
    return m


def operands(name, dtype, same_b=False):
    """(c, o): geometry and CPU operands (fp32; bool mask) of a case in I/O dtype `dtype` ('bf16' | 'fp16').  Rows are [B,h,N,D].
    same_b: every batch row gets the data (and the mask) of the first."""
    c = CASES[name]
    td = DTYPES[dtype]
    g = torch.Generator().manual_seed(seed(c["like"] or name))
    B, h, N, D = c["B"], c["h"], c["N"], c["D"]
    n = 1 if same_b else B

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def r16(t):
        return t.to(td).float() + 0.0                    # (+ 0.0: no negative zero, so that `base + 0` keeps its bits)

    def rows(t):
        return t.expand(B, *t.shape[1:]).contiguous() if same_b else t
    o = {}
    if c["fam"] == "P":
        L = c["side"] ** 2
        o["x"], o["d_mean"] = rows(r16(rn(n, h, N, D))), rows(rn(n, h, L, D))
        o["base"] = rows(r16(0.25 * L / N * rn(n, h, N, D)))
        return c, o
    L = c["L"]
    if c["fam"] == "G":
        o["xq"], o["xk"] = rows(r16(rn(n, h, N, D))), rows(r16(rn(n, h, N, D)))
        o["d_qbar"], o["d_kbar"] = rows(rn(n, h, L, D)), rows(rn(n, h, L, D))
        draws = dict(bias_q=0.3 * rn(h, D), bias_k=0.3 * rn(h, D), mbias_q=0.3 * rn(D), mbias_k=0.3 * rn(D),
                     gq=1 + 0.2 * rn(D), cq=0.1 * rn(D), gk=1 + 0.2 * rn(D), ck=0.1 * rn(D))
        keep = dict(bias_q=c["bias"], bias_k=c["bias"], mbias_q=c["mbias"], mbias_k=c["mbias"], gq=c["ln"], cq=c["ln"], gk=c["ln"], ck=c["ln"])
        o.update({n_: (t if keep[n_] else None) for n_, t in draws.items()})
        o["mask"] = mask_of(c, 1).expand(B, N).contiguous() if (same_b and c["mask"]) else mask_of(c)
        return c, o
    sx = c["sx"]
    o["xq"], o["xk"] = rows(r16(sx * rn(n, h, N, 64))), rows(r16(sx * rn(n, h, N, 64)))
    o["d_qbar"], o["d_kbar"] = rows(rn(n, h, L, 64)), rows(rn(n, h, L, 64))
    for sd in ("q", "k"):
        G = 0.125 * rn(64, 64)
        o["G" + sd] = G if c["raw_G"] else r16(G)
        o["gb" + sd], o["lw" + sd], o["lb" + sd] = c["sgb"] * rn(64), 1 + 0.2 * rn(64), 0.1 * rn(64)
    o["base_q"], o["base_k"] = rows(r16(0.25 * L / N * rn(n, h, N, 64))), rows(r16(0.25 * L / N * rn(n, h, N, 64)))
    if c["C"]:
        C = c["C"]
        gf = torch.Generator().manual_seed(seed(name))                 # (the rows are H3's; the finish operands are the case's own)
        o["fin_qbar"] = rows(0.5 * torch.randn(n, h, C, 64, generator=gf))
        o["fin_uq"] = rows(torch.randn(n, h, C, 64, generator=gf))
        # lse_t: the fp64 log-sum-exp over the sequence of s qbar_c . q_n, stored in fp32
        logit = c["scale"] * torch.einsum("bhcd,bhnd->bhcn", o["fin_qbar"].double(), o["xq"].double())
        o["fin_lse"] = torch.logsumexp(logit, -1).float()
    return c, o
