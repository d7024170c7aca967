"""Host reference of full-vocabulary and nucleus sampling (ea_ceva_sdecode_vocab_sample_full, include/ea_hip.h): numpy and
Python integers.  order: the columns in the total order; masses: q^h_v = floor(exp((l_v - max) / T) 2^32) in fp64; word:
U = word 0 >> 8 of the Philox draw (seed, ctr, sid); draw: r = ((2 U + 1) C) >> 25; target: ceil(double(float32(top_p))
double(Z)); nucleus: kept; eps(mass, size) = 2^-19 mass + size: how far the device's mass of `size` columns may lie from the
host's -- it forms x = (l - max) / T and expf(x) in fp32: |x| <= 22.2 for a live weight, so the two roundings of x move
exp(x) by at most 22.2 * 2^-23 of itself, expf adds 2 ulp, and truncating both sides adds 1 per column."""
import math

import numpy as np

from decoder_sample_reference import philox4x32_10, topk


def order(row):
    return topk(row, np.asarray(row).size)


def masses(row, temperature):
    l = np.asarray(row, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.floor(np.exp((l - l.max()) / float(temperature)) * 2.0 ** 32).astype(np.int64)


def word(seed, ctr, sid):
    seed, ctr = int(seed), int(ctr)
    counter = np.array([ctr & 0xFFFFFFFF, ctr >> 32, int(sid) & 0xFFFFFFFF, 0], dtype=np.uint64)
    return int(philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))[0]) >> 8


def draw(U, C):
    return ((2 * int(U) + 1) * int(C)) >> 25


def target(top_p, Z):
    return math.ceil(float(np.float32(top_p)) * float(int(Z)))


def nucleus(q, ordr, top_p):
    if top_p >= 1.0:
        return len(q)
    C = np.cumsum(np.asarray(q, dtype=np.int64)[ordr])
    return int(np.searchsorted(C, target(top_p, C[-1]), side="left")) + 1


def eps(mass, size):
    return 2.0 ** -19 * float(mass) + size
