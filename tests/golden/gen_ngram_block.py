#!/usr/bin/env python3
"""Dump what the REFERENCE's n-gram blocking bans (data only), for tests/test_decoder_constraints_cpu.py:

  tests/golden/ngram_block.npz   for seeded cases (tokens int64 [rows, step + 1], step, n, vocabulary size): the boolean mask
                                 [rows, vocab] of the columns NGramRepeatBlock(n, use_extension=False)._no_repeat_ngram sets
                                 to -inf in a row of zeros.  Vocabularies of 12 .. 40 tokens, so that repeats are common;
                                 n = 1 .. 4; step + 2 - n negative, zero and positive.  Arrays: `meta` int64 [cases, 4] =
                                 (rows, step, n, vocab), `tokens<i>`, `mask<i>`.

Runs only where the reference tree lies at REF (below): imports its fairseq/ngram_repeat_block.py under a throw-away
`fairseq` package object whose __path__ points into that tree, so that no fairseq/__init__.py runs (the CUDA extension the
module tries first is not there: its own host loop is what runs)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/fairseq/fairseq"


def install_shims():
    pkg = types.ModuleType("fairseq")
    pkg.__path__ = [REF]
    sys.modules["fairseq"] = pkg


def cases():
    """(rows, step, n, vocab): every n with step + 2 - n negative (where it can be), zero (where it can be) and positive."""
    out = []
    for n in (1, 2, 3, 4):
        steps = sorted(set(s for s in (n - 3, n - 2, n - 1, n, n + 3, n + 9, 23) if s >= 0))
        for i, step in enumerate(steps):
            for vocab in (12, 19, 40)[i % 2:][:2]:
                out.append((3, step, n, vocab))
    return out


def main():
    install_shims()
    mod = importlib.import_module("fairseq.ngram_repeat_block")
    g = torch.Generator().manual_seed(36)
    arrays, meta = {}, []
    for i, (rows, step, n, vocab) in enumerate(cases()):
        tokens = torch.randint(0, vocab, (rows, step + 1), generator=g)
        if step >= 6:                                        # one row repeats its own start: a suffix seen three times
            tokens[0, -3:] = tokens[0, :3]
            tokens[0, 3:6] = tokens[0, :3]
        block = mod.NGramRepeatBlock(n, use_extension=False)
        lprobs = block._no_repeat_ngram(tokens, torch.zeros(rows, vocab), rows, 1, step)
        arrays["tokens%d" % i] = tokens.numpy()
        arrays["mask%d" % i] = torch.isinf(lprobs).numpy()
        meta.append((rows, step, n, vocab))
    arrays["meta"] = np.array(meta, dtype=np.int64)
    signs = set(int(np.sign(step + 2 - n)) for _, step, n, _ in meta)
    assert signs == {-1, 0, 1}, signs
    np.savez_compressed(os.path.join(HERE, "ngram_block.npz"), **arrays)
    print(len(meta), "cases;", sum(int(arrays["mask%d" % i].sum()) for i in range(len(meta))), "banned columns")


if __name__ == "__main__":
    main()
