#!/usr/bin/env python3
"""Dump what the REFERENCE's adaptive input and adaptive softmax are and compute (data only), for tests/test_adaptive_cpu.py
and tests/test_gpu_adaptive_score.py:

  tests/golden/adaptive_keys.json   state_dict key -> shape of both modules, for the wikitext-103 recipe's geometry (C = 1024,
                                    cutoffs 20000, 60000, factor 4, V = 267744, weights and projections tied; built on the
                                    meta device: shapes only) and for the small geometry tied, with the projections untied,
                                    and with nothing tied.
  tests/golden/adaptive_small.npz   the small geometry (C = 128, factor 2: widths 128 / 64 / 32, cutoffs 96, 200, V = 333,
                                    tied): the input module's seeded state dict and the softmax's own entries (the tied ones
                                    are the input's: tail.i.0 = embeddings.{i+1}.1, tail.i.2 = embeddings.{i+1}.0,
                                    head.word_proj = embeddings.0.0), every value rounded to bfloat16 so that a 16-bit copy
                                    is exact; tokens [2, 24] that hit every band and both sides of every cutoff;
                                    AdaptiveInput(tokens); hidden rows x [2, 24, 128]; targets [2, 24];
                                    get_log_prob(x, None) and get_log_prob(x, targets) gathered at the targets.

Runs only in the build container: imports /root/reference/fairseq/fairseq/modules/{adaptive_input,adaptive_softmax}.py under
throw-away `fairseq` / `fairseq.modules` package objects whose __path__ points into the reference tree, so that no
fairseq/__init__.py runs."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/fairseq/fairseq"

RECIPE = dict(C=1024, factor=4, cutoff=[20000, 60000], V=267744, pad=1)
SMALL = dict(C=128, factor=2, cutoff=[96, 200], V=333, pad=1)


def install_shims():
    pkg = types.ModuleType("fairseq")
    pkg.__path__ = [REF]
    mods = types.ModuleType("fairseq.modules")
    mods.__path__ = [os.path.join(REF, "modules")]
    pkg.modules = mods
    sys.modules["fairseq"], sys.modules["fairseq.modules"] = pkg, mods


def build(ai, asm, g, tie_weights=True, tie_proj=True, dropout=0.0):
    inp = ai.AdaptiveInput(g["V"], g["pad"], g["C"], g["factor"], g["C"], list(g["cutoff"]))
    out = asm.AdaptiveSoftmax(g["V"], g["C"], list(g["cutoff"]), dropout, factor=g["factor"],
                              adaptive_inputs=inp if tie_weights else None, tie_proj=tie_proj)
    return inp, out


def table(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def main():
    install_shims()
    ai = importlib.import_module("fairseq.modules.adaptive_input")
    asm = importlib.import_module("fairseq.modules.adaptive_softmax")
    keys = {}
    with torch.device("meta"):
        inp, out = build(ai, asm, RECIPE, dropout=0.2)
    keys["recipe"] = dict(geometry=RECIPE, tie_weights=True, tie_proj=True, input=table(inp), output=table(out))
    for name, tw, tp in (("small_tied", True, True), ("small_untied_proj", True, False), ("small_untied", False, False)):
        inp, out = build(ai, asm, SMALL, tw, tp)
        keys[name] = dict(geometry=SMALL, tie_weights=tw, tie_proj=tp, input=table(inp), output=table(out))
    with open(os.path.join(HERE, "adaptive_keys.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)

    torch.manual_seed(20)
    inp, out = build(ai, asm, SMALL)
    inp.eval(), out.eval()
    with torch.no_grad():
        for p in list(inp.parameters()) + list(out.parameters()):
            p.copy_(p.to(torch.bfloat16).float())
        inp._float_tensor.zero_()
        out.head._float_tensor.zero_()
        c0, c1, V = SMALL["cutoff"][0], SMALL["cutoff"][1], SMALL["V"]
        g = torch.Generator().manual_seed(21)
        edges = [0, 1, c0 - 1, c0, c0 + 1, c1 - 1, c1, c1 + 1, V - 1]
        tokens = torch.randint(0, V, (2, 24), generator=g)
        tokens[0, :len(edges)] = torch.tensor(edges)
        tokens[1, -len(edges):] = torch.tensor(edges[::-1])
        targets = torch.roll(tokens.reshape(-1), 5).reshape(2, 24).contiguous()
        x = torch.randn(2, 24, SMALL["C"], generator=g) * 2.0
        embedded = inp(tokens)
        full = out.get_log_prob(x, None)
        at_targets = out.get_log_prob(x, targets).gather(-1, targets.unsqueeze(-1)).squeeze(-1)
    arrays = {"embed_tokens." + k: v.numpy() for k, v in inp.state_dict().items()}
    own = {k: v for k, v in out.state_dict().items() if not k.startswith("tail.") and k != "head.word_proj.weight"}
    arrays.update({"adaptive_softmax." + k: v.numpy() for k, v in own.items()})
    arrays.update(tokens=tokens.numpy(), targets=targets.numpy(), x=x.numpy(), embedded=embedded.numpy(),
                  logp_full=full.numpy(), logp_targets=at_targets.numpy())
    np.savez_compressed(os.path.join(HERE, "adaptive_small.npz"), **arrays)


if __name__ == "__main__":
    main()
