"""-m "not gpu": the interface of static incremental decoding (CausalEVAttention.init_static_decoding): its signature, and
that it refuses what dynamic decoding refuses, with the same messages, before allocating anything -- CPU devices included.
Its numerics are tests/test_gpu_ceva_static_decode.py."""
import inspect

import pytest
import torch

import efficient_attention as ea
from test_api_parity import _causal_eva


def _static(m, device="cpu", dtype=torch.bfloat16):
    return m.init_static_decoding({}, 2, 16, dtype, device)


def _dynamic(m):
    x = torch.randn(1, 2, 64)
    return m(x, x, x, incremental_state={})


def test_static_decoding_interface():
    sig = inspect.signature(ea.CausalEVAttention.init_static_decoding)
    assert list(sig.parameters) == ["self", "incremental_state", "batch_size", "max_tokens", "dtype", "device"]
    sig = inspect.signature(ea.CausalEVAttention.static_decoding_overflowed)
    assert list(sig.parameters) == ["self", "incremental_state"]


@pytest.mark.parametrize("case", ["encoder_decoder", "not_causal", "training", "adaptive_default"])
def test_static_decoding_refuses_what_dynamic_decoding_refuses(case):
    m = {"encoder_decoder": lambda: _causal_eva(self_attention=False).eval(),
         "not_causal": lambda: _causal_eva(attn_args=dict(causal=False)).eval(),
         "training": lambda: _causal_eva().train(),
         "adaptive_default": lambda: _causal_eva(attn_args=dict(adaptive_proj="default")).eval()}[case]()
    with pytest.raises(NotImplementedError) as dyn:
        _dynamic(m)
    with pytest.raises(NotImplementedError) as sta:
        _static(m)
    assert str(sta.value) == str(dyn.value)
    assert "incremental decoding" in str(sta.value) or "adaptive projection" in str(sta.value)


def test_static_decoding_needs_a_chunk_size():
    m = _causal_eva(attn_args=dict(chunk_size=None, num_chunks=4)).eval()
    with pytest.raises(NotImplementedError, match="needs --chunk-size"):
        _static(m)


@pytest.mark.parametrize("device", ["cpu", torch.device("cpu")], ids=["str", "device"])
def test_static_decoding_has_no_cpu_fallback(device):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _static(_causal_eva().eval(), device=device)


def test_static_decoding_cache_dtypes(monkeypatch):
    from efficient_attention import _f32
    with pytest.raises(ValueError, match="bf16, fp16 or fp32"):
        _static(_causal_eva().eval(), dtype=torch.float64)
    monkeypatch.setattr(_f32, "ENABLED", False)
    with pytest.raises(ValueError, match="fp32 cores"):
        _static(_causal_eva().eval(), dtype=torch.float32)
