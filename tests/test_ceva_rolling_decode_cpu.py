"""-m "not gpu": the interface of rolling incremental decoding (CausalEVAttention.init_rolling_decoding, a static state whose
token rows live in a ring, and decoding_state_nbytes): the signatures, and that it refuses what init_static_decoding refuses,
with the same messages, before allocating anything -- CPU devices included -- plus a non-positive max_step_tokens.
Its numerics are tests/test_gpu_ceva_rolling_decode.py."""
import inspect

import pytest
import torch

import efficient_attention as ea
from test_api_parity import _causal_eva


def _static(m, device="cpu", dtype=torch.bfloat16, B=2, T=16):
    return m.init_static_decoding({}, B, T, dtype, device)


def _rolling(m, device="cpu", dtype=torch.bfloat16, B=2, T=16, **kw):
    return m.init_rolling_decoding({}, B, T, dtype, device, **kw)


def _both(exc, m_fn, **kw):
    """The two refusals, message for message."""
    with pytest.raises(exc) as sta:
        _static(m_fn(), **kw)
    with pytest.raises(exc) as rol:
        _rolling(m_fn(), **kw)
    assert type(rol.value) is type(sta.value) and str(rol.value) == str(sta.value)
    return str(rol.value)


def test_rolling_decoding_interface():
    sig = inspect.signature(ea.CausalEVAttention.init_rolling_decoding)
    assert list(sig.parameters) == ["self", "incremental_state", "batch_size", "max_tokens", "dtype", "device",
                                    "max_step_tokens"]
    assert sig.parameters["max_step_tokens"].default is None
    sig = inspect.signature(ea.CausalEVAttention.decoding_state_nbytes)
    assert list(sig.parameters) == ["self", "incremental_state"]
    # (unchanged: tests/test_ceva_static_decode_cpu.py pins it too)
    sig = inspect.signature(ea.CausalEVAttention.init_static_decoding)
    assert list(sig.parameters) == ["self", "incremental_state", "batch_size", "max_tokens", "dtype", "device"]


@pytest.mark.parametrize("case", ["encoder_decoder", "not_causal", "training", "adaptive_default"])
def test_rolling_decoding_refuses_what_static_decoding_refuses(case):
    m_fn = {"encoder_decoder": lambda: _causal_eva(self_attention=False).eval(),
            "not_causal": lambda: _causal_eva(attn_args=dict(causal=False)).eval(),
            "training": lambda: _causal_eva().train(),
            "adaptive_default": lambda: _causal_eva(attn_args=dict(adaptive_proj="default")).eval()}[case]
    msg = _both(NotImplementedError, m_fn)
    assert "incremental decoding" in msg or "adaptive projection" in msg


def test_rolling_decoding_needs_a_chunk_size():
    msg = _both(NotImplementedError, lambda: _causal_eva(attn_args=dict(chunk_size=None, num_chunks=4)).eval())
    assert "needs --chunk-size" in msg


@pytest.mark.parametrize("device", ["cpu", torch.device("cpu")], ids=["str", "device"])
def test_rolling_decoding_has_no_cpu_fallback(device):
    msg = _both(RuntimeError, lambda: _causal_eva().eval(), device=device)
    assert "no CPU fallback" in msg


def test_rolling_decoding_cache_dtypes(monkeypatch):
    from efficient_attention import _f32
    assert "bf16, fp16 or fp32" in _both(ValueError, lambda: _causal_eva().eval(), dtype=torch.float64)
    monkeypatch.setattr(_f32, "ENABLED", False)
    assert "fp32 cores" in _both(ValueError, lambda: _causal_eva().eval(), dtype=torch.float32)


@pytest.mark.parametrize("B,T", [(0, 16), (2, 0), (-1, 16), (2, -3)])
def test_rolling_decoding_sizes(B, T, monkeypatch):
    """Non-positive sizes: the ValueError of init_static_decoding, message for message, before anything is allocated.  The
    size check comes after the device check, which is stubbed here so that it is reached without a GPU."""
    from efficient_attention import _native
    monkeypatch.setattr(_native, "require_cuda", lambda *a, **k: None)
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("allocated before refusing"))
    msg = _both(ValueError, lambda: _causal_eva().eval(), B=B, T=T)
    assert "batch_size > 0 and max_tokens > 0" in msg and "%d, %d" % (B, T) in msg


def test_refusals_come_before_the_step_bound():
    """Everything init_static_decoding refuses is refused first; nothing is allocated or stored on a refusal."""
    m = _causal_eva().eval()
    st = {}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.init_rolling_decoding(st, 2, 16, torch.bfloat16, "cpu", max_step_tokens=0)
    assert st == {}


@pytest.mark.parametrize("S", [0, -5])
def test_rolling_decoding_refuses_a_non_positive_step_bound(S, monkeypatch):
    """ValueError for max_step_tokens <= 0, before anything is allocated (the device check is stubbed: no GPU needed)."""
    from efficient_attention import _native
    monkeypatch.setattr(_native, "require_cuda", lambda *a, **k: None)
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("allocated before refusing"))
    m = _causal_eva().eval()
    st = {}
    with pytest.raises(ValueError, match="max_step_tokens"):
        m.init_rolling_decoding(st, 2, 16, torch.bfloat16, "cpu", max_step_tokens=S)
    assert st == {}


def test_decoding_state_nbytes_of_an_empty_state():
    m = _causal_eva().eval()
    m.init_incremental_state()
    assert m.decoding_state_nbytes({}) == 0
    assert m.decoding_state_nbytes(None) == 0
