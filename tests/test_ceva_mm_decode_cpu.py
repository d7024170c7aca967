"""-m "not gpu": the interface of `matrix_prompts` (csrc/ea_ceva_decode_mm.hip) and of its two entry points, additions to C ABI 38."""
import inspect

import efficient_attention as ea
from test_cabi import declared_symbols, lib  # noqa: F401  (the fixture builds the library when it is missing)


def test_the_two_entry_points_are_declared_bound_and_exported_with_attns_arguments(lib):  # noqa: F811
    from efficient_attention import _native
    for name, twin in (("ea_ceva_sdecode_attn_mm", "ea_ceva_sdecode_attn"), ("ea_ceva_sdecode_attn_mm_l16", "ea_ceva_sdecode_attn_l16")):
        assert name in declared_symbols() and hasattr(lib, name)
        assert _native.SIGNATURES[name] == _native.SIGNATURES[twin] and len(_native.SIGNATURES[name]) == 10
    assert _native.lib().ea_abi_version() == 38 == _native.ABI_VERSION      # additions only: no signature changed


def test_matrix_prompts_is_a_keyword_that_defaults_to_off():
    from ea_harness import sequence as sq
    for f in (ea.CausalEVAttention.init_static_decoding, ea.CausalEVAttention.init_rolling_decoding, sq.DecoderStack.init_decoding):
        assert inspect.signature(inspect.unwrap(f)).parameters["matrix_prompts"].default is False
        assert "matrix_prompts" not in inspect.signature(f).parameters      # (the lists the other tests pin stay)
        assert "matrix_prompts" in f.__doc__
