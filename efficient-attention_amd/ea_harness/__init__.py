"""ea_harness -- the callers either side of the attention hot path.

Builder-written stand-ins for the reference's two harnesses, so that BASELINE.json's configs 2-5 run
as WHOLE models (eager, autocast, DistributedDataParallel over RCCL) on synthetic data:

  vision.DeiTStack      -- the vit/ classifier: patch stem, 12 pre-norm blocks around
                           AttentionFactory.build_attention, mean-pool head
                           (vit/models/efficient_vit.py:85-119,122-233; state_dict keys match)
  vision.PvTStack       -- the four-stage pyramid (3-4-6-3 blocks, sr_ratio -> attention choice)
                           (vit/models/pvt_legacy.py:66-93,187-268; state_dict keys match)
  sequence.EncoderStack -- a fairseq-free Time x Batch x Channel encoder whose self-attention is the
                           adapter of fairseq/fairseq/modules/efficient_attention.py:107-132
  sequence.DecoderStack -- the decoder-only LM of the wikitext-103 recipe around CausalEVAttention
                           (fairseq/modules/transformer_layer.py:236-308 without encoder attention), with
                           incremental decoding on the attention's static / rolling states: init_decoding,
                           decode, generate, beam_search, score; every decoding mode is its argument checks
                           around a pick of token_pick
  token_pick            -- what the decoding modes share: DecodingState and what is attached to it (Sampler,
                           Scorer, Beam, AdaptivePick, the held vocabulary pair) with one lifecycle, the operand
                           helpers of the vocabulary entries, and one pick per launch behind one selector
  vocab_loss            -- vocab_nll: the vocabulary cross-entropy of the plain tied table as one autograd Function,
                           ea_vocab_score forward and a chunked HIP backward (ea_vocab_nll_grad, ea_gemm_nt16), without
                           a [rows, V] tensor; DecoderStack.loss is the stack's forward in front of it
  adaptive_loss         -- adaptive_nll: fairseq's adaptive-softmax criterion as one autograd Function, ea_adaptive_score
                           forward and a HIP backward over device-counted row lists (ea_vocab_nll_grad_rows,
                           ea_gemm_nt16_rows, ea_rows_transpose16); DecoderStack.adaptive_loss is the stack in front of it
  trainer               -- one synthetic training step (forward, loss, backward, optimizer) eagerly or
                           captured in a hipGraph, single process or one process per GPU

Only the attention layers are this repo's product; everything else here is plain PyTorch plumbing
(library GEMMs / MIOpen convolutions) that exists to drive the path the way its call sites do.
"""
from .vision import DeiTStack, PvTStack, deit_tiny, pvt_b2           # noqa: F401
from .sequence import EncoderStack, wmt_en_de_encoder                # noqa: F401
from .sequence import DecoderLayer, DecoderStack, wikitext103_decoder   # noqa: F401
