"""Op layer: Python entry points for the gfx950 HIP kernels (``csrc/kernels``).

Each op dispatches on the tensor's device: CUDA(HIP) tensors run the native kernel (and fail
loudly if the library is missing), CPU tensors run an fp32 PyTorch reference that is also the
oracle in the numerics tests.
"""
from .activation import gelu_, silu_mul
from .attention import (KV_BS, DecodeWorkspace, KVScales, decode, default_scale, gather_kv_ref, kv_dequant,
                        make_kv_scales, prefill, rope_cos_sin, rope_kv_write, write_kv_ref)
from .embedding import embedding
from .norm import layer_norm, rms_norm
from .retrieval import (filtered_topk, filtered_topk_hybrid, filtered_topk_hybrid_ref, hybrid_query_weights,
                        lex_df_add)
from .sampling import (apply_top_k_top_p, fused_lm_head_ok, fused_logprob_ok, lm_head_logprobs, lm_head_sample,
                       lm_head_sample_logprob, lm_head_sample_shard, lm_head_stream_sample,
                       lm_head_stream_sample_logprob, merge_logprob_stats, pick_pairs, sample, sample_shard,
                       token_logprobs, topn_logprobs)
from .constrain import FsmTables, build_masks, sample_constrained
from . import penalty
from .penalty import PenaltyTable, apply_penalties
from . import lora
from .lora import LoRATable, lora_delta
from . import kv_tier
from .kv_tier import gather_blocks, scatter_blocks
from . import fp8_dense
from .fp8_dense import DenseFp8MLP, dense_fp8_gemm, dense_fp8_reference, mlp_fp8, quantize_dense_mlp
from . import mxfp4_dense
from .mxfp4_dense import (DenseMxfp4MLP, dense_mxfp4_gemm, dense_mxfp4_reference, expand_mxfp4, mlp_mxfp4,
                          quantize_dense_mlp_mxfp4, quantize_mxfp4_rowwise, unpack_mxfp4)

__all__ = ["gelu_", "silu_mul", "KV_BS", "DecodeWorkspace", "decode", "default_scale", "prefill", "rope_cos_sin",
           "rope_kv_write", "write_kv_ref", "gather_kv_ref", "kv_dequant", "KVScales", "make_kv_scales", "embedding", "layer_norm", "rms_norm", "filtered_topk",
           "filtered_topk_hybrid", "filtered_topk_hybrid_ref", "hybrid_query_weights", "lex_df_add",
           "apply_top_k_top_p", "sample"]
