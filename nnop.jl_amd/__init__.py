"""nnop.jl_amd -- MI355X-native Flash Attention behind NNop.jl's operator API.

Holds only what the hot path needs: ``csrc/`` (hand-written gfx950 HIP kernels + the C ABI of
``include/nnop_hip.h``), the host-side mirror of the reference interface (``attention.py``; ``rope.py`` for the
Llama rotary embedding applied to q, k right before attention -- SURVEY.md section 8(f) rank 2; ``softmax.py``, ``norms.py``,
``activations.py`` for the MLP's gated activation, ``losses.py`` for the cross-entropy over the LM head's logits and
``qknorm.py`` for the fused QK-norm + RoPE of the extension library, ``include/nnop_hip_ext.h``, ``moe.py`` for the
mixture-of-experts gate and dispatch plan of the third library, ``include/nnop_hip_moe.h``, ``moe_data.py`` for the token
permute and weighted combine of the fourth, ``include/nnop_hip_moe_data.h``, ``moe_gemm.py`` for the grouped expert GEMM of
the fifth, ``include/nnop_hip_moe_gemm.h``, ``moe_linear.py`` for the expert linear layers (bias, [E, K, N] weights, accumulating
gradients) of the sixth, ``include/nnop_hip_moe_linear.h``, ``moe_mx.py`` for the same layers on MXFP4 expert weights (packed blocks
and scale bytes read where they lie, forward and the pullback to the rows) and the MXFP4 quantiser and dequantiser of the seventh,
``include/nnop_hip_moe_mx.h``, ``moe_mx_decode.py`` for the weight-streaming forward of those layers at decode sizes (few rows per
expert) of the eighth, ``include/nnop_hip_moe_mx_decode.h``, ``moe_mx_decode_glu.py`` for that forward on a fused gate-up projection
with the gated activation in its epilogue and the token gather in front of the ninth, ``include/nnop_hip_moe_mx_decode_glu.h``,
``decode_attn.py`` for the attention of a decode step over a KV cache (split-KV, packed GQA, sinks, lengths on the device) of the
tenth, ``include/nnop_hip_decode_attn.h``, ``decode_attn_fp8.py`` for that attention over a cache of one-byte E4M3 codes with a scale
per KV head, expanded in registers, of the eleventh, ``include/nnop_hip_decode_attn_fp8.h``, ``paged_attn.py`` for that attention over
a paged cache (a pool of pages and a block table per sequence, read where they lie) of the twelfth, ``include/nnop_hip_paged_attn.h``,
``paged_prefill.py`` for the prefill step over that cache -- a variable number of new tokens per sequence, packed token-major, behind a
cached prefix (a prompt, a chunk of a chunked prefill, speculative verification of more than 16 rows); row blocks of 128 / G tokens
times the G heads of a KV head, 32-key tiles shared through two LDS images, scores transposed on the 32x32x16 MFMA, table entries
fetched a tile ahead, each workgroup finding its block by a search over cu_seqlens_q (no workspace); forward only, no
split-KV -- of the thirteenth, ``include/nnop_hip_paged_prefill.h``, ``paged_attn_fp8.py`` for the decode step over pages of one-byte
E4M3 codes -- the eleventh library's data path behind the twelfth's block table, the table entries of each of the four ring slots
fetched a refill ahead -- of the fourteenth, ``include/nnop_hip_paged_attn_fp8.h``, ``paged_prefill_fp8.py`` for the prefill step over
those pages of codes -- the thirteenth library's kernel with the codes expanded to q's type in the registers that stage a tile for LDS,
once per tile and off the loop's critical path -- of the fifteenth, ``include/nnop_hip_paged_prefill_fp8.h``,
``paged_prefill_split.py`` for the thirteenth library's prefill step with split-KV -- few new tokens behind a long context: every row
block's key tiles cut into chunks, a workgroup each running the same kernel text over its chunk, fp32 partial results in a workspace and
a merge kernel of one wave per (token, head) row -- of the sixteenth, ``include/nnop_hip_paged_prefill_split.h``,
``paged_kv_write.py`` for the write side of that cache -- the new tokens' K and V rows into their pages in one launch, bit for bit into a
16-bit pool or as E4M3 codes by the project's one quantisation rule, a wave per token with its sequence, position and table entry in
scalar registers and its lanes moving 16-byte pieces -- of the seventeenth, ``include/nnop_hip_paged_kv_write.h``,
``mla_decode.py`` for the decode step of multi-head latent attention (DeepSeek's MLA, weight-absorbed) over a paged latent cache -- one
576-wide row per key that is the key and the value of up to 128 heads, a 32-key tile fetched once per workgroup into one of two LDS
images and read two ways, row-wise for the scores and through the transposing LDS read for the values, 16 heads per wave -- of the
eighteenth, ``include/nnop_hip_mla_decode.h``;
``_common.py`` for the call plumbing they all share and ``_lib.py`` for the one loader of the eighteen ctypes bindings), the
(batch, kv-head) sharding used for multi-GPU runs (``shard.py``) and the Julia package-extension
shim (``julia/``, source only: no Julia in this image).

The directory name contains a dot, so import it through ``__graft_entry__.load_package()``
(registers it as module ``nnop_jl_amd``).
"""
from ._common import NNopError
from .attention import (flash_attention, _flash_attention, grad_flash_attention,
                        shared_memory, bwd_workspace_bytes, fa_fwd_into, fa_bwd_into)
from .rope import LlamaRotaryEmbedding, llama_rope, _llama_rope, grad_llama_rope, llama_rope_into
from .softmax import online_softmax, grad_online_softmax, online_softmax_into
from .norms import rms_norm, _rms_norm, grad_rms_norm, layer_norm, _layer_norm, grad_layer_norm
from .norms import (add_rms_norm, _add_rms_norm, grad_add_rms_norm, add_layer_norm, _add_layer_norm,
                    grad_add_layer_norm)
from .activations import (glu, swiglu, geglu, glu_packed, _glu, grad_glu, grad_glu_packed, glu_into, grad_glu_into)
from .losses import cross_entropy, _cross_entropy, grad_cross_entropy
from .qknorm import qk_norm_rope, _qk_norm_rope, grad_qk_norm_rope, qk_norm_rope_into, grad_qk_norm_rope_into
from .moe import (moe_router, _moe_router, grad_moe_router, moe_router_into, grad_moe_router_into, moe_dispatch_plan,
                  moe_dispatch_plan_into)
from .moe_data import (moe_permute, _moe_permute, grad_moe_permute, moe_permute_into, grad_moe_permute_into, moe_combine, _moe_combine,
                       grad_moe_combine, moe_combine_into, grad_moe_combine_into)
from .moe_gemm import (moe_grouped_gemm, _moe_grouped_gemm, grad_moe_grouped_gemm, moe_grouped_gemm_into,
                       grad_moe_grouped_gemm_x_into, grad_moe_grouped_gemm_w_into)
from .moe_linear import (moe_grouped_linear, _moe_grouped_linear, grad_moe_grouped_linear, moe_grouped_linear_into,
                         grad_moe_grouped_linear_x_into, grad_moe_grouped_linear_w_into, grad_moe_grouped_linear_b_into)
from .moe_mx import (mxfp4_quantize, mxfp4_dequantize, moe_grouped_linear_mxfp4, _moe_grouped_linear_mxfp4,
                     moe_grouped_linear_mxfp4_into, grad_moe_grouped_linear_mxfp4_x_into)
from .moe_mx_decode import moe_decode_linear_mxfp4, _moe_decode_linear_mxfp4, moe_decode_linear_mxfp4_into
from .moe_mx_decode_glu import moe_decode_glu_mxfp4, _moe_decode_glu_mxfp4, moe_decode_glu_mxfp4_into
from .decode_attn import decode_attention, decode_attention_into, decode_attention_plan
from .decode_attn_fp8 import decode_attention_fp8, decode_attention_fp8_into, decode_attention_fp8_plan
from .paged_attn import paged_decode_attention, paged_decode_attention_into, paged_decode_attention_plan
from .paged_prefill import paged_prefill_attention, paged_prefill_attention_into, paged_prefill_attention_plan
from .paged_attn_fp8 import paged_decode_attention_fp8, paged_decode_attention_fp8_into, paged_decode_attention_fp8_plan
from .paged_prefill_fp8 import paged_prefill_attention_fp8, paged_prefill_attention_fp8_into, paged_prefill_attention_fp8_plan
from .paged_prefill_split import paged_prefill_attention_split, paged_prefill_attention_split_into, paged_prefill_attention_split_plan
from .paged_kv_write import paged_kv_cache_write
from .mla_decode import mla_decode_attention, mla_decode_attention_into, mla_decode_attention_plan
from . import (_common, _lib, _lib_decode_attn, _lib_decode_attn_fp8, _lib_ext, _lib_moe, _lib_moe_data, _lib_moe_gemm, _lib_moe_linear, _lib_moe_mx, _lib_moe_mx_decode,
               _lib_moe_mx_decode_glu, _lib_mla_decode, _lib_paged_attn, _lib_paged_attn_fp8, _lib_paged_kv_write, _lib_paged_prefill, _lib_paged_prefill_fp8, _lib_paged_prefill_split, activations, decode_attn, decode_attn_fp8, losses, moe, moe_data, moe_gemm, moe_linear, moe_mx, moe_mx_decode, moe_mx_decode_glu,
               mla_decode, paged_attn, paged_attn_fp8, paged_kv_write, paged_prefill, paged_prefill_fp8, paged_prefill_split, qknorm, shard, workmodel)

__all__ = ["NNopError", "flash_attention", "_flash_attention", "grad_flash_attention",
           "shared_memory", "bwd_workspace_bytes", "fa_fwd_into", "fa_bwd_into", "LlamaRotaryEmbedding", "llama_rope", "_llama_rope", "grad_llama_rope", "llama_rope_into",
           "online_softmax", "grad_online_softmax", "online_softmax_into",
           "rms_norm", "_rms_norm", "grad_rms_norm", "layer_norm", "_layer_norm", "grad_layer_norm",
           "add_rms_norm", "_add_rms_norm", "grad_add_rms_norm", "add_layer_norm", "_add_layer_norm", "grad_add_layer_norm",
           "glu", "swiglu", "geglu", "glu_packed", "_glu", "grad_glu", "grad_glu_packed", "glu_into", "grad_glu_into", "activations",
           "cross_entropy", "_cross_entropy", "grad_cross_entropy", "losses",
           "qk_norm_rope", "_qk_norm_rope", "grad_qk_norm_rope", "qk_norm_rope_into", "grad_qk_norm_rope_into", "qknorm",
           "moe_router", "_moe_router", "grad_moe_router", "moe_router_into", "grad_moe_router_into", "moe_dispatch_plan",
           "moe_dispatch_plan_into", "moe",
           "moe_permute", "_moe_permute", "grad_moe_permute", "moe_permute_into", "grad_moe_permute_into", "moe_combine", "_moe_combine",
           "grad_moe_combine", "moe_combine_into", "grad_moe_combine_into", "moe_data",
           "moe_grouped_gemm", "_moe_grouped_gemm", "grad_moe_grouped_gemm", "moe_grouped_gemm_into", "grad_moe_grouped_gemm_x_into",
           "grad_moe_grouped_gemm_w_into", "moe_gemm",
           "moe_grouped_linear", "_moe_grouped_linear", "grad_moe_grouped_linear", "moe_grouped_linear_into",
           "grad_moe_grouped_linear_x_into", "grad_moe_grouped_linear_w_into", "grad_moe_grouped_linear_b_into", "moe_linear",
           "mxfp4_quantize", "mxfp4_dequantize", "moe_grouped_linear_mxfp4", "_moe_grouped_linear_mxfp4",
           "moe_grouped_linear_mxfp4_into", "grad_moe_grouped_linear_mxfp4_x_into", "moe_mx",
           "moe_decode_linear_mxfp4", "_moe_decode_linear_mxfp4", "moe_decode_linear_mxfp4_into", "moe_mx_decode",
           "moe_decode_glu_mxfp4", "_moe_decode_glu_mxfp4", "moe_decode_glu_mxfp4_into", "moe_mx_decode_glu",
           "decode_attention", "decode_attention_into", "decode_attention_plan", "decode_attn", "_lib_decode_attn",
           "decode_attention_fp8", "decode_attention_fp8_into", "decode_attention_fp8_plan", "decode_attn_fp8", "_lib_decode_attn_fp8",
           "paged_decode_attention", "paged_decode_attention_into", "paged_decode_attention_plan", "paged_attn", "_lib_paged_attn",
           "paged_prefill_attention", "paged_prefill_attention_into", "paged_prefill_attention_plan", "paged_prefill", "_lib_paged_prefill",
           "paged_decode_attention_fp8", "paged_decode_attention_fp8_into", "paged_decode_attention_fp8_plan", "paged_attn_fp8",
           "_lib_paged_attn_fp8",
           "paged_prefill_attention_fp8", "paged_prefill_attention_fp8_into", "paged_prefill_attention_fp8_plan", "paged_prefill_fp8",
           "_lib_paged_prefill_fp8",
           "paged_prefill_attention_split", "paged_prefill_attention_split_into", "paged_prefill_attention_split_plan", "paged_prefill_split",
           "_lib_paged_prefill_split",
           "paged_kv_cache_write", "paged_kv_write", "_lib_paged_kv_write",
           "mla_decode_attention", "mla_decode_attention_into", "mla_decode_attention_plan", "mla_decode", "_lib_mla_decode",
           "shard", "workmodel", "_common", "_lib", "_lib_ext", "_lib_moe", "_lib_moe_data", "_lib_moe_gemm", "_lib_moe_linear", "_lib_moe_mx",
           "_lib_moe_mx_decode", "_lib_moe_mx_decode_glu"]
__version__ = "0.1.0"
