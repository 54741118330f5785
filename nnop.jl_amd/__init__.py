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
with the gated activation in its epilogue and the token gather in front of the ninth, ``include/nnop_hip_moe_mx_decode_glu.h``;
``_common.py`` for the call plumbing they all share and ``_lib.py`` for the one loader of the nine ctypes bindings), the
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
from . import (_common, _lib, _lib_ext, _lib_moe, _lib_moe_data, _lib_moe_gemm, _lib_moe_linear, _lib_moe_mx, _lib_moe_mx_decode,
               _lib_moe_mx_decode_glu, activations, losses, moe, moe_data, moe_gemm, moe_linear, moe_mx, moe_mx_decode, moe_mx_decode_glu,
               qknorm, shard, workmodel)

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
           "shard", "workmodel", "_common", "_lib", "_lib_ext", "_lib_moe", "_lib_moe_data", "_lib_moe_gemm", "_lib_moe_linear", "_lib_moe_mx",
           "_lib_moe_mx_decode", "_lib_moe_mx_decode_glu"]
__version__ = "0.1.0"
