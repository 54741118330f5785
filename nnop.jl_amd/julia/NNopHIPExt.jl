# NNopHIPExt.jl -- package extension that routes NNop's Flash Attention to libnnop_hip.so on AMD GPUs.
#
# SOURCE ONLY: there is no Julia in the build image, so this file is not executed by the test-suite;
# the identical C calls are exercised from Python (nnop.jl_amd/_lib.py + attention.py).  It has the
# shape of the reference's own extension (ext/NNopAMDGPUExt.jl:1-11): it only ADDS METHODS to
# functions owned by NNop, so nothing else in the package changes:
#
#   NNop._shared_memory(::ROCBackend, device_id)             ext/NNopAMDGPUExt.jl:6-9
#   NNop._flash_attention(q,k,v,pair; causal,kpad_mask)       src/attention.jl:133-177   -> (o, ms, ls)
#   NNop.∇flash_attention(Δ,o,ms,ls,q,k,v,pair; causal,...)   src/attention_bwd.jl:199-275 -> (dq,dk,dv,dpair)
#   NNop._llama_rope(q, k, cos, sin; bwd)                     src/rope/llama_rope.jl:69-89 -> (q', k')
#   NNop.online_softmax(x) / NNop.∇online_softmax(Δ, y)       src/softmax.jl:60-80
#   NNop._rms_norm / NNop.∇rms_norm                           src/rms_norm.jl:117-169
#   NNop._layer_norm / NNop.∇layer_norm                       src/layer_norm.jl:150-204
#   add_rms_norm / add_layer_norm (+ _fwd / _bwd, rrules)     the residual add fused into the norms (this library's own)
#   glu (+ glu_fwd / glu_bwd, rrules)                         gated MLP activations: SwiGLU, GeGLU, gpt-oss (this library's own)
#   cross_entropy (+ cross_entropy_fwd / _bwd, rrule)         loss over the LM head's logits: cap, z-loss, smoothing (this library's own)
#   qk_norm_rope (+ qk_norm_rope_fwd / _bwd, rrule)           fused QK-norm + RoPE, from the second library libnnop_hip_ext.so
#
# `flash_attention` and the ChainRules `rrule` (src/attention_crc.jl:4-31) call these generically, so
# `NNop.flash_attention(q, k, v; causal)` and `Zygote.gradient` keep working unchanged.
#
# Install (see INTEGRATION.md):  in NNop's Project.toml
#     [extensions]
#     NNopHIPExt = "AMDGPU"          # REPLACES the line `NNopAMDGPUExt = "AMDGPU"`
# and put this file at ext/NNopHIPExt.jl; point ENV["NNOP_HIP_LIB"] at libnnop_hip.so.
# It replaces NNopAMDGPUExt, it cannot sit beside it: both define NNop._shared_memory(::ROCBackend, ::Integer), and
# two extensions defining one method is a method overwrite, which Julia rejects during precompilation.
#
# GC / stream safety of the ccalls: every array whose raw device pointer is passed is held by GC.@preserve for the
# duration of the call; the library only ENQUEUES kernels on the task-local HIP stream and keeps no pointer.  Arrays
# that die right after the call (the backward workspace `ws`) are safe because AMDGPU.jl frees device memory in stream
# order (hipFreeAsync on the same task-local stream), i.e. after the kernels enqueued here.
module NNopHIPExt

using AMDGPU
using NNop

export local_flash_attention, flash_attention_sinks, softcap_flash_attention, add_rms_norm, add_layer_norm, glu, cross_entropy, qk_norm_rope

const LIB = Ref{String}("")
libnnop() = isempty(LIB[]) ? (LIB[] = get(ENV, "NNOP_HIP_LIB", "libnnop_hip.so")) : LIB[]

# struct nnop_fa_desc (include/nnop_hip.h)
struct FaDesc
    dtype::Int32; emb::Int32; ql::Int32; kl::Int32; qh::Int32; kh::Int32; batch::Int32; causal::Int32
    emb_k::Int32; emb_v::Int32; kl_v::Int32; kh_v::Int32
end

# nnop_dtype
nnop_dtype(::Type{Float32}) = Int32(0)
nnop_dtype(::Type{Float16}) = Int32(1)
# BFloat16 is a Core type from Julia 1.11 on; on older Julia the extension still loads, without the bf16 methods
@static if isdefined(Core, :BFloat16)
    nnop_dtype(::Type{Core.BFloat16}) = Int32(2)      # BFloat16s.BFloat16 (>= 0.5 on 1.11) is this same type
    const HipFloat = Union{Float32, Float16, Core.BFloat16}
else
    const HipFloat = Union{Float32, Float16}
end

# nnop_status -> the reference's ErrorException messages (src/attention.jl:141-144, :204)
function check(st::Cint, q, k, v)
    st == 0 && return
    QE, KE = size(q, 1), size(k, 1)
    st == -1 && error("Embedding dim of Q `$QE` must be the same as of K `$KE`.")
    st == -2 && error("Shapes of K `$(size(k))` and V `$(size(v))` must be the same.")
    st == -3 && error("Only power-of-2 embedding dims are supported.")
    st == -4 && error("Number of query heads `$(size(q, 3))` must be divisible by number of KV heads `$(size(k, 3))`.")
    st == -7 && error("Failed to find groupsize for Flash Attention that satisfies Shared Memory constraint.")
    st == -11 && error("libnnop_hip: a tensor base address is not 16-byte aligned (q, k, v, o, the gradients of q, k, v and the workspace; views of those with odd element offsets are not supported: copy them.  pair / dpair, ms, ls need their element size only)")
    msg = unsafe_string(ccall((:nnop_strerror, libnnop()), Cstring, (Cint,), st))
    error("libnnop_hip: $msg")
end

desc(q, k, v, causal) = FaDesc(nnop_dtype(eltype(q)), size(q, 1), size(q, 2), size(k, 2), size(q, 3), size(k, 3),
                               size(q, 4), causal ? 1 : 0, size(k, 1), size(v, 1), size(v, 2), size(v, 3))

devptr(x) = Ptr{Cvoid}(UInt(pointer(x)))             # device VA of a ROCArray
devptr(::Nothing) = Ptr{Cvoid}(0)
hipstream() = Ptr{Cvoid}(UInt(AMDGPU.stream().stream))   # the task-local HIP stream the arrays live on

# ext/NNopAMDGPUExt.jl:6-9 (device_id is 1-based in AMDGPU.devices())
function NNop._shared_memory(::ROCBackend, device_id::Integer)
    out = Ref{UInt64}(0)
    st = ccall((:nnop_shared_memory, libnnop()), Cint, (Cint, Ptr{UInt64}), device_id - 1, out)
    st == 0 || error("nnop_shared_memory failed ($st)")
    return out[]
end

# src/attention.jl:133-177
function NNop._flash_attention(
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4},
    pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing,
) where T <: HipFloat
    d = Ref(desc(q, k, v, causal))
    o  = similar(q)                                            # :166
    ms = ROCArray{T}(undef, size(q, 2), size(q, 3), size(q, 4))  # :167  (QL, QH, B)
    ls = similar(ms)                                           # :168
    st = GC.@preserve o ms ls q k v pair kpad_mask ccall((:nnop_fa_fwd, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(o), devptr(ms), devptr(ls), devptr(q), devptr(k), devptr(v), devptr(pair), devptr(kpad_mask), hipstream())
    check(st, q, k, v)
    return o, ms, ls                                           # asynchronous, like the KA launch (:170-176)
end

# src/attention_bwd.jl:199-275
function NNop.∇flash_attention(
    Δ::ROCArray{T,4},
    o::ROCArray{T,4}, ms::ROCArray{T,3}, ls::ROCArray{T,3},
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4},
    pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing,
) where T <: HipFloat
    d = Ref(desc(q, k, v, causal))
    nbytes = ccall((:nnop_fa_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{FaDesc},), d)
    if nbytes != 0 && pair !== nothing
        # scratch for the head-major copies of the bias: the backward then runs on 16-byte accesses (include/nnop_hip.h)
        nbytes = max(nbytes, ccall((:nnop_fa_bwd_workspace_bytes_pair, libnnop()), Csize_t, (Ptr{FaDesc},), d))
    end
    if nbytes == 0
        # invalid descriptor (the same four checks as the forward, src/attention_bwd.jl:210-213): a call with NULL
        # tensors returns the status of the failed check before it looks at any pointer
        null = Ptr{Cvoid}(0)
        st = ccall((:nnop_fa_bwd, libnnop()), Cint,
            (Ptr{FaDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
             Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
             Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
             Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
            d, null, null, null, null, null, null, null, null, null, null, null, null, null, null, Csize_t(0), null)
        check(st, q, k, v)
        error("libnnop_hip: invalid attention descriptor")    # unreachable when check() raised
    end
    dq, dk, dv = similar(q), similar(k), similar(v)           # fully overwritten by the library
    dp = isnothing(pair) ? nothing : similar(pair)
    ws = ROCArray{UInt8}(undef, nbytes)                        # replaces Δ_scaled / δ (:224-225)
    st = GC.@preserve dq dk dv dp Δ o ms ls q k v pair kpad_mask ws ccall((:nnop_fa_bwd, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},          # dq dk dv dpair
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},                      # Δ o ms ls
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},          # q k v pair kpad_mask
         Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),                                    # workspace, bytes, stream
        d, devptr(dq), devptr(dk), devptr(dv), devptr(dp), devptr(Δ), devptr(o), devptr(ms), devptr(ls),
        devptr(q), devptr(k), devptr(v), devptr(pair), devptr(kpad_mask), devptr(ws), nbytes, hipstream())
    check(st, q, k, v)
    return dq, dk, dv, dp
end

# A cotangent that is not a ROCArray -- the lazy `FillArrays.Fill` Zygote produces for `sum(flash_attention(...))`
# (test/attention_tests.jl:36-41), a Broadcasted, a host Array -- would miss the method above and fall through to the
# reference's generic KernelAbstractions backward.  Materialise it on the device and stay on the HIP path.
_to_roc(Δ::ROCArray, like) = Δ
_to_roc(Δ::Array, like) = copyto!(similar(like), Δ)
_to_roc(Δ, like) = (d = similar(like); d .= Δ; d)           # Fill / lazy wrappers broadcast without scalar indexing
function NNop.∇flash_attention(
    Δ::AbstractArray{<:Real,4},
    o::ROCArray{T,4}, ms::ROCArray{T,3}, ls::ROCArray{T,3},
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4},
    pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing,
) where T <: HipFloat
    return NNop.∇flash_attention(_to_roc(Δ, o)::ROCArray{T,4}, o, ms, ls, q, k, v, pair; causal, kpad_mask)
end

# ---- sliding-window (local) attention (include/nnop_hip.h: nnop_fa_opts, nnop_fa_fwd_ex / nnop_fa_bwd_ex, ABI version 7) --------------
# NNop's own `flash_attention` keeps the reference's signature; the window is a function of this extension.  `window = (left, right)`
# in flash-attn's `window_size` convention: query i sees key j iff i - left <= j <= i + right (1-based or 0-based alike: the rule
# is on differences), -1 = unbounded side, on top of `causal` and `kpad_mask`; top-left aligned whatever QL and KL are.
const ABI_VERSION = 7
function check_abi()
    v = ccall((:nnop_abi_version, libnnop()), Cint, ())
    v == ABI_VERSION || error("libnnop_hip has ABI version $v, this extension needs $ABI_VERSION")
    return nothing
end

# struct nnop_fa_opts
struct FaOpts
    window_left::Int32
    window_right::Int32
    reserved::NTuple{6, Int32}
end
FaOpts(window::Tuple{Integer, Integer}) = FaOpts(Int32(window[1]), Int32(window[2]), ntuple(_ -> Int32(0), 6))

function local_flash_attention_fwd(
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4}, pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, window::Tuple{Integer, Integer}, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing,
) where T <: HipFloat
    check_abi()
    d = Ref(desc(q, k, v, causal))
    op = Ref(FaOpts(window))
    o  = similar(q)
    ms = ROCArray{T}(undef, size(q, 2), size(q, 3), size(q, 4))
    ls = similar(ms)
    st = GC.@preserve o ms ls q k v pair kpad_mask ccall((:nnop_fa_fwd_ex, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{FaOpts}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}),
        d, op, devptr(o), devptr(ms), devptr(ls), devptr(q), devptr(k), devptr(v), devptr(pair), devptr(kpad_mask), hipstream())
    check(st, q, k, v)
    return o, ms, ls
end

function local_flash_attention_bwd(
    Δ::ROCArray{T,4}, o::ROCArray{T,4}, ms::ROCArray{T,3}, ls::ROCArray{T,3},
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4}, pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, window::Tuple{Integer, Integer}, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing,
) where T <: HipFloat
    d = Ref(desc(q, k, v, causal))
    op = Ref(FaOpts(window))
    # a window needs no more scratch than the plain backward (with a pair bias it always takes the direct path)
    nbytes = ccall((:nnop_fa_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{FaDesc},), d)
    nbytes == 0 && error("libnnop_hip: invalid attention descriptor")
    dq, dk, dv = similar(q), similar(k), similar(v)
    dp = isnothing(pair) ? nothing : similar(pair)
    ws = ROCArray{UInt8}(undef, nbytes)
    st = GC.@preserve dq dk dv dp Δ o ms ls q k v pair kpad_mask ws ccall((:nnop_fa_bwd_ex, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{FaOpts}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        d, op, devptr(dq), devptr(dk), devptr(dv), devptr(dp), devptr(Δ), devptr(o), devptr(ms), devptr(ls),
        devptr(q), devptr(k), devptr(v), devptr(pair), devptr(kpad_mask), devptr(ws), nbytes, hipstream())
    check(st, q, k, v)
    return dq, dk, dv, dp
end

"""
    local_flash_attention(q, k, v, pair=nothing; causal, window, kpad_mask=nothing)

Sliding-window (local) Flash Attention on the HIP kernels: `NNop.flash_attention` with query i seeing only keys
i - window[1] .. i + window[2] (-1 = unbounded side).  Differentiable through the ChainRules rule below.
"""
local_flash_attention(q, k, v, pair = nothing; causal::Bool, window::Tuple{Integer, Integer}, kpad_mask = nothing) =
    local_flash_attention_fwd(q, k, v, pair; causal, window, kpad_mask)[1]

# the shape of the reference's rrule (src/attention_crc.jl:16-31): no tangent for the window or the mask
function NNop.CRC.rrule(::typeof(local_flash_attention), q, k, v, pair = nothing;
                                   causal::Bool, window::Tuple{Integer, Integer}, kpad_mask = nothing)
    o, ms, ls = local_flash_attention_fwd(q, k, v, pair; causal, window, kpad_mask)
    function local_flash_attention_pullback(Δ)
        dq, dk, dv, dp = local_flash_attention_bwd(_to_roc(NNop.CRC.unthunk(Δ), o), o, ms, ls, q, k, v, pair;
                                                   causal, window, kpad_mask)
        return NNop.CRC.NoTangent(), dq, dk, dv, isnothing(pair) ? NNop.CRC.NoTangent() : dp
    end
    return o, local_flash_attention_pullback
end

# ---- learned attention sinks (include/nnop_hip.h: nnop_fa_fwd_sinks / nnop_fa_bwd_sinks) ---------------------------------------------
# One trainable logit per QUERY head (gpt-oss): every row's softmax gets one more column of logit sinks[h] and no value vector.  `causal`,
# `window` and `kpad_mask` act on the real keys only; -Inf32 = no sink for that head.  (o, ms, ls) include the sink, so the backward
# kernels recompute the right P; the library adds the gradient of the sinks.  Not part of the sharding helpers below.
function flash_attention_sinks_fwd(
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4}, sinks::ROCVector{Float32}, pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, window::Tuple{Integer, Integer} = (-1, -1), kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing,
) where T <: HipFloat
    check_abi()
    length(sinks) == size(q, 3) || error("sinks must have one entry per query head ($(size(q, 3))), got $(length(sinks))")
    d = Ref(desc(q, k, v, causal))
    op = Ref(FaOpts(window))
    o  = similar(q)
    ms = ROCArray{T}(undef, size(q, 2), size(q, 3), size(q, 4))
    ls = similar(ms)
    st = GC.@preserve o ms ls q k v sinks pair kpad_mask ccall((:nnop_fa_fwd_sinks, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{FaOpts}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}, Ptr{Cvoid}),
        d, op, devptr(sinks), devptr(o), devptr(ms), devptr(ls), devptr(q), devptr(k), devptr(v), devptr(pair), devptr(kpad_mask),
        hipstream())
    check(st, q, k, v)
    return o, ms, ls
end

function flash_attention_sinks_bwd(
    Δ::ROCArray{T,4}, o::ROCArray{T,4}, ms::ROCArray{T,3}, ls::ROCArray{T,3},
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4}, sinks::ROCVector{Float32}, pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, window::Tuple{Integer, Integer} = (-1, -1), kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing,
) where T <: HipFloat
    d = Ref(desc(q, k, v, causal))
    op = Ref(FaOpts(window))
    # a sink needs no more scratch than the plain backward
    nbytes = ccall((:nnop_fa_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{FaDesc},), d)
    nbytes == 0 && error("libnnop_hip: invalid attention descriptor")
    dq, dk, dv = similar(q), similar(k), similar(v)
    dp = isnothing(pair) ? nothing : similar(pair)
    ds = similar(sinks)                                        # fully overwritten by the library
    ws = ROCArray{UInt8}(undef, nbytes)
    st = GC.@preserve dq dk dv dp ds Δ o ms ls q k v sinks pair kpad_mask ws ccall((:nnop_fa_bwd_sinks, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{FaOpts}, Ptr{Cvoid}, Ptr{Cvoid},                    # sinks dsinks
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},                      # dq dk dv dpair
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},                      # Δ o ms ls
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},          # q k v pair kpad_mask
         Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),                                    # workspace, bytes, stream
        d, op, devptr(sinks), devptr(ds), devptr(dq), devptr(dk), devptr(dv), devptr(dp), devptr(Δ), devptr(o), devptr(ms),
        devptr(ls), devptr(q), devptr(k), devptr(v), devptr(pair), devptr(kpad_mask), devptr(ws), nbytes, hipstream())
    check(st, q, k, v)
    return dq, dk, dv, dp, ds
end

"""
    flash_attention_sinks(q, k, v, sinks, pair=nothing; causal, window=(-1, -1), kpad_mask=nothing)

Flash Attention with learned per-head attention sinks on the HIP kernels (gpt-oss): `sinks::ROCVector{Float32}` holds one logit per
query head in the units of the scaled logits; each row's softmax gets that extra column, whose share of the row is dropped.  `window`
as for `local_flash_attention`.  Differentiable w.r.t. q, k, v, sinks (and pair) through the ChainRules rule below.
"""
flash_attention_sinks(q, k, v, sinks, pair = nothing; causal::Bool, window::Tuple{Integer, Integer} = (-1, -1), kpad_mask = nothing) =
    flash_attention_sinks_fwd(q, k, v, sinks, pair; causal, window, kpad_mask)[1]

# the shape of local_flash_attention's rule, plus a tangent for the sinks
function NNop.CRC.rrule(::typeof(flash_attention_sinks), q, k, v, sinks, pair = nothing;
                                   causal::Bool, window::Tuple{Integer, Integer} = (-1, -1), kpad_mask = nothing)
    o, ms, ls = flash_attention_sinks_fwd(q, k, v, sinks, pair; causal, window, kpad_mask)
    function flash_attention_sinks_pullback(Δ)
        dq, dk, dv, dp, ds = flash_attention_sinks_bwd(_to_roc(NNop.CRC.unthunk(Δ), o), o, ms, ls, q, k, v, sinks, pair;
                                                       causal, window, kpad_mask)
        return NNop.CRC.NoTangent(), dq, dk, dv, ds, isnothing(pair) ? NNop.CRC.NoTangent() : dp
    end
    return o, flash_attention_sinks_pullback
end

# ---- logit soft-capping (include/nnop_hip.h: nnop_fa_fwd_softcap / nnop_fa_bwd_softcap) ---------------------------------------------
# The scaled scores become softcap * tanh(scale * q.k / softcap) (Gemma-2: 50, Grok-1: 30) before the pair bias is added and the masks
# and the softmax apply; the bias and the sinks are not capped.  fp32 arithmetic for every element type.  `window = nothing`: no options
# (a NULL nnop_fa_opts); `sinks = nothing`: no sinks (NULL); `softcap = 0`: no cap -- the library then runs exactly the sinks call.
_opts_ref(window::Nothing) = nothing
_opts_ref(window::Tuple{Integer, Integer}) = Ref(FaOpts(window))
_opts_ptr(op::Nothing) = Ptr{FaOpts}(C_NULL)
_opts_ptr(op::Ref{FaOpts}) = Base.unsafe_convert(Ptr{FaOpts}, op)

function softcap_flash_attention_fwd(
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4}, pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing, window::Union{Nothing,Tuple{Integer, Integer}} = nothing,
    sinks::Union{Nothing,ROCVector{Float32}} = nothing, softcap::Real,
) where T <: HipFloat
    check_abi()
    isnothing(sinks) || length(sinks) == size(q, 3) ||
        error("sinks must have one entry per query head ($(size(q, 3))), got $(length(sinks))")
    d = Ref(desc(q, k, v, causal))
    op = _opts_ref(window)
    o  = similar(q)
    ms = ROCArray{T}(undef, size(q, 2), size(q, 3), size(q, 4))
    ls = similar(ms)
    st = GC.@preserve op o ms ls q k v sinks pair kpad_mask ccall((:nnop_fa_fwd_softcap, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{FaOpts}, Ptr{Cvoid}, Cfloat,                        # sinks softcap
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, _opts_ptr(op), devptr(sinks), Cfloat(softcap), devptr(o), devptr(ms), devptr(ls), devptr(q), devptr(k), devptr(v),
        devptr(pair), devptr(kpad_mask), hipstream())
    check(st, q, k, v)
    return o, ms, ls
end

function softcap_flash_attention_bwd(
    Δ::ROCArray{T,4}, o::ROCArray{T,4}, ms::ROCArray{T,3}, ls::ROCArray{T,3},
    q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4}, pair::Union{Nothing,ROCArray{T,4}} = nothing;
    causal::Bool, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing, window::Union{Nothing,Tuple{Integer, Integer}} = nothing,
    sinks::Union{Nothing,ROCVector{Float32}} = nothing, softcap::Real,
) where T <: HipFloat
    d = Ref(desc(q, k, v, causal))
    op = _opts_ref(window)
    # a cap needs no more scratch than the plain backward (with a pair bias it always takes the direct path)
    nbytes = ccall((:nnop_fa_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{FaDesc},), d)
    nbytes == 0 && error("libnnop_hip: invalid attention descriptor")
    dq, dk, dv = similar(q), similar(k), similar(v)
    dp = isnothing(pair) ? nothing : similar(pair)
    ds = isnothing(sinks) ? nothing : similar(sinks)
    ws = ROCArray{UInt8}(undef, nbytes)
    st = GC.@preserve op dq dk dv dp ds Δ o ms ls q k v sinks pair kpad_mask ws ccall((:nnop_fa_bwd_softcap, libnnop()), Cint,
        (Ptr{FaDesc}, Ptr{FaOpts}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat,            # sinks dsinks softcap
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},                      # dq dk dv dpair
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},                      # Δ o ms ls
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},          # q k v pair kpad_mask
         Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),                                    # workspace, bytes, stream
        d, _opts_ptr(op), devptr(sinks), devptr(ds), Cfloat(softcap), devptr(dq), devptr(dk), devptr(dv), devptr(dp), devptr(Δ),
        devptr(o), devptr(ms), devptr(ls), devptr(q), devptr(k), devptr(v), devptr(pair), devptr(kpad_mask), devptr(ws), nbytes,
        hipstream())
    check(st, q, k, v)
    return dq, dk, dv, dp, ds
end

"""
    softcap_flash_attention(q, k, v, pair=nothing; causal, kpad_mask=nothing, window=nothing, sinks=nothing, softcap)

Flash Attention with logit soft-capping on the HIP kernels: the scaled scores become `softcap * tanh(scale * q.k / softcap)` before the
pair bias, the masks and the softmax (Gemma-2: 50, Grok-1: 30).  `window` as for `local_flash_attention`, `sinks` as for
`flash_attention_sinks`; neither the bias nor the sinks are capped.  Differentiable w.r.t. q, k, v and pair through the ChainRules
rule below.  NOT w.r.t. `sinks`: they are a keyword here, and ChainRules gives keyword arguments no tangent, so automatic
differentiation treats them as constants.  To train sinks under a cap call `softcap_flash_attention_fwd` and
`softcap_flash_attention_bwd` yourself: the fifth value the latter returns is `dsinks`.
"""
softcap_flash_attention(q, k, v, pair = nothing; causal::Bool, kpad_mask = nothing, window = nothing, sinks = nothing, softcap::Real) =
    softcap_flash_attention_fwd(q, k, v, pair; causal, kpad_mask, window, sinks, softcap)[1]

# the shape of local_flash_attention's rule: no tangent for the cap, the window or the mask.  ChainRules gives keyword arguments no
# tangent, so `sinks` gets none here: softcap_flash_attention_bwd returns their gradient for a caller that trains them under a cap
function NNop.CRC.rrule(::typeof(softcap_flash_attention), q, k, v, pair = nothing;
                                   causal::Bool, kpad_mask = nothing, window = nothing, sinks = nothing, softcap::Real)
    o, ms, ls = softcap_flash_attention_fwd(q, k, v, pair; causal, kpad_mask, window, sinks, softcap)
    function softcap_flash_attention_pullback(Δ)
        dq, dk, dv, dp, _ = softcap_flash_attention_bwd(_to_roc(NNop.CRC.unthunk(Δ), o), o, ms, ls, q, k, v, pair;
                                                        causal, kpad_mask, window, sinks, softcap)
        return NNop.CRC.NoTangent(), dq, dk, dv, isnothing(pair) ? NNop.CRC.NoTangent() : dp
    end
    return o, softcap_flash_attention_pullback
end

# ---- several devices (include/nnop_hip.h: nnop_fa_shards, ABI version 6) -------------------------------------------------------------
# The reference has no multi-GPU code; (batch, kv-head) slices are independent in forward and backward (src/attention.jl:27-28,33;
# src/attention_bwd.jl:28-29,34), so the H x B axis shards with pointer offsets and NO data-path collective.  nnop_fa_shards gives
# rank g of `world` its contiguous unit range as <= 3 dense rectangles; each is a problem of its own for _flash_attention at the
# element offsets it reports.  Two ways to use it from Julia:
#   * one process per GPU (MPI.jl / Distributed.jl): call `flash_attention_shard(q, k, v, world, rank; causal)` on the rank's device
#     with the FULL arrays resident there, or with the rank's slices and world = 1;
#   * one process driving all GPUs (below): `flash_attention_multi(qs, ks, vs; causal)` with one (q, k, v) replica or slice per device
#     -- a task per device, each on its own task-local HIP stream (AMDGPU.device! is task-local), joined at the end.
# struct nnop_fa_shard
struct FaShard
    desc::FaDesc
    b0::Int32; b1::Int32; kh0::Int32; kh1::Int32
    q_off::UInt64; kv_off::UInt64; row_off::UInt64; mask_off::UInt64; pair_off::Int64
end

function fa_shards(q, k, v, causal::Bool, world::Integer, rank::Integer)
    out = Vector{FaShard}(undef, 3)
    n = ccall((:nnop_fa_shards, libnnop()), Cint, (Ptr{FaDesc}, Cint, Cint, Ptr{FaShard}), Ref(desc(q, k, v, causal)), world, rank, out)
    n < 0 && check(n, q, k, v)
    return out[1:n]
end

# Rank `rank` (0-based) of `world`: its rectangles of o, ms, ls are written in place into full-size outputs (the rest is left
# untouched: another rank's).  No copies: `view`s of the (E, L, H, B) arrays over head / batch ranges are the rectangles.
function flash_attention_shard!(o, ms, ls, q::ROCArray{T,4}, k::ROCArray{T,4}, v::ROCArray{T,4}, world::Integer, rank::Integer;
                                causal::Bool, kpad_mask::Union{Nothing,ROCMatrix{Bool}} = nothing) where T <: HipFloat
    rep = size(q, 3) ÷ size(k, 3)
    for s in fa_shards(q, k, v, causal, world, rank)
        b, h, qh = (s.b0 + 1):s.b1, (s.kh0 + 1):s.kh1, (s.kh0 * rep + 1):(s.kh1 * rep)
        # the four views are dense (whole batches, or a head range of one batch): the library sees plain [B'][H'][L][E] problems
        oo, mm, ll = NNop._flash_attention(q[:, :, qh, b], k[:, :, h, b], v[:, :, h, b]; causal,
                                           kpad_mask = isnothing(kpad_mask) ? nothing : kpad_mask[:, b])
        o[:, :, qh, b] .= oo; ms[:, qh, b] .= mm; ls[:, qh, b] .= ll
    end
    return o, ms, ls
end
# (The indexing above copies the rectangle -- the simple, allocation-tolerant form.  The zero-copy form passes
#  devptr(q) + s.q_off * sizeof(T), devptr(k) + s.kv_off * sizeof(T), ... with Ref(s.desc) straight to :nnop_fa_fwd / :nnop_fa_bwd,
#  exactly as _flash_attention does with offset 0; the offsets are multiples of L * E elements, so 16-byte alignment is kept.
#  A pair bias goes the same way, devptr(pair) + s.pair_off * sizeof(T): that offset is any multiple of the element size, which is
#  all the library asks of pair / dpair.)

# One process, all devices: qs[g], ks[g], vs[g] live on device g (replicas or batch slices of the global problem).
function flash_attention_multi(qs::Vector, ks::Vector, vs::Vector; causal::Bool)
    world = length(qs)
    tasks = map(1:world) do g
        Threads.@spawn begin
            AMDGPU.device!(AMDGPU.devices()[g])                 # task-local: this task's arrays and stream live on device g
            o, ms, ls = similar(qs[g]), ROCArray{eltype(qs[g])}(undef, size(qs[g])[2:4]...), ROCArray{eltype(qs[g])}(undef, size(qs[g])[2:4]...)
            flash_attention_shard!(o, ms, ls, qs[g], ks[g], vs[g], world, g - 1; causal)
            AMDGPU.synchronize()
            (o, ms, ls)
        end
    end
    return fetch.(tasks)
end

# struct nnop_rope_desc (include/nnop_hip.h)
struct RopeDesc
    dtype::Int32; cs_dtype::Int32; dim::Int32; seq::Int32; qh::Int32; kh::Int32; batch::Int32
end

# src/rope/llama_rope.jl:69-89.  `llama_rope`, `∇llama_rope` and the rrule (:67, :91-98) call this generically.
# One pass, out of place: replaces copy(q), copy(k) + the in-place kernel (:75-86).
function NNop._llama_rope(
    q::ROCArray{T,4}, k::ROCArray{T,4}, cos::ROCArray{C,3}, sin::ROCArray{C,3}; bwd::Bool,
) where {T <: HipFloat, C <: HipFloat}
    head_dim, q_seq, q_heads, batch = size(q)
    @assert size(k, 1) == head_dim "Head dimension mismatch"    # :72
    @assert size(k, 2) == q_seq && size(k, 4) == batch          # :73
    @assert size(cos) == size(sin) == (head_dim, q_seq, batch)
    d = Ref(RopeDesc(nnop_dtype(T), nnop_dtype(C), head_dim, q_seq, q_heads, size(k, 3), batch))
    qo, ko = similar(q), similar(k)
    st = GC.@preserve qo ko q k cos sin ccall((:nnop_llama_rope, libnnop()), Cint,
        (Ptr{RopeDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}),
        d, devptr(qo), devptr(ko), devptr(q), devptr(k), devptr(cos), devptr(sin), bwd ? -1f0 : 1f0, hipstream())
    st == 0 || error("libnnop_hip: " * unsafe_string(ccall((:nnop_strerror, libnnop()), Cstring, (Cint,), st)))
    return qo, ko
end

# struct nnop_softmax_desc (include/nnop_hip.h)
struct SoftmaxDesc
    dtype::Int32; n::Int32; batch::Int64
end

# src/softmax.jl:60-68.  The rrule (:82-86) calls online_softmax / ∇online_softmax generically.
function NNop.online_softmax(x::ROCMatrix{T}) where T <: HipFloat
    y = similar(x)
    d = Ref(SoftmaxDesc(nnop_dtype(T), size(x, 1), size(x, 2)))
    st = GC.@preserve y x ccall((:nnop_online_softmax, libnnop()), Cint, (Ptr{SoftmaxDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(y), devptr(x), hipstream())
    st == 0 || error("libnnop_hip: " * unsafe_string(ccall((:nnop_strerror, libnnop()), Cstring, (Cint,), st)))
    return y
end

# src/softmax.jl:70-80: the two broadcasts + reduction fused into one pass (first derivatives only, like the
# reference's fast path :75-78; under nested differentiation the generic method still applies).
function NNop.∇online_softmax(Δ::ROCMatrix{T}, y::ROCMatrix{T}) where T <: HipFloat
    NNop.within_gradient(y) && return invoke(NNop.∇online_softmax, Tuple{AbstractArray, AbstractArray}, Δ, y)
    dx = similar(y)
    d = Ref(SoftmaxDesc(nnop_dtype(T), size(y, 1), size(y, 2)))
    st = GC.@preserve dx Δ y ccall((:nnop_online_softmax_bwd, libnnop()), Cint,
        (Ptr{SoftmaxDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), d, devptr(dx), devptr(Δ), devptr(y), hipstream())
    st == 0 || error("libnnop_hip: " * unsafe_string(ccall((:nnop_strerror, libnnop()), Cstring, (Cint,), st)))
    return dx
end

# struct nnop_norm_desc (include/nnop_hip.h)
struct NormDesc
    dtype::Int32; w_dtype::Int32; emb::Int32; reserved::Int32; n::Int64
end
normdesc(x, w) = Ref(NormDesc(nnop_dtype(eltype(x)), nnop_dtype(eltype(w)), size(x, 1), 0, size(x, 2)))
ok(st) = st == 0 || error("libnnop_hip: " * unsafe_string(ccall((:nnop_strerror, libnnop()), Cstring, (Cint,), st)))

# src/rms_norm.jl:117-137 (the public rms_norm and the rrule, :171-185, call these generically)
function NNop._rms_norm(x::ROCMatrix{T}, w::ROCVector{W}; ϵ::Float32, offset::Float32 = 0f0) where {T <: HipFloat, W <: HipFloat}
    @assert size(x, 1) == length(w)
    y = similar(x); rms = ROCArray{Float32}(undef, size(x, 2))
    ok(GC.@preserve y rms x w ccall((:nnop_rms_norm, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Cfloat, Ptr{Cvoid}),
        normdesc(x, w), devptr(y), devptr(rms), devptr(x), devptr(w), offset, ϵ, hipstream()))
    return y, rms
end

# src/rms_norm.jl:139-169: dw comes back already summed over rows (Float32, :146)
function NNop.∇rms_norm(Δ::ROCMatrix{T}, rms::ROCVector{Float32}, x::ROCMatrix{T}, w::ROCVector{W};
                        offset::Float32) where {T <: HipFloat, W <: HipFloat}
    d = normdesc(x, w)
    dx = similar(x); dw = ROCArray{Float32}(undef, size(x, 1))
    nbytes = ccall((:nnop_norm_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{NormDesc}, Cint), d, 0)
    ws = ROCArray{UInt8}(undef, nbytes)
    ok(GC.@preserve dx dw Δ rms x w ws ccall((:nnop_rms_norm_bwd, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        d, devptr(dx), devptr(dw), devptr(Δ), devptr(rms), devptr(x), devptr(w), offset, devptr(ws), nbytes, hipstream()))
    return dx, dw
end

# src/layer_norm.jl:150-170
function NNop._layer_norm(x::ROCMatrix{T}, w::ROCVector{W}, b::ROCVector{W}; ϵ::Float32 = 1f-6) where {T <: HipFloat, W <: HipFloat}
    y = similar(x); μ = ROCArray{Float32}(undef, size(x, 2)); Σ = similar(μ)
    ok(GC.@preserve y μ Σ x w b ccall((:nnop_layer_norm, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}),
        normdesc(x, w), devptr(y), devptr(μ), devptr(Σ), devptr(x), devptr(w), devptr(b), ϵ, hipstream()))
    return y, μ, Σ
end

# src/layer_norm.jl:172-204: dw, db in eltype(w) (:179-180), already summed over rows
function NNop.∇layer_norm(Δ::ROCMatrix{T}, μ::ROCVector{Float32}, Σ::ROCVector{Float32}, x::ROCMatrix{T},
                          w::ROCVector{W}, b::ROCVector{W}) where {T <: HipFloat, W <: HipFloat}
    d = normdesc(x, w)
    dx = similar(x); dw = similar(w); db = similar(b)
    nbytes = ccall((:nnop_norm_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{NormDesc}, Cint), d, 1)
    ws = ROCArray{UInt8}(undef, nbytes)
    ok(GC.@preserve dx dw db Δ μ Σ x w ws ccall((:nnop_layer_norm_bwd, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        d, devptr(dx), devptr(dw), devptr(db), devptr(Δ), devptr(μ), devptr(Σ), devptr(x), devptr(w), devptr(ws), nbytes, hipstream()))
    return dx, dw, db
end


# ---- residual add fused into the norms (include/nnop_hip.h: nnop_add_rms_norm and siblings; no counterpart in the reference) -----------
# h = x + residual (one rounding to T) is written out and normalised in the same pass; the pullbacks take the cotangents of y and of h
# and return ONE gradient, that of x and of residual alike.  `h_out` may be `x` or `residual` (in-place residual stream), `dx_out`
# may be `dh`; the differentiable forms below never write in place.
function add_rms_norm_fwd(x::ROCMatrix{T}, residual::ROCMatrix{T}, w::ROCVector{W}; ϵ::Float32 = 1f-6, offset::Float32 = 0f0,
                          h_out::ROCMatrix{T} = similar(x)) where {T <: HipFloat, W <: HipFloat}
    @assert size(x, 1) == length(w)
    @assert size(residual) == size(x) && size(h_out) == size(x)
    y = similar(x); rms = ROCArray{Float32}(undef, size(x, 2))
    ok(GC.@preserve y h_out rms x residual w ccall((:nnop_add_rms_norm, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Cfloat, Ptr{Cvoid}),
        normdesc(x, w), devptr(y), devptr(h_out), devptr(rms), devptr(x), devptr(residual), devptr(w), offset, ϵ, hipstream()))
    return y, h_out, rms
end

# dh: cotangent of h, or nothing (then exactly NNop.∇rms_norm on h)
function add_rms_norm_bwd(Δ::ROCMatrix{T}, dh::Union{ROCMatrix{T}, Nothing}, rms::ROCVector{Float32}, h::ROCMatrix{T}, w::ROCVector{W};
                          offset::Float32 = 0f0, dx_out::ROCMatrix{T} = similar(h)) where {T <: HipFloat, W <: HipFloat}
    d = normdesc(h, w)
    dw = ROCArray{Float32}(undef, size(h, 1))
    nbytes = ccall((:nnop_norm_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{NormDesc}, Cint), d, 0)
    ws = ROCArray{UInt8}(undef, nbytes)
    ok(GC.@preserve dx_out dw Δ dh rms h w ws ccall((:nnop_add_rms_norm_bwd, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        d, devptr(dx_out), devptr(dw), devptr(Δ), devptr(dh), devptr(rms), devptr(h), devptr(w), offset, devptr(ws), nbytes, hipstream()))
    return dx_out, dw
end

function add_layer_norm_fwd(x::ROCMatrix{T}, residual::ROCMatrix{T}, w::ROCVector{W}, b::ROCVector{W}; ϵ::Float32 = 1f-6,
                            h_out::ROCMatrix{T} = similar(x)) where {T <: HipFloat, W <: HipFloat}
    @assert size(x, 1) == length(w) == length(b)
    @assert size(residual) == size(x) && size(h_out) == size(x)
    y = similar(x); μ = ROCArray{Float32}(undef, size(x, 2)); Σ = similar(μ)
    ok(GC.@preserve y h_out μ Σ x residual w b ccall((:nnop_add_layer_norm, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}),
        normdesc(x, w), devptr(y), devptr(h_out), devptr(μ), devptr(Σ), devptr(x), devptr(residual), devptr(w), devptr(b), ϵ, hipstream()))
    return y, h_out, μ, Σ
end

function add_layer_norm_bwd(Δ::ROCMatrix{T}, dh::Union{ROCMatrix{T}, Nothing}, μ::ROCVector{Float32}, Σ::ROCVector{Float32},
                            h::ROCMatrix{T}, w::ROCVector{W}; dx_out::ROCMatrix{T} = similar(h)) where {T <: HipFloat, W <: HipFloat}
    d = normdesc(h, w)
    dw = similar(w); db = similar(w)
    nbytes = ccall((:nnop_norm_bwd_workspace_bytes, libnnop()), Csize_t, (Ptr{NormDesc}, Cint), d, 1)
    ws = ROCArray{UInt8}(undef, nbytes)
    ok(GC.@preserve dx_out dw db Δ dh μ Σ h w ws ccall((:nnop_add_layer_norm_bwd, libnnop()), Cint,
        (Ptr{NormDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        d, devptr(dx_out), devptr(dw), devptr(db), devptr(Δ), devptr(dh), devptr(μ), devptr(Σ), devptr(h), devptr(w), devptr(ws), nbytes,
        hipstream()))
    return dx_out, dw, db
end

"""
    add_rms_norm(x, residual, w; ϵ=1f-6, offset=0f0) -> (y, h)
    add_layer_norm(x, residual, w, b; ϵ=1f-6) -> (y, h)

`h = x + residual` and `y = rms_norm(h, w; ϵ, offset)` / `layer_norm(h, w, b; ϵ)` in one pass over memory (the pre-norm transformer block's
add and norm).  Differentiable through the ChainRules rules below; the tangents of `x` and of `residual` are the same array.
"""
add_rms_norm(x, residual, w; ϵ::Float32 = 1f-6, offset::Float32 = 0f0) = add_rms_norm_fwd(x, residual, w; ϵ, offset)[1:2]
add_layer_norm(x, residual, w, b; ϵ::Float32 = 1f-6) = add_layer_norm_fwd(x, residual, w, b; ϵ)[1:2]

# a cotangent that is a ChainRules zero (an output the caller never used) reaches the library as a NULL pointer, not as zeros
_cot(Δ, like) = Δ isa NNop.CRC.AbstractZero ? nothing : _to_roc(NNop.CRC.unthunk(Δ), like)

function NNop.CRC.rrule(::typeof(add_rms_norm), x, residual, w; ϵ::Float32 = 1f-6, offset::Float32 = 0f0)
    y, h, rms = add_rms_norm_fwd(x, residual, w; ϵ, offset)
    function add_rms_norm_pullback(Δ)
        dy, dh = _cot(Δ[1], y), _cot(Δ[2], h)
        if isnothing(dy)                                  # only h was used: the add alone
            dx = isnothing(dh) ? NNop.CRC.ZeroTangent() : dh
            return NNop.CRC.NoTangent(), dx, dx, NNop.CRC.ZeroTangent()
        end
        dx, dw = add_rms_norm_bwd(dy, dh, rms, h, w; offset)
        return NNop.CRC.NoTangent(), dx, dx, eltype(w) === Float32 ? dw : eltype(w).(dw)
    end
    return (y, h), add_rms_norm_pullback
end

function NNop.CRC.rrule(::typeof(add_layer_norm), x, residual, w, b; ϵ::Float32 = 1f-6)
    y, h, μ, Σ = add_layer_norm_fwd(x, residual, w, b; ϵ)
    function add_layer_norm_pullback(Δ)
        dy, dh = _cot(Δ[1], y), _cot(Δ[2], h)
        if isnothing(dy)
            dx = isnothing(dh) ? NNop.CRC.ZeroTangent() : dh
            return NNop.CRC.NoTangent(), dx, dx, NNop.CRC.ZeroTangent(), NNop.CRC.ZeroTangent()
        end
        dx, dw, db = add_layer_norm_bwd(dy, dh, μ, Σ, h, w)
        return NNop.CRC.NoTangent(), dx, dx, dw, db
    end
    return (y, h), add_layer_norm_pullback
end


# ---- gated MLP activations (include/nnop_hip.h: nnop_glu / nnop_glu_bwd; no counterpart in the reference) -----------------------------
# y = act(gate) .* up in one pass; the pullback recomputes act and its derivative from gate and up.  Matrices are (n, rows) -- the same
# memory as the header's [rows][n].  `gate` and `up` may be two dense matrices or the two halves `view(gu, 1:n, :)`, `view(gu, n+1:2n, :)`
# of one fused projection (one common column stride `ld`, no copy); `glu(gu; layout = :interleaved)` takes gate = gu[1:2:end, :],
# up = gu[2:2:end, :] (gpt-oss).
struct GluDesc
    dtype::Int32; act::Int32; layout::Int32; reserved::Int32
    rows::Int64; n::Int64; ld::Int64
    alpha::Float32; limit::Float32
end
const GLU_ACTS = (silu = Int32(0), gelu_tanh = Int32(1), gelu_erf = Int32(2), swiglu_oai = Int32(3))
const RowsOf{T} = Union{ROCMatrix{T}, SubArray{T, 2, <:ROCMatrix{T}, <:Tuple{UnitRange{Int}, Base.Slice}}}
_ld(x) = stride(x, 2)
gludesc(x, act::Symbol, layout, n, ld, alpha, limit) =
    Ref(GluDesc(nnop_dtype(eltype(x)), GLU_ACTS[act], layout, 0, size(x, 2), n, ld, alpha, limit))

function glu_fwd(gate::RowsOf{T}, up::RowsOf{T}; act::Symbol = :silu, alpha::Float32 = 1.702f0, limit::Float32 = 7f0,
                 y::ROCMatrix{T} = ROCArray{T}(undef, size(gate))) where {T <: HipFloat}
    @assert size(gate) == size(up) == size(y) && _ld(gate) == _ld(up)
    d = gludesc(gate, act, 0, size(gate, 1), size(gate, 2) == 1 ? size(gate, 1) : _ld(gate), alpha, limit)
    ok(GC.@preserve y gate up ccall((:nnop_glu, libnnop()), Cint,
        (Ptr{GluDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(y), devptr(gate), devptr(up), hipstream()))
    return y
end

# dgate / dup: laid out like gate / up (they may BE gate / up: in place)
function glu_bwd(Δ::ROCMatrix{T}, gate::RowsOf{T}, up::RowsOf{T}; act::Symbol = :silu, alpha::Float32 = 1.702f0, limit::Float32 = 7f0,
                 dgate::RowsOf{T} = ROCArray{T}(undef, size(gate)), dup::RowsOf{T} = ROCArray{T}(undef, size(up))) where {T <: HipFloat}
    @assert size(gate) == size(up) == size(Δ) && _ld(gate) == _ld(up)
    if _ld(dgate) != _ld(gate) || _ld(dup) != _ld(gate)      # fresh dense gradients for strided inputs: dense copies of the inputs
        gate, up = ROCArray(gate), ROCArray(up)
    end
    d = gludesc(gate, act, 0, size(gate, 1), size(gate, 2) == 1 ? size(gate, 1) : _ld(gate), alpha, limit)
    ok(GC.@preserve dgate dup Δ gate up ccall((:nnop_glu_bwd, libnnop()), Cint,
        (Ptr{GluDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(dgate), devptr(dup), devptr(Δ), devptr(gate), devptr(up), hipstream()))
    return dgate, dup
end

# one fused projection gu (2n, rows)
function glu_fwd(gu::ROCMatrix{T}; layout::Symbol = :halves, kw...) where {T <: HipFloat}
    n = size(gu, 1) ÷ 2
    @assert size(gu, 1) == 2n && layout in (:halves, :interleaved)
    layout === :halves && return glu_fwd(view(gu, 1:n, :), view(gu, n+1:2n, :); kw...)
    act = get(kw, :act, :silu); alpha = get(kw, :alpha, 1.702f0); limit = get(kw, :limit, 7f0)
    y = ROCArray{T}(undef, n, size(gu, 2))
    d = gludesc(gu, act, 1, n, 2n, alpha, limit)
    ok(GC.@preserve y gu ccall((:nnop_glu, libnnop()), Cint,
        (Ptr{GluDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(y), devptr(gu), devptr(nothing), hipstream()))
    return y
end

function glu_bwd(Δ::ROCMatrix{T}, gu::ROCMatrix{T}; layout::Symbol = :halves, dgu::ROCMatrix{T} = similar(gu), kw...) where {T <: HipFloat}
    n = size(gu, 1) ÷ 2
    @assert size(gu, 1) == 2n && size(Δ) == (n, size(gu, 2)) && size(dgu) == size(gu)
    if layout === :halves
        glu_bwd(Δ, view(gu, 1:n, :), view(gu, n+1:2n, :); dgate = view(dgu, 1:n, :), dup = view(dgu, n+1:2n, :), kw...)
        return dgu
    end
    act = get(kw, :act, :silu); alpha = get(kw, :alpha, 1.702f0); limit = get(kw, :limit, 7f0)
    d = gludesc(gu, act, 1, n, 2n, alpha, limit)
    ok(GC.@preserve dgu Δ gu ccall((:nnop_glu_bwd, libnnop()), Cint,
        (Ptr{GluDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(dgu), devptr(nothing), devptr(Δ), devptr(gu), devptr(nothing), hipstream()))
    return dgu
end

"""
    glu(gate, up; act=:silu, alpha=1.702f0, limit=7f0) -> y
    glu(gu; layout=:halves, act=:silu, ...) -> y

`y = act(gate) .* up`: SwiGLU (`:silu`), GeGLU (`:gelu_tanh`, `:gelu_erf`) and the clamped gpt-oss SwiGLU (`:swiglu_oai`,
`min(g, limit) * σ(alpha * min(g, limit)) * (clamp(u, -limit, limit) + 1)`).  Differentiable through the ChainRules rules below, which keep
only `gate` and `up` (or `gu`).
"""
glu(gate, up; kw...) = glu_fwd(gate, up; kw...)
glu(gu; kw...) = glu_fwd(gu; kw...)

function NNop.CRC.rrule(::typeof(glu), gate, up; kw...)
    y = glu_fwd(gate, up; kw...)
    glu_pullback(Δ) = (NNop.CRC.NoTangent(), glu_bwd(_to_roc(NNop.CRC.unthunk(Δ), y), gate, up; kw...)...)
    return y, glu_pullback
end

function NNop.CRC.rrule(::typeof(glu), gu; kw...)
    y = glu_fwd(gu; kw...)
    glu_packed_pullback(Δ) = (NNop.CRC.NoTangent(), glu_bwd(_to_roc(NNop.CRC.unthunk(Δ), y), gu; kw...))
    return y, glu_packed_pullback
end


# ---- cross-entropy over the classes (include/nnop_hip.h: nnop_cross_entropy / nnop_cross_entropy_bwd; no counterpart in the reference) ---
# logits (n, rows) -- the same memory as the header's [rows][n] -- or a view of the first n rows of a padded (ld, rows) matrix; targets
# are Julia class indices 1..n (index_base = 1), Int32 or Int64; `ignore_index` is compared with the stored value.  Forward: one pass,
# per-token losses and log-sum-exp in Float32; pullback: one pass, recomputing the probabilities from lse.
struct XentDesc
    dtype::Int32; index_bytes::Int32
    rows::Int64; n::Int64
    ld::Int64; ld_grad::Int64
    ignore_index::Int64
    index_base::Int32; reserved::Int32
    label_smoothing::Float32; z_loss::Float32; softcap::Float32; reserved_f::Float32
end
xentdesc(x, dx, targets, ignore_index, label_smoothing, z_loss, softcap) =
    Ref(XentDesc(nnop_dtype(eltype(x)), sizeof(eltype(targets)), size(x, 2), size(x, 1), size(x, 2) == 1 ? size(x, 1) : _ld(x),
                 size(dx, 2) == 1 ? size(dx, 1) : _ld(dx), ignore_index, 1, 0, label_smoothing, z_loss, softcap, 0f0))

# -> (loss, lse), Float32 vectors of length rows
function cross_entropy_fwd(logits::RowsOf{T}, targets::ROCVector{I}; ignore_index::Integer = -100, label_smoothing::Real = 0,
                           z_loss::Real = 0, softcap::Real = 0) where {T <: HipFloat, I <: Union{Int32, Int64}}
    @assert length(targets) == size(logits, 2)
    loss = ROCArray{Float32}(undef, size(logits, 2)); lse = similar(loss)
    d = xentdesc(logits, logits, targets, ignore_index, label_smoothing, z_loss, softcap)
    ok(GC.@preserve loss lse logits targets ccall((:nnop_cross_entropy, libnnop()), Cint,
        (Ptr{XentDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(loss), devptr(lse), devptr(logits), devptr(targets), hipstream()))
    return loss, lse
end

# dlogits: laid out like a dense matrix by default; it may BE logits (in place)
function cross_entropy_bwd(Δ::ROCVector{Float32}, lse::ROCVector{Float32}, logits::RowsOf{T}, targets::ROCVector{I};
                           ignore_index::Integer = -100, label_smoothing::Real = 0, z_loss::Real = 0, softcap::Real = 0,
                           dlogits::RowsOf{T} = ROCArray{T}(undef, size(logits))) where {T <: HipFloat, I <: Union{Int32, Int64}}
    @assert length(targets) == length(Δ) == length(lse) == size(logits, 2) && size(dlogits) == size(logits)
    d = xentdesc(logits, dlogits, targets, ignore_index, label_smoothing, z_loss, softcap)
    ok(GC.@preserve dlogits Δ lse logits targets ccall((:nnop_cross_entropy_bwd, libnnop()), Cint,
        (Ptr{XentDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(dlogits), devptr(Δ), devptr(lse), devptr(logits), devptr(targets), hipstream()))
    return dlogits
end

"""
    cross_entropy(logits, targets; ignore_index=-100, label_smoothing=0, z_loss=0, softcap=0) -> loss

Per-token cross-entropy losses (a Float32 vector of length `size(logits, 2)`) of `logits` (n, tokens) against the classes `targets`
in 1..n; tokens whose target equals `ignore_index` have loss 0 and no gradient.  `softcap = c` caps the logits with `c * tanh(x / c)`
(Gemma-2: 30), `z_loss` adds `z_loss * lse^2`, `label_smoothing` is PyTorch's.  Reduce with `sum` / `mean` as the trainer needs.
"""
cross_entropy(logits, targets; kw...) = cross_entropy_fwd(logits, targets; kw...)[1]

function NNop.CRC.rrule(::typeof(cross_entropy), logits, targets; kw...)
    loss, lse = cross_entropy_fwd(logits, targets; kw...)
    cross_entropy_pullback(Δ) = (NNop.CRC.NoTangent(), cross_entropy_bwd(_to_roc(NNop.CRC.unthunk(Δ), loss), lse, logits, targets; kw...),
                                 NNop.CRC.NoTangent())
    return loss, cross_entropy_pullback
end


# ---- fused QK-norm + RoPE (include/nnop_hip_ext.h: the SECOND library, libnnop_hip_ext.so; no counterpart in the reference) ------------
# Operators beyond the NNop drop-in boundary live in a library of their own with its own ABI version.  It is opened once with dlopen
# and its functions are called through dlsym pointers, so the calls into the two libraries cannot be mixed up; status codes are
# nnop_status, turned into text by the main library (`ok`).  Point ENV["NNOP_HIP_EXT_LIB"] at libnnop_hip_ext.so.
import Libdl

const EXT_ABI_VERSION = 1
const EXT_LIB = Ref{Ptr{Cvoid}}(C_NULL)
function libnnop_ext()
    if EXT_LIB[] == C_NULL
        h = Libdl.dlopen(get(ENV, "NNOP_HIP_EXT_LIB", "libnnop_hip_ext.so"))
        v = ccall(Libdl.dlsym(h, :nnop_ext_abi_version), Cint, ())
        v == EXT_ABI_VERSION || error("libnnop_hip_ext has ext-ABI version $v, this extension needs $EXT_ABI_VERSION")
        EXT_LIB[] = h
    end
    return EXT_LIB[]
end

# struct nnop_qknr_desc (include/nnop_hip_ext.h), 48 bytes
struct QknrDesc
    dtype::Int32; w_dtype::Int32; cs_dtype::Int32
    dim::Int32; seq::Int32; qh::Int32; kh::Int32; batch::Int32
    eps::Float32; offset::Float32
    reserved::NTuple{2, Int32}
end
function qknrdesc(q::ROCArray{T,4}, k::ROCArray{T,4}, wq::ROCVector{W}, wk::ROCVector{W}, cos::ROCArray{C,3}, sin::ROCArray{C,3},
                  ϵ, offset) where {T, W, C}
    head_dim, seq, q_heads, batch = size(q)
    @assert size(k, 1) == head_dim && size(k, 2) == seq && size(k, 4) == batch
    @assert length(wq) == length(wk) == head_dim
    @assert size(cos) == size(sin) == (head_dim, seq, batch)
    return Ref(QknrDesc(nnop_dtype(T), nnop_dtype(W), nnop_dtype(C), head_dim, seq, q_heads, size(k, 3), batch, ϵ, offset, (Int32(0), Int32(0))))
end

# q (D, L, QH, B), k (D, L, KH, B), cos / sin (D, L, B), wq / wk (D): the memory of the header's layouts.  q_out may be q, k_out may be k.
function qk_norm_rope_fwd(q::ROCArray{T,4}, k::ROCArray{T,4}, wq::ROCVector{W}, wk::ROCVector{W}, cos::ROCArray{C,3}, sin::ROCArray{C,3};
                          ϵ::Float32 = 1f-6, offset::Float32 = 0f0, q_out::ROCArray{T,4} = similar(q),
                          k_out::ROCArray{T,4} = similar(k)) where {T <: HipFloat, W <: HipFloat, C <: HipFloat}
    @assert size(q_out) == size(q) && size(k_out) == size(k)
    d = qknrdesc(q, k, wq, wk, cos, sin, ϵ, offset)
    ok(GC.@preserve q_out k_out q k wq wk cos sin ccall(Libdl.dlsym(libnnop_ext(), :nnop_qk_norm_rope), Cint,
        (Ptr{QknrDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        d, devptr(q_out), devptr(k_out), devptr(q), devptr(k), devptr(wq), devptr(wk), devptr(cos), devptr(sin), hipstream()))
    return q_out, k_out
end

# (Δq, Δk) -> (dq, dk, dwq, dwk); dwq, dwk Float32, summed over rows in a fixed order.  dq may be Δq, dk may be Δk.
function qk_norm_rope_bwd(Δq::ROCArray{T,4}, Δk::ROCArray{T,4}, q::ROCArray{T,4}, k::ROCArray{T,4}, wq::ROCVector{W}, wk::ROCVector{W},
                          cos::ROCArray{C,3}, sin::ROCArray{C,3}; ϵ::Float32 = 1f-6, offset::Float32 = 0f0,
                          dq::ROCArray{T,4} = similar(q), dk::ROCArray{T,4} = similar(k)) where {T <: HipFloat, W <: HipFloat, C <: HipFloat}
    @assert size(Δq) == size(dq) == size(q) && size(Δk) == size(dk) == size(k)
    d = qknrdesc(q, k, wq, wk, cos, sin, ϵ, offset)
    dwq = ROCArray{Float32}(undef, length(wq)); dwk = similar(dwq)
    nbytes = ccall(Libdl.dlsym(libnnop_ext(), :nnop_qk_norm_rope_bwd_workspace_bytes), Csize_t, (Ptr{QknrDesc},), d)
    nbytes == 0 && error("libnnop_hip_ext: invalid qk_norm_rope descriptor")
    ws = ROCArray{UInt8}(undef, nbytes)
    ok(GC.@preserve dq dk dwq dwk Δq Δk q k wq wk cos sin ws ccall(Libdl.dlsym(libnnop_ext(), :nnop_qk_norm_rope_bwd), Cint,
        (Ptr{QknrDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}),
        d, devptr(dq), devptr(dk), devptr(dwq), devptr(dwk), devptr(Δq), devptr(Δk), devptr(q), devptr(k), devptr(wq), devptr(wk),
        devptr(cos), devptr(sin), devptr(ws), nbytes, hipstream()))
    return dq, dk, dwq, dwk
end

"""
    qk_norm_rope(q, k, wq, wk; cos, sin, ϵ=1f-6, offset=0f0) -> (q′, k′)

The per-head RMSNorm of Qwen3 / Gemma 3 / OLMo 2 on `q` and `k` (weights `wq`, `wk`, gain `w + offset`), then the Llama rotary embedding,
in one pass over memory: `llama_rope(rms_norm(q, wq), rms_norm(k, wk); cos, sin)` with the norm per head row and no rounding in between.
Differentiable in `q`, `k`, `wq`, `wk` through the ChainRules rule below, which keeps only its inputs.
"""
qk_norm_rope(q, k, wq, wk; cos, sin, ϵ::Float32 = 1f-6, offset::Float32 = 0f0) = qk_norm_rope_fwd(q, k, wq, wk, cos, sin; ϵ, offset)

function NNop.CRC.rrule(::typeof(qk_norm_rope), q, k, wq, wk; cos, sin, ϵ::Float32 = 1f-6, offset::Float32 = 0f0)
    q2, k2 = qk_norm_rope_fwd(q, k, wq, wk, cos, sin; ϵ, offset)
    function qk_norm_rope_pullback(Δ)
        Δq = Δ[1] isa NNop.CRC.AbstractZero ? fill!(similar(q2), 0) : _to_roc(NNop.CRC.unthunk(Δ[1]), q2)
        Δk = Δ[2] isa NNop.CRC.AbstractZero ? fill!(similar(k2), 0) : _to_roc(NNop.CRC.unthunk(Δ[2]), k2)
        dq, dk, dwq, dwk = qk_norm_rope_bwd(Δq, Δk, q, k, wq, wk, cos, sin; ϵ, offset)
        cast(dw, w) = eltype(w) === Float32 ? dw : eltype(w).(dw)
        return NNop.CRC.NoTangent(), dq, dk, cast(dwq, wq), cast(dwk, wk)
    end
    return (q2, k2), qk_norm_rope_pullback
end

end # module
