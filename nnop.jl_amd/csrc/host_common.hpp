// host_common.hpp -- host-side helpers shared by the three C boundaries (nnop_capi.cpp, nnop_ext_capi.cpp, nnop_moe_capi.cpp) and
// the row-operator launchers: what a dtype is, how a pointer list is checked, how a launcher gets from a nnop_dtype to a type.
// Host only, and nothing beyond include/nnop_hip.h: the extension and MoE libraries include it without the main library's tuning table.
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>
#include "../../include/nnop_hip.h"

namespace nnop {

static inline bool known_dtype(int32_t t) { return t == NNOP_F32 || t == NNOP_F16 || t == NNOP_BF16; }
static inline size_t dtype_bytes(int32_t t) { return t == NNOP_F32 ? 4 : 2; }

// a: a power of two.  NULL counts as aligned: an optional pointer is passed as it is, a required one has met the NULL pass first.
static inline bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
// every base fit for 16-byte accesses (what a launcher asks before it picks a vector kernel)
static inline bool aligned16(std::initializer_list<const void*> ptrs) {
    uintptr_t u = 0;
    for (const void* q : ptrs) u |= reinterpret_cast<uintptr_t>(q);
    return (u & 15) == 0;
}

// finite, and finite and >= 0; false for NaN (every comparison with it is)
static inline bool finite(float x) { return x >= -FLT_MAX && x <= FLT_MAX; }
static inline bool finite_nonneg(float x) { return x >= 0.f && x <= FLT_MAX; }

// The pointer check of every entry point, in two passes: NNOP_ERR_NULL if any pointer is NULL, only then NNOP_ERR_ALIGN if any is
// misaligned.  A group is the pointers that share one alignment.  `between` runs between the passes: an operator's own rule that
// belongs there (nnop_glu's absent pointers); its status is returned if it is not NNOP_OK.
struct PtrGroup { std::initializer_list<const void*> ptrs; size_t align; };
struct NoCheck { int operator()() const { return NNOP_OK; } };
template <typename F = NoCheck> static inline int check_ptrs(std::initializer_list<PtrGroup> groups, const F& between = F{}) {
    for (const PtrGroup& g : groups)
        for (const void* q : g.ptrs)
            if (!q) return NNOP_ERR_NULL;
    if (const int st = between(); st != NNOP_OK) return st;
    for (const PtrGroup& g : groups)
        for (const void* q : g.ptrs)
            if (misaligned(q, g.align)) return NNOP_ERR_ALIGN;
    return NNOP_OK;
}

// From a nnop_dtype to a type, in the style of dispatch_row_shape (row_common.hpp): f is a generic lambda that receives type tags
// (`typename decltype(t)::type` is the type) and returns a status; NNOP_ERR_DTYPE for an unknown value.
template <typename T> struct TypeTag { typedef T type; };
template <typename F> static inline int dispatch_dtype(int32_t dtype, F&& f) {
    switch (dtype) {
        case NNOP_F32:  return f(TypeTag<float>{});
        case NNOP_F16:  return f(TypeTag<_Float16>{});
        case NNOP_BF16: return f(TypeTag<__bf16>{});
    }
    return NNOP_ERR_DTYPE;
}
// f(T, S) for a tensor of `dtype` beside a side array (weights, cos / sin) of `side`: S = float when side is NNOP_F32, else T.
// T = float has the one combination (float, float) either way.
template <typename F> static inline int dispatch_dtype_side(int32_t dtype, int32_t side, F&& f) {
    return dispatch_dtype(dtype, [&](auto t) { return side == NNOP_F32 ? f(t, TypeTag<float>{}) : f(t, t); });
}

}  // namespace nnop
