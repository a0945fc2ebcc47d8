// hipcub's two-call idiom in one place: a call with no buffer says how much temporary storage it wants, the buffer is grown, the same
// call then runs with the buffer's whole capacity.
#pragma once
#include "lsg_ctx.h"
#include <hipcub/hipcub.hpp>

namespace lsg {

struct Widen { __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t& v) const { return (uint64_t)v; } };
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// call(void* p, size_t& bytes) -> hipError_t makes the hipcub call(s) on the caller's stream; `what` names it in the error text, beside
// the caller's file:line.  0, or -1 with the error set.
template <class F> int with_cub_tmp(DevBuf& tmp, const char* what, F call, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess) {
        if (tmp.reserve(bytes + 256)) return -1;
        bytes = tmp.cap;
        e = call(tmp.p, bytes);
    }
    if (e != hipSuccess) { set_error("%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line); return -1; }
    return 0;
}

template <class In, class Out> int exclusive_sum(DevBuf& tmp, In in, Out out, int64_t n, hipStream_t st, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    return with_cub_tmp(tmp, "hipcub::DeviceScan::ExclusiveSum", [&](void* p, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(p, b, in, out, (int)n, st); }, file, line);
}

} // namespace lsg
