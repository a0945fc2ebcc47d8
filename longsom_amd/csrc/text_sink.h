// The sinks and number printers of the tables printed on the device (tables.hip, cellgeno.hip, genecounts.hip): a row is printed twice,
// first into a sink that only counts (its length), then into one that stores (its bytes).  What the host does between the two kernels -
// the rows' places from their lengths, the table's buffer - is text_table.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lsg {
namespace {

__device__ __forceinline__ int n_digits(uint64_t v) {
    int n = 1;
    while (v >= 10000) { v /= 10000; n += 4; }
    return n + (v >= 1000 ? 3 : v >= 100 ? 2 : v >= 10 ? 1 : 0);
}

struct LenSink {
    uint32_t n = 0;
    __device__ __forceinline__ void ch(char) { ++n; }
    __device__ __forceinline__ void str(const char*, int k) { n += (uint32_t)k; }
    __device__ __forceinline__ void u64(uint64_t v) { n += (uint32_t)n_digits(v); }
};
struct PutSink {
    char* p;
    __device__ __forceinline__ void ch(char c) { *p++ = c; }
    __device__ __forceinline__ void str(const char* s, int k) { for (int i = 0; i < k; ++i) p[i] = s[i]; p += k; }
    __device__ __forceinline__ void u64(uint64_t v) {
        const int d = n_digits(v);
        char* e = p + d;
        p = e;
        do { const uint64_t q = v / 10; *--e = (char)('0' + (int)(v - q * 10)); v = q; } while (v);
    }
};
#define LIT(s, text) (s).str(text, (int)sizeof(text) - 1)

template <class S> __device__ __forceinline__ void put_i64(S& s, int64_t v) {
    if (v < 0) { s.ch('-'); s.u64((uint64_t)(-v)); } else s.u64((uint64_t)v);
}
// repr(k / 10000.0) for the integer k = round(p, 4) * 1e4: at least one decimal, trailing zeros cut (tsvwrite.cpp put_p4)
template <class S> __device__ __forceinline__ void put_p4(S& s, int64_t k) {
    if (k < 0) { s.ch('-'); k = -k; }
    s.u64((uint64_t)(k / 10000));
    s.ch('.');
    const int f = (int)(k % 10000);
    const char d[4] = {(char)('0' + f / 1000), (char)('0' + f / 100 % 10), (char)('0' + f / 10 % 10), (char)('0' + f % 10)};
    int n = 4;
    while (n > 1 && d[n - 1] == '0') --n;
    for (int i = 0; i < n; ++i) s.ch(d[i]);
}
// str(round(a / float(b), 4)): the double quotient, its EXACT binary value rounded half-even to 4 decimals (what glibc's "%.4f" prints
// in tsvwrite.cpp put_ratio).  x * 1e4 = hi + lo exactly (fma); the fraction of hi against 1/2, then lo, decide.
template <class S> __device__ __forceinline__ void put_ratio(S& s, int64_t a, int64_t b) {
    if (b == 0) { LIT(s, "nan"); return; }          // (not reachable: a considered cell type has DP >= min_cov and NC >= min_cells)
    const double x = (double)a / (double)b;
    const double hi = x * 10000.0, lo = fma(x, 10000.0, -hi);
    const double fl = floor(hi);
    int64_t k = (int64_t)fl;
    const double t = ((hi - fl) - 0.5) + lo;        // (exact wherever its sign is in doubt: hi - fl is exact, and within [1/4, 3/4] so is the - 1/2)
    if (t > 0.0 || (t == 0.0 && (k & 1))) ++k;
    put_p4(s, k);
}

} // namespace
} // namespace lsg
