// What the tables printed on the device (text_sink.h) and the row codes a host program shares with them (hccv_core.h) have in common:
// the two sinks a row is printed into - one that counts, one that stores -, the number printers, and the tests on a cell's text.
// Plain C++: every function is __host__ __device__ under hipcc and an ordinary inline function under a host compiler.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LSGT_HD __host__ __device__ __forceinline__
#define LSGT_HD_CALL __host__ __device__ inline      // (a function the compiler may keep as a call)
#else
#define LSGT_HD inline
#define LSGT_HD_CALL inline
#endif

namespace lsgt {

LSGT_HD int n_digits(uint64_t v) {
    int n = 1;
    while (v >= 10000) { v /= 10000; n += 4; }
    return n + (v >= 1000 ? 3 : v >= 100 ? 2 : v >= 10 ? 1 : 0);
}

struct LenSink {
    uint32_t n = 0;
    LSGT_HD void ch(char) { ++n; }
    LSGT_HD void str(const char*, int k) { n += (uint32_t)k; }
    LSGT_HD void u64(uint64_t v) { n += (uint32_t)n_digits(v); }
};
struct PutSink {
    char* p;
    LSGT_HD void ch(char c) { *p++ = c; }
    LSGT_HD void str(const char* s, int k) { for (int i = 0; i < k; ++i) p[i] = s[i]; p += k; }
    LSGT_HD void u64(uint64_t v) {
        const int d = n_digits(v);
        char* e = p + d;
        p = e;
        do { const uint64_t q = v / 10; *--e = (char)('0' + (int)(v - q * 10)); v = q; } while (v);
    }
};
#define LIT(s, text) (s).str(text, (int)sizeof(text) - 1)

template <class S> LSGT_HD void put_i64(S& s, int64_t v) {
    if (v < 0) { s.ch('-'); s.u64((uint64_t)(-v)); } else s.u64((uint64_t)v);
}
// repr(k / 10000.0) for the integer k = round(p, 4) * 1e4: at least one decimal, trailing zeros cut (tsvwrite.cpp put_p4)
template <class S> LSGT_HD void put_p4(S& s, int64_t k) {
    if (k < 0) { s.ch('-'); k = -k; }
    s.u64((uint64_t)(k / 10000));
    s.ch('.');
    const int f = (int)(k % 10000);
    const char d[4] = {(char)('0' + f / 1000), (char)('0' + f / 100 % 10), (char)('0' + f / 10 % 10), (char)('0' + f % 10)};
    int n = 4;
    while (n > 1 && d[n - 1] == '0') --n;
    for (int i = 0; i < n; ++i) s.ch(d[i]);
}
// k of round(a / float(b), 4) = k / 1e4: the double quotient, its EXACT binary value rounded half-even to 4 decimals (what glibc's
// "%.4f" prints in tsvwrite.cpp put_ratio).  x * 1e4 = hi + lo exactly (fma); the fraction of hi against 1/2, then lo, decide.  b != 0.
LSGT_HD int64_t ratio_k4(int64_t a, int64_t b) {
    const double x = (double)a / (double)b;
    const double hi = x * 10000.0, lo = fma(x, 10000.0, -hi);
    const double fl = floor(hi);
    int64_t k = (int64_t)fl;
    const double t = ((hi - fl) - 0.5) + lo;        // (exact wherever its sign is in doubt: hi - fl is exact, and within [1/4, 3/4] so is the - 1/2)
    if (t > 0.0 || (t == 0.0 && (k & 1))) ++k;
    return k;
}
// str(round(a / float(b), 4))
template <class S> LSGT_HD void put_ratio(S& s, int64_t a, int64_t b) {
    if (b == 0) { LIT(s, "nan"); return; }          // (not reachable: a considered cell type has DP >= min_cov and NC >= min_cells)
    put_p4(s, ratio_k4(a, b));
}

LSGT_HD bool text_eq(const char* f, int n, const char* lit, int m) {
    if (n != m) return false;
    for (int i = 0; i < n; ++i) if (f[i] != lit[i]) return false;
    return true;
}
#define TEXT_IS(f, n, lit) lsgt::text_eq(f, n, lit, (int)sizeof(lit) - 1)
// the strings pandas.read_csv takes for a missing value (tsvstep3.cpp is_na)
LSGT_HD_CALL bool text_is_na(const char* f, int n) {
    if (n == 0) return true;
    if (n > 8) return false;
    return TEXT_IS(f, n, "#N/A") || TEXT_IS(f, n, "#N/A N/A") || TEXT_IS(f, n, "#NA") || TEXT_IS(f, n, "-1.#IND") || TEXT_IS(f, n, "-1.#QNAN") || TEXT_IS(f, n, "-NaN") ||
           TEXT_IS(f, n, "-nan") || TEXT_IS(f, n, "1.#IND") || TEXT_IS(f, n, "1.#QNAN") || TEXT_IS(f, n, "<NA>") || TEXT_IS(f, n, "N/A") || TEXT_IS(f, n, "NA") ||
           TEXT_IS(f, n, "NULL") || TEXT_IS(f, n, "NaN") || TEXT_IS(f, n, "None") || TEXT_IS(f, n, "n/a") || TEXT_IS(f, n, "nan") || TEXT_IS(f, n, "null");
}
LSGT_HD_CALL bool text_contains(const char* f, int n, const char* lit, int m) {
    for (int i = 0; i + m <= n; ++i) { int j = 0; while (j < m && f[i + j] == lit[j]) ++j; if (j == m) return true; }
    return false;
}
#define TEXT_HAS(f, n, lit) lsgt::text_contains(f, n, lit, (int)sizeof(lit) - 1)

} // namespace lsgt
