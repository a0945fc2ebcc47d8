// What the row codes over a step-2 table's text share (hccv_core.h: the high-confidence cancer variant filter; step3_core.h: step 3's
// final filters): the plain forms of the numbers a table prints, the pieces of a split field, the FILTER without its Multi-allelic tag,
// and the two halves of the multi-allelic resolvers both filters start from - the Cancer column's strongest non-reference base, and one
// cell type's counts and ratios at that base.  Plain C++: __host__ __device__ under hipcc, ordinary inline functions elsewhere.
#pragma once
#include <cstdint>
#include "text_core.h"
#include "../../include/longsom_hip.h"

namespace lsgh {
using lsgt::LenSink;
using lsgt::PutSink;

constexpr int FILTER_MAX = 256;                      // the longest FILTER the Multi-allelic strip takes

LSGT_HD bool is_dig(char c) { return c >= '0' && c <= '9'; }
// int(text) for the plain form the tables print: 1 to 15 digits
LSGT_HD bool parse_uint(const char* f, int n, int64_t& v) {
    if (n < 1 || n > 15) return false;
    int64_t x = 0;
    for (int i = 0; i < n; ++i) { if (!is_dig(f[i])) return false; x = x * 10 + (f[i] - '0'); }
    v = x;
    return true;
}
// float(text) for digits[.digits] of at most 15 digits in all: an integer over a power of ten, both exact, one correctly rounded division
LSGT_HD bool parse_dec(const char* f, int n, double& v) {
    if (n < 1 || n > 16) return false;
    int64_t m = 0; double p10 = 1.0; int nd = 0, ni = 0; bool dot = false;
    for (int i = 0; i < n; ++i) {
        if (f[i] == '.') { if (dot) return false; dot = true; ni = nd; continue; }
        if (!is_dig(f[i])) return false;
        m = m * 10 + (f[i] - '0'); ++nd;
        if (dot) p10 *= 10.0;
    }
    if (!dot) ni = nd;
    if (ni < 1 || nd > 15 || (dot && nd == ni)) return false;      // (".5" and "1." are numbers to Python, but not what a table prints)
    v = (double)m / p10;
    return true;
}
// field `idx` of f split by sep (str.split(sep)[idx]); false: there is none
LSGT_HD bool nth_field(const char* f, int n, char sep, int idx, int& off, int& len) {
    int a = 0;
    for (int k = 0;; ++k) {
        int b = a;
        while (b < n && f[b] != sep) ++b;
        if (k == idx) { off = a; len = b - a; return true; }
        if (b >= n) return false;
        a = b + 1;
    }
}
// int(info.split("|")[part].split(":")[idx])
LSGT_HD bool info_count(const char* f, int n, int part, int idx, int64_t& v) {
    int o, l, o2, l2;
    return nth_field(f, n, '|', part, o, l) && nth_field(f + o, l, ':', idx, o2, l2) && parse_uint(f + o + o2, l2, v);
}
// str.replace(pat, ""): out may not alias in
LSGT_HD int remove_all(const char* in, int n, const char* pat, int m, char* out) {
    int w = 0;
    for (int i = 0; i < n;) {
        int j = 0;
        if (i + m <= n) while (j < m && in[i + j] == pat[j]) ++j;
        if (j == m) i += m; else out[w++] = in[i++];
    }
    return w;
}
// the FILTER without its Multi-allelic tag (the three replacements in the reference's order); n <= FILTER_MAX
LSGT_HD int strip_multiallelic(const char* f, int n, char* out) {
    char tmp[FILTER_MAX];
    const int n1 = remove_all(f, n, "Multi-allelic,", 14, out);
    const int n2 = remove_all(out, n1, ",Multi-allelic", 14, tmp);
    return remove_all(tmp, n2, "Multi-allelic", 13, out);
}

// The strongest non-reference A/C/T/G base of a cell type's column (its read counts, part 3 of the info), the first of equals as
// np.argmax takes it, its reads and the runner-up's.  LSG_HCCV_OK, or why the Python would raise: a REF that is not one of ACTG, a count
// that is no plain integer (LSG_HCCV_NUMBER), no non-reference read at all - the reference divides by it - (LSG_HCCV_MAX_ZERO).
LSGT_HD int dominant_alt(const char* ref, int n_ref, const char* info, int n_info, int& top, int64_t& best, int64_t& second) {
    if (n_ref != 1) return LSG_HCCV_NUMBER;
    int i_ref = -1;
    for (int b = 0; b < 4; ++b) if ("ACTG"[b] == ref[0]) i_ref = b;
    if (i_ref < 0) return LSG_HCCV_NUMBER;
    int64_t cnt[4];
    for (int b = 0; b < 4; ++b) if (!info_count(info, n_info, 3, b, cnt[b])) return LSG_HCCV_NUMBER;
    cnt[i_ref] = 0;
    top = 0;
    for (int b = 1; b < 4; ++b) if (cnt[b] > cnt[top]) top = b;
    best = cnt[top];
    second = 0;
    for (int b = 0; b < 4; ++b) if (b != top && cnt[b] > second) second = cnt[b];
    return best == 0 ? LSG_HCCV_MAX_ZERO : LSG_HCCV_OK;
}
// One cell type's values at base `top`: bc, cc from its column's info, round(bc / dp, 4) and round(cc / nc, 4) as k of k / 1e4, dp and nc
// the i_ct-th of the row's Dp and Nc (i_ct < 0: the whole field, a table of one cell type).  false: a value the Python would raise on,
// a zero divisor among them.
LSGT_HD bool celltype_values(const char* info, int n_info, int top, const char* dp_f, int n_dp, const char* nc_f, int n_nc, int i_ct,
                             int64_t& bc, int64_t& cc, int64_t& vaf_k, int64_t& mcf_k) {
    int64_t dp, nc; int o, l;
    if (!info_count(info, n_info, 3, top, bc) || !info_count(info, n_info, 2, top, cc)) return false;
    if (i_ct < 0) { if (!parse_uint(dp_f, n_dp, dp) || !parse_uint(nc_f, n_nc, nc)) return false; }
    else if (!nth_field(dp_f, n_dp, ',', i_ct, o, l) || !parse_uint(dp_f + o, l, dp) || !nth_field(nc_f, n_nc, ',', i_ct, o, l) || !parse_uint(nc_f + o, l, nc)) return false;
    if (dp == 0 || nc == 0) return false;
    vaf_k = lsgt::ratio_k4(bc, dp); mcf_k = lsgt::ratio_k4(cc, nc);
    return true;
}

} // namespace lsgh
