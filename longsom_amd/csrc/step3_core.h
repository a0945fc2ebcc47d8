// The row code of step 3's final filters that the device kernels (step3.hip) and the host twin (hostio/step3rows.cpp) share: one data
// row of a step-2 table in; out what becomes of it (dropped / kept), its STEP3FILTER as a small set of tags, the rewritten fields of a
// multi-allelic row, and its INDEX - and the row's text in calling.step3.unfiltered.tsv / calling.step3.tsv.  Plain C++: every function is
// __host__ __device__ under hipcc and an ordinary inline function under a host compiler.  The field, number and multi-allelic helpers
// are row_core.h's, shared with hccv_core.h.
//
// Replaces, row for row, BaseCellCalling.step3.py:41-316 in the reference's order: the Cell_types drop (:41), MultiAllelic_filtering
// (:163-231), INDEX, chrM rows: the FILTER drop (:49-52) and chrM_filtering (:101-161); other rows: Min_cell_types, BC_CC_filtering
// (:233-251), BetaBino_filtering (:254-280), the FILTER drops (:60-84).  The executable statement of the rules is longsom_amd/calling.py
// (step3 and _multiallelic, _chrm, _bc_cc, _betabin) and hostio/tsvstep3.cpp.  As calling.step3 does, a row whose FILTER as it CAME holds
// one of the drop patterns (or whose Cell_types is Non-Cancer) is dropped before anything of it is parsed.  The cluster test (:283-306)
// needs a row's neighbours: step3_cluster.h, on the host, over the PASS rows' INDEX texts; its answer comes back as a sorted set of
// INDEX records that every kept row is looked up in (in_records).
//
// MultiAllelic_filtering differs from hccv_core.h's resolver in three places: the row is kept and tagged where HCCV drops it; with two
// cell types FILTER is left exactly as it came (only the one-cell-type branch strips Multi-allelic); and with two cell types the pairs
// print as (Non-Cancer, Cancer) whatever the order of Cell_types - while chrM_filtering afterwards picks from them BY that order.
//
// A row this code cannot decide as pandas and the reference's Python would is reported as undecided with a reason (enum lsg_hccv_reason);
// the caller then runs calling.step3 over the same input.  Nothing is guessed.
#pragma once
#include "row_core.h"

namespace lsg3 {
using lsgh::nth_field;
using lsgh::parse_dec;
using lsgh::parse_uint;
using lsgt::LenSink;
using lsgt::PutSink;

// lsg_step3_params::col, by name in the header line (hostio/tsvstep3.cpp's Col)
enum { C_CHROM = 0, C_START, C_REF, C_ALT, C_FILTER, C_CT, C_DP, C_NC, C_BC, C_CC, C_VAF, C_MCF, C_CTF, C_CANCER, C_NONCANCER, N_USED };
static_assert(N_USED == LSG_STEP3_COLS, "lsg_step3_params::col");
constexpr int INDEX_REC = LSG_STEP3_INDEX_MAX + 1;   // a record of the cluster set: the INDEX's length, its bytes, zeros

enum Fate { DROPPED = 0, KEPT, UNDECIDED };
// STEP3FILTER: the tags a row can get, in the order the code paths append them - which is the order they print in (tag(): the first
// replaces "PASS", later ones are comma-appended)
enum Tag { T_MULTI = 1, T_NOCOV = 2, T_LOWDEPTH = 4, T_LOWDVAF = 8, T_LOWDMCF = 16, T_LOWVAF = 32, T_LOWMCF = 64, T_CANCER_NONSIG = 128, T_NONCANCER_SIG = 256,
           T_CLUST = 512 };
struct Row {
    int32_t fo[N_USED], fl[N_USED];                  // the used fields: offset and length in the row (Non-Cancer may be absent: fl = -1)
    uint16_t tags;
    uint8_t fate, is_m, reason;
    uint8_t multi, top;                              // multi: 0 the six fields print as they came, 1 / 2 replaced for one / several cell types; top: the base index
    int64_t bc[2], cc[2], vaf_k[2], mcf_k[2];        // the replaced values in printing order (several cell types: Non-Cancer, Cancer); ratios as k of k / 1e4
};

// the FILTER patterns rows are dropped by: chrM rows (:49-52), the others' first (:60) and their remaining ones (:64-84)
LSGT_HD bool dead_m(const char* f, int n) { return TEXT_HAS(f, n, "Min") || TEXT_HAS(f, n, "LR") || TEXT_HAS(f, n, "gnomAD") || TEXT_HAS(f, n, "LC") || TEXT_HAS(f, n, "RNA"); }
LSGT_HD bool dead_min_ct(const char* f, int n) { return TEXT_HAS(f, n, "Min_cell_types"); }
LSGT_HD bool dead_rest(const char* f, int n) {
    return TEXT_HAS(f, n, "Noisy_site") || TEXT_HAS(f, n, "LC_Upstream") || TEXT_HAS(f, n, "LC_Downstream") || TEXT_HAS(f, n, "RNA_editing_db") || TEXT_HAS(f, n, "PoN") ||
           TEXT_HAS(f, n, "Cell_type_noise") || TEXT_HAS(f, n, "gnomAD");
}
LSGT_HD bool has_char(const char* f, int n, char c) { for (int i = 0; i < n; ++i) if (f[i] == c) return true; return false; }

// chrM_filtering's two differences (:120-135), the operations of the Python in their order.  No multiply-add may be fused in here.
LSGT_HD_CALL int chrm_delta_tag(double vaf_c, double vaf_n, double mcf_c, double mcf_n, double d_vaf, double d_mcf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dv = vaf_c - vaf_n;
    if (dv < d_vaf) return T_LOWDVAF;
    const double dm = mcf_c - mcf_n;
    return dm < d_mcf ? T_LOWDMCF : 0;
}

// [float(x) for x in text.split(",")]: every value must be a plain decimal, at least two of them; the first two come back
LSGT_HD bool two_decimals(const char* f, int n, double* v) {
    int o, l, k = 0; double x;
    for (; nth_field(f, n, ',', k, o, l); ++k) { if (!parse_dec(f + o, l, x)) return false; if (k < 2) v[k] = x; }
    return k >= 2;
}

// Decides one data row r[0 .. n) (its newline not counted).  Returns the row's fate; UNDECIDED leaves the reason in st.reason.
LSGT_HD_CALL int decide(const char* r, int n, const lsg_step3_params& p, Row& st) {
    st.tags = 0; st.fate = UNDECIDED; st.is_m = 0; st.reason = LSG_HCCV_OK; st.multi = 0; st.top = 0;
    auto undecided = [&](int why) { st.fate = UNDECIDED; st.reason = (uint8_t)why; return (int)UNDECIDED; };
    auto drop = [&]() { st.fate = DROPPED; return (int)DROPPED; };
    for (int k = 0; k < N_USED; ++k) { st.fo[k] = 0; st.fl[k] = -1; }
    // the fields; a character pandas' reader or writer treats specially (a quote, a carriage return, the comment sign) or a blank line: undecided
    if (n == 0) return undecided(LSG_HCCV_ODD_TEXT);
    int nf = 0;
    for (int f0 = 0; f0 <= n; ++nf) {
        int f1 = f0;
        while (f1 < n && r[f1] != '\t') { const char ch = r[f1]; if (ch == '"' || ch == '\r' || ch == '#') return undecided(LSG_HCCV_ODD_TEXT); ++f1; }
        for (int k = 0; k < N_USED; ++k) if (p.col[k] == nf) { st.fo[k] = f0; st.fl[k] = f1 - f0; }
        f0 = f1 + 1;
    }
    if (nf < p.n_cols) return undecided(LSG_HCCV_SHORT_ROW);
    if (nf > p.n_cols) return undecided(LSG_HCCV_LONG_ROW);
    auto F = [&](int k) { return r + st.fo[k]; };
    auto L = [&](int k) { return (int)st.fl[k]; };
    auto na = [&](int k) { return L(k) < 0 || lsgt::text_is_na(F(k), L(k)); };
    // 1. Cell_types (:41), and the FILTER patterns over the FILTER as it came (calling.step3 parses the survivors of both only)
    if (TEXT_IS(F(C_CT), L(C_CT), "Non-Cancer")) return drop();
    st.is_m = TEXT_IS(F(C_CHROM), L(C_CHROM), "chrM") ? 1 : 0;
    if (st.is_m ? dead_m(F(C_FILTER), L(C_FILTER)) : (dead_min_ct(F(C_FILTER), L(C_FILTER)) || dead_rest(F(C_FILTER), L(C_FILTER)))) return drop();
    // INDEX is made of #CHROM, Start and ALT and split at ':' again by the cluster test; FILTER, ALT and Cell_types are text to every row function
    if (na(C_CHROM) || na(C_START) || na(C_ALT) || na(C_FILTER) || na(C_CT)) return undecided(LSG_HCCV_MISSING);
    if (has_char(F(C_CHROM), L(C_CHROM), ':') || has_char(F(C_START), L(C_START), ':')) return undecided(LSG_STEP3_CHROM_COLON);
    // the cell types: how many, and where Cancer is among the first two (_cancer_index: the first, or else the second)
    int n_ct = 1;
    for (int i = 0; i < L(C_CT); ++i) n_ct += F(C_CT)[i] == ',';
    int i_c = 0;
    { int o, l; nth_field(F(C_CT), L(C_CT), ',', 0, o, l); i_c = TEXT_IS(F(C_CT) + o, l, "Cancer") ? 0 : 1; }
    const int i_n = 1 - i_c;
    // 2. MultiAllelic_filtering (:163-231)
    char filt[lsgh::FILTER_MAX];
    const char* flt = F(C_FILTER); int n_flt = L(C_FILTER);
    if (TEXT_HAS(flt, n_flt, "Multi-allelic") || has_char(F(C_ALT), L(C_ALT), '|')) {
        if (na(C_CANCER)) return undecided(LSG_HCCV_MISSING);
        int top; int64_t best, second;
        if (const int why = lsgh::dominant_alt(F(C_REF), L(C_REF), F(C_CANCER), L(C_CANCER), top, best, second)) return undecided(why);
        if (!((double)second / (double)best < 0.05)) st.tags |= T_MULTI;
        st.top = (uint8_t)top;
        if (n_ct > 1) {
            // (Non-Cancer, Cancer) whatever the order of Cell_types; FILTER stays exactly as it came
            if (na(C_NONCANCER)) return undecided(LSG_HCCV_MISSING);
            if (!lsgh::celltype_values(F(C_CANCER), L(C_CANCER), top, F(C_DP), L(C_DP), F(C_NC), L(C_NC), i_c, st.bc[1], st.cc[1], st.vaf_k[1], st.mcf_k[1]) ||
                !lsgh::celltype_values(F(C_NONCANCER), L(C_NONCANCER), top, F(C_DP), L(C_DP), F(C_NC), L(C_NC), i_n, st.bc[0], st.cc[0], st.vaf_k[0], st.mcf_k[0]))
                return undecided(LSG_HCCV_NUMBER);
            st.multi = 2;
        } else {
            if (!lsgh::celltype_values(F(C_CANCER), L(C_CANCER), top, F(C_DP), L(C_DP), F(C_NC), L(C_NC), -1, st.bc[0], st.cc[0], st.vaf_k[0], st.mcf_k[0]))
                return undecided(LSG_HCCV_NUMBER);
            if (n_flt > lsgh::FILTER_MAX) return undecided(LSG_HCCV_TOO_LONG);
            n_flt = lsgh::strip_multiallelic(flt, n_flt, filt); flt = filt;
            st.multi = 1;
        }
    }
    // 3. INDEX takes ALT's first value after the rewrite
    char alt0 = "ACTG"[st.top];
    if (!st.multi) {
        int o, l;
        nth_field(F(C_ALT), L(C_ALT), ',', 0, o, l);
        if (has_char(F(C_ALT) + o, l, ':')) return undecided(LSG_STEP3_CHROM_COLON);
        alt0 = F(C_ALT)[0];
    }
    if (st.is_m) {
        // 4. chrM rows: the FILTER patterns once more over the rewritten FILTER, then chrM_filtering (:101-161)
        if (dead_m(flt, n_flt)) return drop();
        if (n_ct > 1) {
            int o, l, o2, l2, o3, l3; int64_t d1, d2;
            if (!nth_field(F(C_DP), L(C_DP), ',', 0, o, l) || !nth_field(F(C_DP), L(C_DP), ',', 1, o2, l2) || nth_field(F(C_DP), L(C_DP), ',', 2, o3, l3)) return undecided(LSG_HCCV_NUMBER);
            if (!parse_uint(F(C_DP) + o, l, d1)) return undecided(LSG_HCCV_NUMBER);
            bool low = d1 < 100;
            if (!low) { if (!parse_uint(F(C_DP) + o2, l2, d2)) return undecided(LSG_HCCV_NUMBER); low = d2 < 100; }
            if (low) st.tags |= T_LOWDEPTH;
            else {
                double v[2], m[2];
                if (st.multi) { for (int q = 0; q < 2; ++q) { v[q] = (double)st.vaf_k[q] / 10000.0; m[q] = (double)st.mcf_k[q] / 10000.0; } }
                else if (!two_decimals(F(C_VAF), L(C_VAF), v) || !two_decimals(F(C_MCF), L(C_MCF), m)) return undecided(LSG_HCCV_NUMBER);
                st.tags |= (uint16_t)chrm_delta_tag(v[i_c], v[i_n], m[i_c], m[i_n], p.delta_vaf, p.delta_mcf);
            }
        } else {
            int64_t d; double v;
            if (!parse_uint(F(C_DP), L(C_DP), d)) return undecided(LSG_HCCV_NUMBER);
            if (d < 100) st.tags |= T_LOWDEPTH;
            else {
                if (st.multi) v = (double)st.vaf_k[0] / 10000.0; else if (!parse_dec(F(C_VAF), L(C_VAF), v)) return undecided(LSG_HCCV_NUMBER);
                if (v < 0.05) st.tags |= T_LOWVAF;
                else {
                    if (st.multi) v = (double)st.mcf_k[0] / 10000.0; else if (!parse_dec(F(C_MCF), L(C_MCF), v)) return undecided(LSG_HCCV_NUMBER);
                    if (v < 0.05) st.tags |= T_LOWMCF;
                }
            }
        }
    } else {
        // 5. the other rows: Min_cell_types (:60), BC_CC_filtering (:233-251), BetaBino_filtering (:254-280), the remaining drops (:64-84)
        if (dead_min_ct(flt, n_flt)) return drop();
        int i_alt = -1;
        for (int b = 0; b < 4; ++b) if ("ACTG"[b] == alt0) i_alt = b;
        if (i_alt < 0) return undecided(LSG_STEP3_ALT);
        if (na(C_CANCER)) st.tags |= T_NOCOV;
        else {
            int64_t reads, cells;
            if (!lsgh::info_count(F(C_CANCER), L(C_CANCER), 3, i_alt, reads)) return undecided(LSG_HCCV_NUMBER);
            if (reads < p.min_ac_reads) st.tags |= T_LOWDEPTH;
            else {
                if (!lsgh::info_count(F(C_CANCER), L(C_CANCER), 2, i_alt, cells)) return undecided(LSG_HCCV_NUMBER);
                if (cells < p.min_ac_cells) st.tags |= T_LOWDEPTH;
            }
        }
        auto weak = [](const char* f, int k) { return TEXT_IS(f, k, "Non-Significant") || TEXT_IS(f, k, "Low-Significance"); };
        if (n_ct == 1) { if (!na(C_CTF) && weak(F(C_CTF), L(C_CTF))) st.tags |= T_CANCER_NONSIG; }
        else {
            int o, l;
            if (na(C_CTF)) return undecided(LSG_HCCV_MISSING);
            if (!nth_field(F(C_CTF), L(C_CTF), ',', i_c, o, l)) return undecided(LSG_HCCV_CELL_TYPES);
            if (weak(F(C_CTF) + o, l)) st.tags |= T_CANCER_NONSIG;
            else {
                if (!nth_field(F(C_CTF), L(C_CTF), ',', i_n, o, l)) return undecided(LSG_HCCV_CELL_TYPES);
                if (TEXT_IS(F(C_CTF) + o, l, "PASS") || TEXT_IS(F(C_CTF) + o, l, "Low-Significance")) st.tags |= T_NONCANCER_SIG;
            }
        }
        if (dead_rest(flt, n_flt)) return drop();
    }
    st.fate = KEPT;
    return KEPT;
}

// INDEX = #CHROM:Start:ALT.split(",")[0], ALT after the rewrite
template <class S> LSGT_HD void put_index(S& s, const char* r, const Row& st) {
    s.str(r + st.fo[C_CHROM], st.fl[C_CHROM]); s.ch(':'); s.str(r + st.fo[C_START], st.fl[C_START]); s.ch(':');
    if (st.multi) s.ch("ACTG"[st.top]);
    else { int o, l; nth_field(r + st.fo[C_ALT], st.fl[C_ALT], ',', 0, o, l); s.str(r + st.fo[C_ALT] + o, l); }
}
// the row's record in the cluster set's form: rec[0] = the INDEX's length, then its bytes, then zeros.  false: longer than a record holds
LSGT_HD bool index_record(const char* r, const Row& st, uint8_t* rec) {
    LenSink m; put_index(m, r, st);
    if (m.n > (uint32_t)LSG_STEP3_INDEX_MAX) return false;
    rec[0] = (uint8_t)m.n;
    PutSink s{reinterpret_cast<char*>(rec + 1)}; put_index(s, r, st);
    for (int i = 1 + (int)m.n; i < INDEX_REC; ++i) rec[i] = 0;
    return true;
}
LSGT_HD int record_cmp(const uint8_t* a, const uint8_t* b) {
    for (int i = 0; i < INDEX_REC; ++i) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
// is key among the n sorted records?
LSGT_HD bool in_records(const uint8_t* recs, int64_t n, const uint8_t* key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int c = record_cmp(recs + mid * INDEX_REC, key);
        if (c == 0) return true;
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return false;
}

template <class S> LSGT_HD void put_tags(S& s, uint32_t tags, int64_t clust_dist) {
    if (!tags) { LIT(s, "PASS"); return; }
    bool first = true;
    auto name = [&](uint32_t bit, const char* text, int k) { if (tags & bit) { if (!first) s.ch(','); first = false; s.str(text, k); } };
#define STEP3_TAG(bit, text) name(bit, text, (int)sizeof(text) - 1)
    STEP3_TAG(T_MULTI, "Multi-Allelic"); STEP3_TAG(T_NOCOV, "NoCov"); STEP3_TAG(T_LOWDEPTH, "LowDepth"); STEP3_TAG(T_LOWDVAF, "LowDeltaVAF"); STEP3_TAG(T_LOWDMCF, "LowDeltaMCF");
    STEP3_TAG(T_LOWVAF, "LowVAF"); STEP3_TAG(T_LOWMCF, "LowMCF"); STEP3_TAG(T_CANCER_NONSIG, "CancerNonSig"); STEP3_TAG(T_NONCANCER_SIG, "NonCancerSig");
#undef STEP3_TAG
    if (tags & T_CLUST) { if (!first) s.ch(','); LIT(s, "Clust_dist_"); lsgt::put_i64(s, clust_dist); }
}
// what the cluster tag adds to a row's length
LSGT_HD uint32_t clust_tag_len(uint32_t tags_before, int64_t clust_dist) {
    LenSink a, b; put_tags(a, tags_before, clust_dist); put_tags(b, tags_before | T_CLUST, clust_dist);
    return b.n - a.n;
}

// The row's text in both tables, its newline included: every field as it came - a missing cell as nothing -, the six fields of a
// multi-allelic row replaced, then STEP3FILTER and INDEX.
template <class S> LSGT_HD void print_row(S& s, const char* r, int n, const lsg_step3_params& p, const Row& st, uint32_t tags) {
    int c = 0;
    const int m = st.multi;                          // values to print: 1 or 2
    for (int f0 = 0; f0 <= n; ++c) {
        int f1 = f0;
        while (f1 < n && r[f1] != '\t') ++f1;
        if (c) s.ch('\t');
        int which = -1;
        if (m) { const int ks[6] = {C_ALT, C_FILTER, C_BC, C_CC, C_VAF, C_MCF}; for (int q = 0; q < 6; ++q) if (p.col[ks[q]] == c) which = ks[q]; }
        if (which == C_FILTER && m == 2) which = -1;
        if (which == C_ALT) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); s.ch("ACTG"[st.top]); } }
        else if (which == C_FILTER) { char filt[lsgh::FILTER_MAX]; const int k = lsgh::strip_multiallelic(r + f0, f1 - f0, filt); s.str(filt, k); }
        else if (which == C_BC) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); s.u64((uint64_t)st.bc[q]); } }
        else if (which == C_CC) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); s.u64((uint64_t)st.cc[q]); } }
        else if (which == C_VAF) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); lsgt::put_p4(s, st.vaf_k[q]); } }
        else if (which == C_MCF) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); lsgt::put_p4(s, st.mcf_k[q]); } }
        else if (!lsgt::text_is_na(r + f0, f1 - f0)) s.str(r + f0, f1 - f0);
        f0 = f1 + 1;
    }
    s.ch('\t'); put_tags(s, tags, p.clust_dist);
    s.ch('\t'); put_index(s, r, st);
    s.ch('\n');
}
// a PASS row's line in the export the cluster test reads: its ordinal, a tab, its INDEX
template <class S> LSGT_HD void print_export(S& s, const char* r, const Row& st, int64_t ordinal) {
    s.u64((uint64_t)ordinal); s.ch('\t'); put_index(s, r, st); s.ch('\n');
}

} // namespace lsg3
