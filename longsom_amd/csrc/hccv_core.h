// The row code of the high-confidence cancer variant filter that the device kernels (hccv.hip) and the host twin (hostio/hccvrows.cpp)
// share: one data row of the step-2 table in, what becomes of it and the text of its row in <out>.HCCV.tsv2 / .HCCV.tsv3 out.  Plain
// C++: every function is __host__ __device__ under hipcc and an ordinary inline function under a host compiler.
//
// Replaces, row for row, HCCV_SNV of workflow/scripts/CellTypeReannotation/HighConfidenceCancerVariants.py:8-88 with its helpers
// MultiAllelic_filtering (:90-163), DP_filtering (:200-209) and MCF_filtering (:212-255), in the reference's order; the executable
// statement of the rules is longsom_amd/reanno.py (_resolve_multiallelic, _depth_verdict, _delta_verdict, hccv_filter).  The cluster test
// (:165-197) needs a row's neighbours and stays with the caller, over the few PASS rows.
//
// A row this code cannot decide as pandas and the reference's Python would (a field that is not the number it should be, a division by
// zero, a missing ALT or FILTER, a short row ...) is reported as undecided with a reason; the caller then runs reanno.hccv_filter over
// the whole table.  Nothing is guessed.
#pragma once
#include "row_core.h"

namespace lsgh {

// lsg_hccv_params::col, by name in the header line
enum { C_CHROM = 0, C_START, C_REF, C_ALT, C_FILTER, C_CTYPES, C_DP, C_NC, C_BC, C_CC, C_VAF, C_MCF, C_CANCER, C_NONCANCER, N_USED };
static_assert(N_USED == LSG_HCCV_COLS, "lsg_hccv_params::col");

// how far a row came (in the reference's order), its verdict, and why it could not be decided
enum Stage { DROP_CELL_TYPES = 0, DROP_MULTI, DROP_DEPTH, IN_TSV2, IN_TSV3, UNDECIDED };
enum Verdict { V_PASS = 0, V_LOW, V_NONSIG, V_HET, V_LOW_DELTA, V_NONCANCER };
struct Row {
    int32_t fo[N_USED], fl[N_USED];                  // the used fields: offset and length in the row (Non-Cancer / Cancer may be absent: fl = -1)
    uint8_t stage, verdict, is_m, reason;
    uint8_t multi, top;                              // multi: 0 the six fields print as they came, 1 / 2 replaced for one / two cell types; top: the base index
    int64_t bc[2], cc[2], vaf_k[2], mcf_k[2];        // the replaced values in printing order (two cell types: Non-Cancer, Cancer); ratios as k of k / 1e4
};

// MCF_filtering's comparisons for two cell types (:230-251), the operations of the Python in their order; two_d_vaf = 2 * delta_vaf as
// the host computed it.  No multiply-add may be fused in here.
LSGT_HD_CALL int verdict_two(double vaf_c, double vaf_n, double mcf_c, double mcf_n, double two_d_vaf, double d_mcf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (vaf_c < 0.05) return V_NONSIG;
    if (vaf_n > 0.1) { const double d = vaf_c - vaf_n; if (d < two_d_vaf) return V_HET; }
    if (vaf_n > 0.2) return V_HET;
    const double d = mcf_c - mcf_n;
    return d < d_mcf ? V_LOW_DELTA : V_PASS;
}

LSGT_HD const char* verdict_name(int v, int& n) {
    switch (v) {
        case V_PASS: n = 4; return "PASS";
        case V_LOW: n = 11; return "Low VAF/MCF";
        case V_NONSIG: n = 6; return "NonSig";
        case V_HET: n = 12; return "Heterozygous";
        case V_LOW_DELTA: n = 11; return "LowDeltaMCF";
        default: n = 9; return "NonCancer";
    }
}

// Decides one data row r[0 .. n) (its newline not counted).  Returns the row's stage; UNDECIDED leaves the reason in st.reason.
LSGT_HD_CALL int decide(const char* r, int n, const lsg_hccv_params& p, Row& st) {
    st.stage = UNDECIDED; st.verdict = V_NONCANCER; st.is_m = 0; st.reason = LSG_HCCV_OK; st.multi = 0; st.top = 0;
    auto undecided = [&](int why) { st.stage = UNDECIDED; st.reason = (uint8_t)why; return (int)UNDECIDED; };
    auto stop = [&](int stage) { st.stage = (uint8_t)stage; return stage; };
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
    auto na = [&](int k) { return lsgt::text_is_na(F(k), L(k)); };
    // 1. Cell_types (:36)
    if (TEXT_IS(F(C_CTYPES), L(C_CTYPES), "Non-Cancer")) return stop(DROP_CELL_TYPES);
    // 2. INDEX is made of #CHROM, Start and ALT as they came (:33); FILTER and ALT are text to every row function
    if (na(C_CHROM) || na(C_START) || na(C_ALT) || na(C_FILTER)) return undecided(LSG_HCCV_MISSING);
    st.is_m = TEXT_IS(F(C_CHROM), L(C_CHROM), "chrM") ? 1 : 0;
    // the cell types: one or two, and which of two is Cancer (:95-100)
    int n_ct = 1;
    for (int i = 0; i < L(C_CTYPES); ++i) n_ct += F(C_CTYPES)[i] == ',';
    int i_c = 0; bool ct_ok = !na(C_CTYPES) && n_ct <= 2, one_is_cancer = false;
    if (ct_ok) {
        int o, l;
        nth_field(F(C_CTYPES), L(C_CTYPES), ',', 0, o, l);
        const bool c0 = TEXT_IS(F(C_CTYPES) + o, l, "Cancer");
        if (n_ct == 1) one_is_cancer = c0;
        else {
            nth_field(F(C_CTYPES), L(C_CTYPES), ',', 1, o, l);
            const bool c1 = TEXT_IS(F(C_CTYPES) + o, l, "Cancer");
            if (!c0 && !c1) ct_ok = false;
            i_c = c0 ? 0 : 1;
        }
    }
    // 3. MultiAllelic_filtering (:90-163)
    char filt[FILTER_MAX];
    const char* flt = F(C_FILTER); int n_flt = L(C_FILTER);
    bool touched = TEXT_HAS(flt, n_flt, "Multi-allelic");
    for (int i = 0; i < L(C_ALT) && !touched; ++i) touched = F(C_ALT)[i] == '|';
    if (touched) {
        if (!ct_ok) return undecided(LSG_HCCV_CELL_TYPES);
        if (n_ct == 1 && !one_is_cancer) return stop(DROP_MULTI);
        if (L(C_CANCER) < 0 || na(C_CANCER)) return undecided(LSG_HCCV_MISSING);
        // the cancer column's strongest non-reference base; kept only when the runner-up has less than 1/20 of its reads (:108-117)
        int top; int64_t best, second;
        if (const int why = dominant_alt(F(C_REF), L(C_REF), F(C_CANCER), L(C_CANCER), top, best, second)) return undecided(why);
        if (!((double)second / (double)best < 0.05)) return stop(DROP_MULTI);
        st.top = (uint8_t)top;
        // the six fields' new values (:119-160)
        auto one = [&](int col, int i_ct, int slot, bool whole) {          // bc, cc, round(bc / dp, 4), round(cc / nc, 4) of one cell type's column
            if (L(col) < 0 || na(col)) return false;
            return celltype_values(F(col), L(col), top, F(C_DP), L(C_DP), F(C_NC), L(C_NC), whole ? -1 : i_ct, st.bc[slot], st.cc[slot], st.vaf_k[slot], st.mcf_k[slot]);
        };
        if (n_ct == 1) { if (!one(C_CANCER, 0, 0, true)) return undecided(LSG_HCCV_NUMBER); st.multi = 1; }
        else { if (!one(C_CANCER, i_c, 1, false) || !one(C_NONCANCER, 1 - i_c, 0, false)) return undecided(LSG_HCCV_NUMBER); st.multi = 2; }
        if (n_flt > FILTER_MAX) return undecided(LSG_HCCV_TOO_LONG);
        n_flt = strip_multiallelic(flt, n_flt, filt); flt = filt;
    }
    // 4. DP_filtering (:200-209): both columns present, and min_dp reads in both
    if (L(C_CANCER) < 0 || L(C_NONCANCER) < 0 || na(C_CANCER) || na(C_NONCANCER)) return stop(DROP_DEPTH);
    {
        int o, l; int64_t d_c, d_n;
        nth_field(F(C_CANCER), L(C_CANCER), '|', 0, o, l);
        if (!parse_uint(F(C_CANCER) + o, l, d_c)) return undecided(LSG_HCCV_NUMBER);
        nth_field(F(C_NONCANCER), L(C_NONCANCER), '|', 0, o, l);
        if (!parse_uint(F(C_NONCANCER) + o, l, d_n)) return undecided(LSG_HCCV_NUMBER);
        if ((double)d_n < p.min_dp || (double)d_c < p.min_dp) return stop(DROP_DEPTH);
    }
    // 5. the FILTER patterns, chrM with its own list (:53-72)
    const bool dead = st.is_m ? (TEXT_HAS(flt, n_flt, "Min") || TEXT_HAS(flt, n_flt, "LR") || TEXT_HAS(flt, n_flt, "gnomAD") || TEXT_HAS(flt, n_flt, "LC") || TEXT_HAS(flt, n_flt, "RNA"))
                              : (TEXT_HAS(flt, n_flt, "Noisy_site") || TEXT_HAS(flt, n_flt, "LC_Upstream") || TEXT_HAS(flt, n_flt, "LC_Downstream") || TEXT_HAS(flt, n_flt, "gnomAD") ||
                                 TEXT_HAS(flt, n_flt, "RNA_editing_db") || TEXT_HAS(flt, n_flt, "PoN"));
    if (dead) return stop(IN_TSV2);
    // 6. MCF_filtering (:212-255) on the VAF and MCF of step 3
    if (!ct_ok) return undecided(LSG_HCCV_CELL_TYPES);
    if (n_ct == 1 && !one_is_cancer) { st.verdict = V_NONCANCER; return stop(IN_TSV3); }
    double vaf[2], mcf[2];                                   // in the field's own order
    if (st.multi) {
        // (the replaced values of two cell types read Non-Cancer, Cancer while Cell_types stays as it was: MCF_filtering picks by
        // Cell_types' order, and so does this)
        for (int q = 0; q < n_ct; ++q) { vaf[q] = (double)st.vaf_k[q] / 10000.0; mcf[q] = (double)st.mcf_k[q] / 10000.0; }
    } else {
        for (int q = 0; q < n_ct; ++q) {
            int o, l;
            if (!nth_field(F(C_VAF), L(C_VAF), ',', q, o, l) || !parse_dec(F(C_VAF) + o, l, vaf[q])) return undecided(LSG_HCCV_NUMBER);
            if (!nth_field(F(C_MCF), L(C_MCF), ',', q, o, l) || !parse_dec(F(C_MCF) + o, l, mcf[q])) return undecided(LSG_HCCV_NUMBER);
        }
        int o, l;
        if (nth_field(F(C_VAF), L(C_VAF), ',', n_ct, o, l) || nth_field(F(C_MCF), L(C_MCF), ',', n_ct, o, l)) return undecided(LSG_HCCV_NUMBER);      // (more values than cell types)
    }
    if (n_ct == 1) st.verdict = (vaf[0] >= p.delta_vaf && mcf[0] >= p.delta_mcf) ? V_PASS : V_LOW;
    else st.verdict = (uint8_t)verdict_two(vaf[i_c], vaf[1 - i_c], mcf[i_c], mcf[1 - i_c], p.two_delta_vaf, p.delta_mcf);
    return stop(IN_TSV3);
}

// The row's text in .HCCV.tsv2 (with_verdict: .HCCV.tsv3), its newline included: every field as it came - a missing cell as nothing -,
// the six fields of a resolved row replaced, then INDEX, DP_FILTER ("PASS": the rows that fail are gone) and the verdict.
template <class S> LSGT_HD void print_row(S& s, const char* r, int n, const lsg_hccv_params& p, const Row& st, bool with_verdict) {
    int c = 0;
    for (int f0 = 0; f0 <= n; ++c) {
        int f1 = f0;
        while (f1 < n && r[f1] != '\t') ++f1;
        if (c) s.ch('\t');
        int which = -1;
        if (st.multi) for (int k = C_ALT; k <= C_MCF; ++k) if (p.col[k] == c && k != C_CTYPES && k != C_DP && k != C_NC) which = k;
        const int m = st.multi;                      // values to print: 1 or 2
        if (which == C_ALT) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); s.ch("ACTG"[st.top]); } }
        else if (which == C_FILTER) { char filt[FILTER_MAX]; const int k = strip_multiallelic(r + f0, f1 - f0, filt); s.str(filt, k); }
        else if (which == C_BC) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); s.u64((uint64_t)st.bc[q]); } }
        else if (which == C_CC) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); s.u64((uint64_t)st.cc[q]); } }
        else if (which == C_VAF) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); lsgt::put_p4(s, st.vaf_k[q]); } }
        else if (which == C_MCF) { for (int q = 0; q < m; ++q) { if (q) s.ch(','); lsgt::put_p4(s, st.mcf_k[q]); } }
        else if (!lsgt::text_is_na(r + f0, f1 - f0)) s.str(r + f0, f1 - f0);
        f0 = f1 + 1;
    }
    s.ch('\t');
    s.str(r + st.fo[C_CHROM], st.fl[C_CHROM]); s.ch(':'); s.str(r + st.fo[C_START], st.fl[C_START]); s.ch(':');
    { int o, l; nth_field(r + st.fo[C_ALT], st.fl[C_ALT], ',', 0, o, l); s.str(r + st.fo[C_ALT] + o, l); }
    LIT(s, "\tPASS");
    if (with_verdict) { int k; const char* v = verdict_name(st.verdict, k); s.ch('\t'); s.str(v, k); }
    s.ch('\n');
}

} // namespace lsgh
