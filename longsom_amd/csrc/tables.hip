// The text of the reference's three big tables, printed on the device.
//
// Replaces the writers of
//   BaseCellCounter TSV rows     workflow/scripts/SNVCalling/BaseCellCounter.py:300-308
//   merged TSV rows              workflow/scripts/SNVCalling/MergeBaseCellCounts.py:48-84,116-204
//   step-1 TSV rows              workflow/scripts/SNVCalling/BaseCellCalling.step1.py:430-476
// (and the awk filter of BaseCellCalling.step2.py:23 for the rows step 2 keeps).  At C2 these are 16.6 GB of text for 24 M sites; on the
// host's cores (hostio/tsvwrite.cpp, the same rules, kept as the test reference and for the per-region pieces) printing them is what an
// end-to-end run waits for.  Here one thread prints one row, twice: a first pass with a sink that only counts gives every row its
// length, a scan gives it its place (the contigs in Python string order: a row's place is its genomic-order offset plus its contig's
// shift), a second pass with a sink that stores writes the bytes.  The host moves bytes: lsg_append_table streams the buffer through two
// pinned staging buffers into pwrite.
#include "lsg_ctx.h"
#include "call_rec.h"
#include "text_sink.h"
#include "text_table.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include <fcntl.h>
#include <unistd.h>

namespace lsg {
int run_export_rows(lsg_ctx* c, int ct, DevBuf& dk, DevBuf& dr, DevBuf& dc);

namespace {

// 'DP|NC|CC|BC|BQ|BCf|BCr' values of one LSG_ROW_WORDS row: six printed classes per vector
template <class S> __device__ __forceinline__ void put_row(S& s, const uint32_t* c) {
    s.u64(c[0]); s.ch('|'); s.u64(c[1]);
    for (int o = 2; o < 42; o += 8) {
        s.ch('|');
        for (int k = 0; k < 6; ++k) { if (k) s.ch(':'); s.u64(c[o + k]); }
    }
}

struct FmtArgs {
    int32_t kind, ct, n_ct, n_contigs;
    int64_t n;                                        // rows of the cell type (counts) or merged sites
    const int64_t* keys[LSG_MAX_CELLTYPES]; const uint8_t* refs[LSG_MAX_CELLTYPES]; const uint32_t* rows[LSG_MAX_CELLTYPES]; int64_t n_rows[LSG_MAX_CELLTYPES];
    const SiteRec* sites; const CandCt* cands;
    const uint8_t* const* ref_ptr; const int64_t* contig_len;
    const char* contig_txt; const uint32_t* contig_off;       // contig t's name = contig_txt[contig_off[t] .. contig_off[t + 1])
    const char* ct_txt; const uint32_t* ct_off;
    uint32_t* len; const uint64_t* off; const int64_t* shift; char* text;
    const int64_t* posset[3]; int64_t n_posset[3];    // K_STEP2: the resident position sets (RNA editing, PoN_SR, PoN_LR)
    const int64_t* alleles; int64_t n_alleles;        // K_STEP2: the resident allele set of the gnomAD filter (n_alleles < 0: none loaded)
};
enum { K_COUNTS = 0, K_MERGED, K_STEP1, K_KEPT, K_STEP2 };

__device__ __forceinline__ int64_t row_of(const FmtArgs& a, int ct, int64_t key) {
    const int64_t* k = a.keys[ct];
    int64_t lo = 0, hi = a.n_rows[ct];
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (k[mid] < key) lo = mid + 1; else hi = mid; }
    return (lo < a.n_rows[ct] && k[lo] == key) ? lo : -1;
}
template <class S> __device__ __forceinline__ void put_name(S& s, const char* txt, const uint32_t* off, int i) {
    s.str(txt + off[i], (int)(off[i + 1] - off[i]));
}
__device__ __forceinline__ const char* ct_filter_name(int f, int& n) {
    switch (f) {
        case LSG_CF_NONSIG: n = 15; return "Non-Significant";
        case LSG_CF_LOWSIG: n = 16; return "Low-Significance";
        case LSG_CF_MULTI: n = 13; return "Multi-allelic";
        case LSG_CF_LOW_CELLS: n = 9; return "Low_cells";
        case LSG_CF_LOW_READS: n = 9; return "Low_reads";
        case LSG_CF_PASS: n = 4; return "PASS";
        default: n = 0; return "";
    }
}
__device__ __forceinline__ const char* site_filter_name(int bit, int& n) {
    switch (bit) {
        case 0: n = 19; return "Multiple_cell_types";
        case 1: n = 13; return "Multi-allelic";
        case 2: n = 14; return "Min_cell_types";
        case 3: n = 15; return "Cell_type_noise";
        case 4: n = 10; return "Noisy_site";
        case 5: n = 11; return "LC_Upstream";
        default: n = 13; return "LC_Downstream";
    }
}

template <class S> __device__ void count_row(S& s, const FmtArgs& a, int64_t i) {
    const int64_t k = a.keys[a.ct][i];
    put_name(s, a.contig_txt, a.contig_off, (int)(k >> 32)); s.ch('\t');
    s.u64((uint64_t)(k & 0xFFFFFFFFll) + 1); s.ch('\t');
    s.ch((char)a.refs[a.ct][i]); s.ch('\t'); LIT(s, "DP|NC|CC|BC|BQ|BCf|BCr"); s.ch('\t');
    put_row(s, a.rows[a.ct] + i * LSG_ROW_WORDS); s.ch('\n');
}

template <class S> __device__ void merged_row(S& s, const FmtArgs& a, int64_t i) {
    const int64_t k = a.sites[i].key;
    int64_t r[LSG_MAX_CELLTYPES];
    for (int c = 0; c < a.n_ct; ++c) r[c] = row_of(a, c, k);
    put_name(s, a.contig_txt, a.contig_off, (int)(k >> 32)); s.ch('\t');
    s.u64((uint64_t)(k & 0xFFFFFFFFll) + 1); s.ch('\t'); s.u64((uint64_t)(k & 0xFFFFFFFFll) + 1); s.ch('\t');
    // sort_set (MergeBaseCellCounts.py:48-57): distinct REFs by decreasing count, first-seen order on ties
    char seen[LSG_MAX_CELLTYPES]; int cnt[LSG_MAX_CELLTYPES]; int ns = 0;
    for (int c = 0; c < a.n_ct; ++c) {
        if (r[c] < 0) continue;
        const char b = (char)a.refs[c][r[c]];
        int q = 0; while (q < ns && seen[q] != b) ++q;
        if (q == ns) { seen[ns] = b; cnt[ns++] = 1; } else ++cnt[q];
    }
    int idx[LSG_MAX_CELLTYPES] = {0, 1, 2, 3};
    for (int x = 1; x < ns; ++x) { const int v = idx[x]; int y = x; while (y > 0 && cnt[idx[y - 1]] < cnt[v]) { idx[y] = idx[y - 1]; --y; } idx[y] = v; }
    for (int q = 0; q < ns; ++q) { if (q) s.ch('|'); s.ch(seen[idx[q]]); }
    s.ch('\t'); LIT(s, "DP|NC|CC|BC|BQ|BCf|BCr");
    for (int c = 0; c < a.n_ct; ++c) {
        s.ch('\t');
        if (r[c] < 0) LIT(s, "NA"); else put_row(s, a.rows[c] + r[c] * LSG_ROW_WORDS);
    }
    s.ch('\n');
}

__device__ __forceinline__ bool in_set(const int64_t* k, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (k[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < n && k[lo] == key;
}
__device__ __forceinline__ bool in_posset(const FmtArgs& a, int kind, int64_t key) { return in_set(a.posset[kind], a.n_posset[kind], key); }

// The allele key (lsg_load_alleleset) of a candidate site whose ALT field prints as exactly one base - one cell type with candidates,
// carrying one alternative -, else -1.  That string is what step 2 looks up in gnomAD (BaseCellCalling.step2.py:98-114): "A|C" and "A,A"
// are no allele of the database.
__device__ __forceinline__ int64_t allele_key_of(const SiteRec& c, const CandCt* cands, int n_ct) {
    int only = -1, n_with = 0;
    for (int ct = 0; ct < n_ct; ++ct) if ((c.has_cand >> ct) & 1) { only = ct; ++n_with; }
    if (n_with != 1) return -1;
    const CandCt& d = cands[(uint64_t)c.cand * n_ct + only];
    if (d.n_alt != 1) return -1;
    const int64_t tid = c.key >> 32, pos1 = (c.key & 0xFFFFFFFFll) + 1;
    return (tid << 48) | (pos1 << 16) | ((int64_t)c.ref << 8) | (int64_t)(uint8_t)"ACTG"[d.alt[0] & 3];
}

// one row of the step-1 table (tsvwrite.cpp lsio_write_step1_rows, from the compact records instead of their lsg_call expansion).
// STEP2: the row as BaseCellCalling.step2.py leaves it when it has no gnomAD source and no distance filter (calling._step2_scanned):
// FILTER tagged by the position sets (GetExtraFilters, step2.py:142-158: "RNA_editing_db", "PoN_SR", "PoN_LR"; a tag replaces a bare
// "PASS"), every field but the first that is exactly "NA" empty (what the pandas round trip of step2.py does to them).
template <bool STEP2, class S> __device__ void step1_row(S& s, const FmtArgs& a, int64_t i) {
    const SiteRec c = a.sites[i];
    const int64_t k = c.key;
    const int tid = (int)(k >> 32);
    const int64_t pos = k & 0xFFFFFFFFll;
    const uint32_t sf = c.site_filter;
    const bool cand = (sf & (uint32_t)LSG_SF_CANDIDATE) != 0;
    int64_t r[LSG_MAX_CELLTYPES];
    for (int ct = 0; ct < a.n_ct; ++ct) r[ct] = row_of(a, ct, k);
    put_name(s, a.contig_txt, a.contig_off, tid); s.ch('\t');
    s.u64((uint64_t)pos + 1); s.ch('\t'); s.u64((uint64_t)pos + 1); s.ch('\t');
    s.ch((char)c.ref); s.ch('\t');
    auto context = [&]() {                             // Up_context \t Down_context ("." "." when POS < 6, step1.py:98-105)
        if (pos >= 5) {
            const uint8_t* ref = a.ref_ptr[tid];
            for (int q = 0; q < 5; ++q) s.ch((char)ref[pos - 5 + q]);
            s.ch('\t');
            if (STEP2 && pos + 3 == a.contig_len[tid] && ref[pos + 1] == 'N' && ref[pos + 2] == 'A') return;      // (a two-base context that reads "NA")
            for (int q = 0; q < 5 && pos + 1 + q < a.contig_len[tid]; ++q) s.ch((char)ref[pos + 1 + q]);
        } else LIT(s, ".\t.");
    };
    auto rest = [&](int q) {                           // Rest_BC / Rest_CC
        const int64_t s_alt = q ? c.sum_alts_cc : c.sum_alts_bc, s_tot = q ? c.sum_nc : c.sum_dp, pk = q ? c.noise_p_cc : c.noise_p_bc;
        put_i64(s, s_alt); s.ch(';'); put_i64(s, s_tot); s.ch(';');
        if (c.sum_alts_bc == 0) s.ch('1'); else if (pk == -2) LIT(s, "nan"); else put_p4(s, pk);
    };
    if (cand) {
        const CandCt* d = a.cands + (uint64_t)c.cand * a.n_ct;
        auto n_alt = [&](int ct) { const int na = d[ct].n_alt; return na < LSG_CALL_MAX_ALT ? na : LSG_CALL_MAX_ALT; };
        auto column = [&](auto&& per_ct) {             // one value group per cell type with candidates, ',' between them
            bool first = true;
            for (int ct = 0; ct < a.n_ct; ++ct) {
                if (!((c.has_cand >> ct) & 1)) continue;
                if (!first) s.ch(',');
                first = false;
                per_ct(ct);
            }
        };
        auto per_alt = [&](int ct, auto&& one) { const int na = n_alt(ct); for (int q = 0; q < na; ++q) { if (q) s.ch('|'); one(q); } };
        auto filters = [&]() { column([&](int ct) { int n; const char* f = ct_filter_name(d[ct].ct_filter, n); s.str(f, n); }); };
        bool any_pass = false; int n_alt_str = 0;
        for (int ct = 0; ct < a.n_ct; ++ct) {
            if (!((c.has_cand >> ct) & 1)) continue;
            any_pass |= d[ct].ct_filter == LSG_CF_PASS;
            bool dup = false;                          // distinct ALT strings among the cell types (step1.py: len(set(ALTs)))
            for (int o = 0; o < ct; ++o) {
                if (!((c.has_cand >> o) & 1) || n_alt(o) != n_alt(ct)) continue;
                bool same = true;
                for (int q = 0; q < n_alt(ct); ++q) same &= (d[o].alt[q] & 3) == (d[ct].alt[q] & 3);
                dup |= same;
            }
            n_alt_str += !dup;
        }
        column([&](int ct) { per_alt(ct, [&](int q) { s.ch("ACTG"[d[ct].alt[q] & 3]); }); });
        s.ch('\t');
        bool any_site = false;
        for (int b = 0; b < 7; ++b) if (sf & (1u << b)) { if (any_site) s.ch(','); any_site = true; int n; const char* f = site_filter_name(b, n); s.str(f, n); }
        bool bare_pass = false;
        if (!any_site) { if (any_pass) bare_pass = true; else filters(); }
        if (STEP2) {
            const int64_t k1 = ((int64_t)tid << 32) | (pos + 1);
            const bool tag[3] = {in_posset(a, 0, k1), in_posset(a, 1, k1), in_posset(a, 2, k1)};
            for (int q = 0; q < 3; ++q) {
                if (!tag[q]) continue;
                if (bare_pass) bare_pass = false; else s.ch(',');
                if (q == 0) LIT(s, "RNA_editing_db"); else if (q == 1) LIT(s, "PoN_SR"); else LIT(s, "PoN_LR");
            }
            if (a.n_alleles > 0) {                     // gnomAD (step2.py:223-235): after the position sets' tags
                const int64_t ak = allele_key_of(c, a.cands, a.n_ct);
                if (ak >= 0 && in_set(a.alleles, a.n_alleles, ak)) {
                    if (bare_pass) bare_pass = false; else s.ch(',');
                    LIT(s, "gnomAD");
                }
            }
        }
        if (bare_pass) LIT(s, "PASS");
        s.ch('\t');
        {
            int only = -1, n_with = 0;
            for (int ct = 0; ct < a.n_ct; ++ct) if ((c.has_cand >> ct) & 1) { only = ct; ++n_with; }
            const bool reads_na = STEP2 && n_with == 1 && a.ct_off[only + 1] - a.ct_off[only] == 2 && a.ct_txt[a.ct_off[only]] == 'N' && a.ct_txt[a.ct_off[only] + 1] == 'A';
            if (!reads_na) column([&](int ct) { put_name(s, a.ct_txt, a.ct_off, ct); });
        }
        s.ch('\t'); context(); s.ch('\t');
        s.u64((uint64_t)n_alt_str);
        s.ch('\t'); column([&](int ct) { s.u64(a.rows[ct][r[ct] * LSG_ROW_WORDS]); });
        s.ch('\t'); column([&](int ct) { s.u64(a.rows[ct][r[ct] * LSG_ROW_WORDS + 1]); });
        s.ch('\t'); column([&](int ct) { per_alt(ct, [&](int q) { s.u64(d[ct].alt_bc[q]); }); });
        s.ch('\t'); column([&](int ct) { per_alt(ct, [&](int q) { s.u64(d[ct].alt_cc[q]); }); });
        s.ch('\t'); column([&](int ct) { per_alt(ct, [&](int q) { put_ratio(s, d[ct].alt_bc[q], a.rows[ct][r[ct] * LSG_ROW_WORDS]); }); });
        s.ch('\t'); column([&](int ct) { per_alt(ct, [&](int q) { put_ratio(s, d[ct].alt_cc[q], a.rows[ct][r[ct] * LSG_ROW_WORDS + 1]); }); });
        s.ch('\t'); column([&](int ct) { per_alt(ct, [&](int q) { put_p4(s, d[ct].p_bc[q]); }); });
        s.ch('\t'); column([&](int ct) { per_alt(ct, [&](int q) { put_p4(s, d[ct].p_cc[q]); }); });
        s.ch('\t'); put_i64(s, c.cell_types_min); s.ch('\t'); put_i64(s, c.cell_types_min);
        s.ch('\t'); rest(0); s.ch('\t'); rest(1); LIT(s, "\t.\t"); filters();
    } else {
        LIT(s, ".\t");
        if (sf & 16u) LIT(s, "Noisy_site"); else s.ch('.');
        LIT(s, "\t.\t"); context();
        LIT(s, "\t.\t.\t.\t.\t.\t.\t.\t.\t.\t"); put_i64(s, c.cell_types_min); s.ch('\t'); put_i64(s, c.cell_types_min);
        s.ch('\t'); rest(0); s.ch('\t'); rest(1); LIT(s, "\t.\t.");
    }
    s.ch('\t'); LIT(s, "DP|NC|CC|BC|BQ|BCf|BCr");
    for (int ct = 0; ct < a.n_ct; ++ct) {
        s.ch('\t');
        if (r[ct] < 0) { if (!STEP2) LIT(s, "NA"); } else put_row(s, a.rows[ct] + r[ct] * LSG_ROW_WORDS);
    }
    s.ch('\n');
}

template <class S> __device__ __forceinline__ void any_row(S& s, const FmtArgs& a, int64_t i) {
    switch (a.kind) {
        case K_COUNTS: count_row(s, a, i); break;
        case K_MERGED: merged_row(s, a, i); break;
        case K_STEP1: step1_row<false>(s, a, i); break;
        case K_KEPT: if (a.sites[i].site_filter & (uint32_t)LSG_SF_CANDIDATE) step1_row<false>(s, a, i); break;      // (a candidate's ALT and FILTER are never ".")
        default: if (a.sites[i].site_filter & (uint32_t)LSG_SF_CANDIDATE) step1_row<true>(s, a, i);
    }
}
__device__ __forceinline__ int64_t key_at(const FmtArgs& a, int64_t i) { return a.kind == K_COUNTS ? a.keys[a.ct][i] : a.sites[i].key; }

__global__ __launch_bounds__(256) void k_row_len(FmtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.n) return;
    LenSink s;
    if (i < a.n) any_row(s, a, i);
    a.len[i] = s.n;
}
__global__ __launch_bounds__(256) void k_row_put(FmtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    PutSink s{a.text + (int64_t)a.off[i] + a.shift[(int)(key_at(a, i) >> 32)]};
    any_row(s, a, i);
}
// the allele queries of the rows step 2 keeps (lsg_step2_allele_queries): a "row" of length 1 per candidate site with a one-base ALT,
// placed like the tables' rows
__global__ __launch_bounds__(256) void k_query_len(FmtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.n) return;
    a.len[i] = (i < a.n && (a.sites[i].site_filter & (uint32_t)LSG_SF_CANDIDATE) && allele_key_of(a.sites[i], a.cands, a.n_ct) >= 0) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_query_put(FmtArgs a, int64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || a.len[i] == 0) return;
    out[(int64_t)a.off[i] + a.shift[(int)(a.sites[i].key >> 32)]] = allele_key_of(a.sites[i], a.cands, a.n_ct);
}
// lo[t] = first row of contig t (t = n_contigs: the row count); then, contig after contig in output order, shift[t] = where the contig's
// text starts in the output minus where it starts in genomic order
__global__ void k_contig_lo(FmtArgs a, int64_t* lo) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > a.n_contigs) return;
    const int64_t want = (int64_t)t << 32;
    int64_t l = 0, h = a.n;
    while (l < h) { const int64_t mid = (l + h) >> 1; if (key_at(a, mid) < want) l = mid + 1; else h = mid; }
    lo[t] = l;
}
__global__ void k_contig_shift(const int64_t* lo, const uint64_t* off, const int32_t* order, int n_contigs, int64_t* shift) {
    if (threadIdx.x || blockIdx.x) return;
    int64_t base = 0;
    for (int j = 0; j < n_contigs; ++j) {
        const int t = order[j];
        const int64_t b = (int64_t)off[lo[t]], e = (int64_t)off[lo[t + 1]];
        shift[t] = base - b;
        base += e - b;
    }
}
// the contig step of finish_places for rows whose keys `a` holds
void contig_order(const FmtArgs& a, const RowPlaces& r, const int32_t* order, hipStream_t st) {
    hipLaunchKernelGGL(k_contig_lo, dim3((unsigned)(a.n_contigs / 64 + 1)), dim3(64), 0, st, a, r.lo);
    hipLaunchKernelGGL(k_contig_shift, dim3(1), dim3(1), 0, st, r.lo, r.off, order, a.n_contigs, r.shift);
}

// ---- what step 3 wants to know about the step-2 table, read off its text where it lies ---------------------------------------------
// (calling.step3 parses only the rows that survive its FILTER patterns, given the kinds of cell every column holds over ALL rows: the
// host finds both with passes over the table's gigabytes, hostio/tsvstep3.cpp lsio_step3_column_kinds and tsvscan.cpp; these are the
// same rules over the same bytes, one thread per row.)
using lsgt::text_is_na;      // (text_core.h: the cell tests a host program shares)
__device__ __forceinline__ bool is_dig(char c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ bool is_xdig(char c) { return is_dig(c) || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'); }
__device__ __forceinline__ char lower(char c) { return (c >= 'A' && c <= 'Z') ? (char)(c + 32) : c; }
__device__ bool all_digits(const char* s, int n) { if (n <= 0) return false; for (int i = 0; i < n; ++i) if (!is_dig(s[i])) return false; return true; }
__device__ bool ci_prefix(const char* f, int n, const char* lit, int m) { if (n < m) return false; for (int i = 0; i < m; ++i) if (lower(f[i]) != lit[i]) return false; return true; }
// does strtod (C locale) take the whole field, trailing blanks aside?  (tsvstep3.cpp classify: a number pandas would read and print differently)
__device__ bool strtod_takes_all(const char* f, int n) {
    int i = 0;
    while (i < n && (f[i] == ' ' || (f[i] >= '\t' && f[i] <= '\r'))) ++i;
    if (i < n && (f[i] == '+' || f[i] == '-')) ++i;
    int end;
    if (ci_prefix(f + i, n - i, "inf", 3)) { end = i + 3; if (ci_prefix(f + end, n - end, "inity", 5)) end += 5; }
    else if (ci_prefix(f + i, n - i, "nan", 3)) {
        end = i + 3;
        if (end < n && f[end] == '(') {
            int k = end + 1;
            while (k < n && (is_dig(f[k]) || (lower(f[k]) >= 'a' && lower(f[k]) <= 'z') || f[k] == '_')) ++k;
            if (k < n && f[k] == ')') end = k + 1;
        }
    } else if (i + 1 < n && f[i] == '0' && (f[i + 1] == 'x' || f[i + 1] == 'X')) {
        int j = i + 2, nd = 0;
        while (j < n && is_xdig(f[j])) { ++j; ++nd; }
        if (j < n && f[j] == '.') { int j2 = j + 1, nf = 0; while (j2 < n && is_xdig(f[j2])) { ++j2; ++nf; } if (nd + nf > 0) { j = j2; nd += nf; } }
        if (nd == 0) end = i + 1;                       // only the "0" of "0x" is a number
        else {
            if (j < n && (f[j] == 'p' || f[j] == 'P')) { int k = j + 1; if (k < n && (f[k] == '+' || f[k] == '-')) ++k; if (k < n && is_dig(f[k])) { while (k < n && is_dig(f[k])) ++k; j = k; } }
            end = j;
        }
    } else {
        int j = i, nd = 0;
        while (j < n && is_dig(f[j])) { ++j; ++nd; }
        if (j < n && f[j] == '.') { int j2 = j + 1, nf = 0; while (j2 < n && is_dig(f[j2])) { ++j2; ++nf; } if (nd + nf > 0) { j = j2; nd += nf; } }
        if (nd == 0) j = 0;                             // no number: strtod hands the start of the field back ...
        else if (j < n && (f[j] == 'e' || f[j] == 'E')) { int k = j + 1; if (k < n && (f[k] == '+' || f[k] == '-')) ++k; if (k < n && is_dig(f[k])) { while (k < n && is_dig(f[k])) ++k; j = k; } }
        end = j;
    }
    while (end < n && f[end] == ' ') ++end;             // (... from where the host's check walks over blanks too: a field of blanks alone counts as taken)
    return end == n && end != 0;
}
enum { KIND_NA = 1, KIND_INT = 2, KIND_FLOAT = 4, KIND_ODD = 8, KIND_OTHER = 16 };
// the kind of one cell (tsvstep3.cpp classify, rule for rule)
__device__ int text_kind(const char* f, int n) {
    if (text_is_na(f, n)) return KIND_NA;
    const char* s = f; int m = n; bool neg = false;
    if (m && s[0] == '-') { neg = true; ++s; --m; }
    if (all_digits(s, m)) return ((m > 1 && s[0] == '0') || (neg && m == 1 && s[0] == '0') || m > 18) ? KIND_ODD : KIND_INT;
    int dot = -1;
    for (int i = 0; i < m; ++i) if (s[i] == '.') { dot = i; break; }
    if (dot >= 0 && all_digits(s, dot) && all_digits(s + dot + 1, m - dot - 1)) {
        const char* ip = s; const int ni = dot; const char* fp = s + dot + 1; const int nf = m - dot - 1;
        if (ni > 1 && ip[0] == '0') return KIND_ODD;
        if (nf > 1 && fp[nf - 1] == '0') return KIND_ODD;
        int lead = 0;
        while (lead < ni + nf && (lead < ni ? ip[lead] : fp[lead - ni]) == '0') ++lead;
        const int sig = ni + nf - lead;
        if (sig > 15 || ni > 15) return KIND_ODD;
        if (sig == 0) return (nf == 1 && ni == 1) ? KIND_FLOAT : KIND_ODD;      // "0.0" / "-0.0"
        if (ni == 1 && ip[0] == '0') { int z = 0; while (z < nf && fp[z] == '0') ++z; if (z >= 4) return KIND_ODD; }
        return KIND_FLOAT;
    }
    if (TEXT_IS(s, m, "inf")) return KIND_FLOAT;
    const char c0 = f[0];
    if (is_dig(c0) || c0 == '+' || c0 == '-' || c0 == '.' || c0 == ' ' || c0 == 'i' || c0 == 'I' || c0 == 'n' || c0 == 'N') {
        if (n >= 72) return KIND_OTHER;
        if (strtod_takes_all(f, n)) return KIND_ODD;
    }
    if (TEXT_IS(f, n, "True") || TEXT_IS(f, n, "False") || TEXT_IS(f, n, "TRUE") || TEXT_IS(f, n, "FALSE") || TEXT_IS(f, n, "true") || TEXT_IS(f, n, "false")) return KIND_ODD;
    return KIND_OTHER;
}

struct TextRows {                                      // the rows of a formatted table: row i = text[off[i] + shift[tid of row i] ..) of len[i] bytes (0: no row)
    const char* text; const uint32_t* len; const uint64_t* off; const int64_t* shift; const SiteRec* sites; int64_t n;      // (sites = nullptr: rows in the text's own order, no shift)
};
__device__ __forceinline__ const char* row_text(const TextRows& t, int64_t i) { return t.text + (int64_t)t.off[i] + (t.sites ? t.shift[(int)(t.sites[i].key >> 32)] : 0); }

// per column, the OR of the kinds of its cells over every row (a '#' cuts the row as pandas' comment="#" does; columns past the row's
// last field hold a missing value)
__global__ __launch_bounds__(256) void k_text_kinds(TextRows t, int n_cols, uint32_t* kinds) {
    __shared__ uint32_t sh[64];
    if (threadIdx.x < 64) sh[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < t.n && t.len[i] > 0) {
        const char* r = row_text(t, i);
        int e = (int)t.len[i] - 1;                      // (without the newline)
        for (int q = 0; q < e; ++q) if (r[q] == '#') { e = q; break; }
        int f0 = 0;
        for (int c = 0; c < n_cols && r[0] != '#'; ++c) {      // (a line that starts with '#' is a comment)
            int k;
            if (f0 > e) k = KIND_NA;
            else {
                int f1 = f0;
                while (f1 < e && r[f1] != '\t') ++f1;
                k = text_kind(r + f0, f1 - f0);
                f0 = f1 + 1;
            }
            if ((sh[c] & (uint32_t)k) == 0) atomicOr(&sh[c], (uint32_t)k);
        }
    }
    __syncthreads();
    if (threadIdx.x < n_cols && sh[threadIdx.x]) atomicOr(&kinds[threadIdx.x], sh[threadIdx.x]);
}

// the rows step 3 can keep (calling._step3_survivors): FILTER free of the patterns of BaseCellCalling.step3.py:49-52 (chrM rows:
// "Min|LR|gnomAD|LC|RNA") / :60-84 (the others), Cell_types (field 6) not "Non-Cancer"; a row of fewer than 7 fields is not kept
__global__ __launch_bounds__(256) void k_text_survivors(TextRows t, uint32_t* len2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > t.n) return;
    uint32_t keep = 0;
    if (i < t.n && t.len[i] > 0 && row_text(t, i)[0] != '#') {
        const char* r = row_text(t, i);
        const int e = (int)t.len[i] - 1;
        int fo[8], fl[8], nf = 0, f0 = 0;
        while (nf < 8 && f0 <= e) { int f1 = f0; while (f1 < e && r[f1] != '\t') ++f1; fo[nf] = f0; fl[nf] = f1 - f0; ++nf; f0 = f1 + 1; }
        if (nf > 6) {
            const char* F = r + fo[5]; const int n = fl[5];
            const bool is_m = TEXT_IS(r + fo[0], fl[0], "chrM");
            const bool dead = is_m ? (TEXT_HAS(F, n, "Min") || TEXT_HAS(F, n, "LR") || TEXT_HAS(F, n, "gnomAD") || TEXT_HAS(F, n, "LC") || TEXT_HAS(F, n, "RNA"))
                                   : (TEXT_HAS(F, n, "Min_cell_types") || TEXT_HAS(F, n, "Noisy_site") || TEXT_HAS(F, n, "LC_Upstream") || TEXT_HAS(F, n, "LC_Downstream") ||
                                      TEXT_HAS(F, n, "RNA_editing_db") || TEXT_HAS(F, n, "PoN") || TEXT_HAS(F, n, "Cell_type_noise") || TEXT_HAS(F, n, "gnomAD"));
            if (!dead && !TEXT_IS(r + fo[6], fl[6], "Non-Cancer")) keep = t.len[i];
        }
    }
    len2[i] = keep;
}
__global__ __launch_bounds__(256) void k_text_copy_rows(TextRows t, const uint32_t* len2, const uint64_t* off2, const int64_t* shift2, char* dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.n || len2[i] == 0) return;
    const char* r = row_text(t, i);
    char* w = dst + (int64_t)off2[i] + shift2[(int)(t.sites[i].key >> 32)];
    for (uint32_t q = 0; q < len2[i]; ++q) w[q] = r[q];
}

std::vector<std::string> split_names(const char* joined, int n) {
    std::vector<std::string> out;
    const char* p = joined;
    for (int i = 0; i < n; ++i) {
        const char* e = strchr(p, '\n');
        if (!e) e = p + strlen(p);
        out.emplace_back(p, (size_t)(e - p));
        p = *e ? e + 1 : e;
    }
    return out;
}

} // namespace

int run_set_table_names(lsg_ctx* c, int32_t n_contigs, const char* contig_names, int32_t n_ct, const char* ct_names) {
    if (n_contigs != c->n_contigs) { set_error("lsg_set_table_names: %d contig names for %d contigs (lsg_set_contigs)", n_contigs, c->n_contigs); return -2; }
    if (n_ct < 1 || n_ct > LSG_MAX_CELLTYPES) { set_error("lsg_set_table_names: n_celltypes %d not in [1,%d]", n_ct, LSG_MAX_CELLTYPES); return -2; }
    const auto cn = split_names(contig_names, n_contigs), tn = split_names(ct_names, n_ct);
    // one buffer: contig offsets, cell-type offsets, contigs in Python string order, the names' bytes
    std::vector<uint32_t> coff(n_contigs + 1, 0), toff(n_ct + 1, 0);
    std::string ctxt, ttxt;
    for (int i = 0; i < n_contigs; ++i) { ctxt += cn[(size_t)i]; coff[(size_t)i + 1] = (uint32_t)ctxt.size(); }
    for (int i = 0; i < n_ct; ++i) { ttxt += tn[(size_t)i]; toff[(size_t)i + 1] = (uint32_t)ttxt.size(); }
    std::vector<int32_t> order(n_contigs);
    for (int i = 0; i < n_contigs; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cn[(size_t)x] < cn[(size_t)y]; });
    HostBlob b;
    b.add(coff.data(), coff.size() * 4);                 // (at 0: FmtArgs::contig_off is the buffer's start)
    const size_t at_ct_off = b.add(toff.data(), toff.size() * 4), at_order = b.add(order.data(), order.size() * 4), at_ctxt = b.add(ctxt.data(), ctxt.size()),
                 at_ttxt = b.add(ttxt.data(), ttxt.size());
    if (b.upload(c->tab_names, c->stream)) return -1;
    c->tab_n_contigs = n_contigs; c->tab_n_ct = n_ct;
    c->tab_ct_off_at = (uint32_t)at_ct_off; c->tab_order_at = (uint32_t)at_order; c->tab_contig_txt_at = (uint32_t)at_ctxt; c->tab_ct_txt_at = (uint32_t)at_ttxt;
    return 0;
}

// the limits of the allele key: 15 bits of contig index, 32 of 1-based position
static int allele_limits(lsg_ctx* c, const char* who) {
    if (c->n_contigs > LSG_ALLELE_MAX_TID) { set_error("%s: %d contigs, an allele key holds %d", who, c->n_contigs, LSG_ALLELE_MAX_TID); return -2; }
    for (int t = 0; t < c->n_contigs; ++t)
        if (c->contig_len[(size_t)t] >= (int64_t)1 << 32) { set_error("%s: contig %d is %lld long, an allele key holds positions below 2^32", who, t, (long long)c->contig_len[(size_t)t]); return -2; }
    return 0;
}

int run_format_table(lsg_ctx* c, int32_t table, int64_t* n_bytes) {
    if (n_bytes) *n_bytes = 0;
    if (table >= LSG_TABLE_SPLIT_BAM && table < LSG_TABLE_ALL_SLOTS) { set_error("lsg_format_table: table %d is made by lsg_split_bam / lsg_bgzf_compress / lsg_bam_index", table); return -2; }
    if (table < 0 || table >= LSG_TABLE_SLOTS) { set_error("lsg_format_table: no table %d", table); return -2; }
    if (table == LSG_TABLE_FASTQ) { set_error("lsg_format_table: table %d is made by lsg_bam_fastq", table); return -2; }
    if (!c->counted) { set_error("lsg_format_table: no count rows (lsg_pileup_count or lsg_load_counts first)"); return -2; }
    if (c->tab_n_contigs != c->n_contigs || c->tab_n_ct < c->n_ct) { set_error("lsg_format_table: lsg_set_table_names first (names of %d contigs and %d cell types)", c->n_contigs, c->n_ct); return -2; }
    if (table == LSG_TABLE_STEP3_ROWS) { set_error("lsg_format_table: table %d is made by lsg_step2_summary", table); return -2; }
    const bool counts = table < LSG_TABLE_MERGED;
    if (counts && table >= c->n_ct) { set_error("lsg_format_table: no cell type %d", table); return -2; }
    if (!counts && !c->called) { set_error("lsg_format_table: the merged and step-1 tables need lsg_call_step1 (its merged site list)"); return -2; }
    for (int t = 0; t < c->n_contigs; ++t)          // (REF of the count rows, the step-1 rows' contexts)
        if (!c->ref_ptr[t]) { set_error("lsg_format_table: reference of contig %d not loaded", t); return -2; }
    hipStream_t st = c->stream;
    // flat copies of the rows the table prints (kept until the next count)
    for (int ct = counts ? table : 0; ct < (counts ? table + 1 : c->n_ct); ++ct) {
        if (c->tab_rows_serial[ct] == c->count_serial) continue;
        if (int rc = run_export_rows(c, ct, c->tab_keys[ct], c->tab_refs[ct], c->tab_rows[ct])) return rc;
        c->tab_rows_serial[ct] = c->count_serial;
    }
    FmtArgs a{};
    a.kind = counts ? K_COUNTS : table == LSG_TABLE_MERGED ? K_MERGED : table == LSG_TABLE_STEP1 ? K_STEP1 : table == LSG_TABLE_STEP1_KEPT ? K_KEPT : K_STEP2;
    for (int q = 0; q < 3; ++q) { a.posset[q] = c->posset[q].keys.as<int64_t>(); a.n_posset[q] = c->posset[q].n; }
    a.alleles = c->alleleset.keys.as<int64_t>(); a.n_alleles = c->alleleset_loaded ? c->alleleset.n : -1;
    if (a.kind == K_STEP2 && a.n_alleles > 0)
        if (int rc = allele_limits(c, "lsg_format_table")) return rc;
    a.ct = counts ? table : 0; a.n_ct = c->n_ct; a.n_contigs = c->n_contigs;
    a.n = counts ? c->n_rows[table] : c->n_sites;
    for (int ct = 0; ct < c->n_ct; ++ct) {
        a.keys[ct] = c->tab_keys[ct].as<int64_t>(); a.refs[ct] = c->tab_refs[ct].as<uint8_t>(); a.rows[ct] = c->tab_rows[ct].as<uint32_t>();
        a.n_rows[ct] = c->n_rows[ct];
    }
    a.sites = c->d_calls.as<SiteRec>(); a.cands = c->ws[WS_CALL_CANDS].as<CandCt>();
    a.ref_ptr = c->d_ref_ptrs.as<const uint8_t*>(); a.contig_len = c->d_contig_len.as<int64_t>();
    const char* names = c->tab_names.as<char>();
    a.contig_off = reinterpret_cast<const uint32_t*>(names); a.ct_off = reinterpret_cast<const uint32_t*>(names + c->tab_ct_off_at);
    a.contig_txt = names + c->tab_contig_txt_at; a.ct_txt = names + c->tab_ct_txt_at;
    const int32_t* order = reinterpret_cast<const int32_t*>(names + c->tab_order_at);
    c->tab_bytes[table] = -1;
    c->tab_scratch_table = -1;
    if (a.n == 0) { c->tab_bytes[table] = 0; return 0; }
    if (a.n >= (int64_t)1 << 31) { set_error("lsg_format_table: %lld rows", (long long)a.n); return -2; }
    RowPlaces r;
    if (row_places(c->tab_scratch, a.n, c->n_contigs, r)) return -1;
    a.len = r.len; a.off = r.off; a.shift = r.shift;
    const unsigned blocks = (unsigned)((a.n + 1 + 255) / 256);
    hipLaunchKernelGGL(k_row_len, dim3(blocks), dim3(256), 0, st, a);
    int64_t bytes = 0;
    if (finish_places(c, r, &bytes, [&] { contig_order(a, r, order, st); return 0; })) return -1;
    if (print_table(c, table, bytes, [&](char* text) { a.text = text; hipLaunchKernelGGL(k_row_put, dim3(blocks), dim3(256), 0, st, a); })) return -1;
    c->tab_scratch_table = table; c->tab_scratch_rows = a.n;      // (the rows' places stay in the scratch: lsg_step2_summary reads the text by them)
    if (n_bytes) *n_bytes = bytes;
    return 0;
}

// k_text_kinds over rows that lie in the text's own order (hccv.hip: a table the caller uploaded): row i = text[off[i] ..) of len[i] bytes,
// its newline counted; kinds = 64 zeroed words on the device
void launch_text_kinds(const char* text, const uint32_t* len, const uint64_t* off, int64_t n, int n_cols, uint32_t* kinds, hipStream_t st) {
    const TextRows t{text, len, off, nullptr, nullptr, n};
    hipLaunchKernelGGL(k_text_kinds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t, n_cols, kinds);
}

// Count, then compact: the keys' places come from the same scan and contig shifts as a table's rows, with every query one unit long
int run_step2_allele_queries(lsg_ctx* c, int64_t* keys_out, int64_t capacity, int64_t* n_out) {
    *n_out = 0;
    if (!c->called) { set_error("lsg_step2_allele_queries: call lsg_call_step1 first"); return -2; }
    if (c->tab_n_contigs != c->n_contigs) { set_error("lsg_step2_allele_queries: lsg_set_table_names first (the rows' order is the contig names')"); return -2; }
    if (int rc = allele_limits(c, "lsg_step2_allele_queries")) return rc;
    const int64_t n = c->n_sites;
    if (n == 0) return 0;
    if (n >= (int64_t)1 << 31) { set_error("lsg_step2_allele_queries: %lld sites", (long long)n); return -2; }
    hipStream_t st = c->stream;
    FmtArgs a{};
    a.kind = K_KEPT; a.n_ct = c->n_ct; a.n_contigs = c->n_contigs; a.n = n;
    a.sites = c->d_calls.as<SiteRec>(); a.cands = c->ws[WS_CALL_CANDS].as<CandCt>();
    RowPlaces r;
    if (row_places(c->tab_scratch2, n, c->n_contigs, r)) return -1;
    a.len = r.len; a.off = r.off; a.shift = r.shift;
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(k_query_len, dim3(blocks), dim3(256), 0, st, a);
    const int32_t* order = reinterpret_cast<const int32_t*>(c->tab_names.as<char>() + c->tab_order_at);
    int64_t k = 0;
    if (finish_places(c, r, &k, [&] { contig_order(a, r, order, st); return 0; })) return -1;
    *n_out = k;
    if (!keys_out || k == 0) return 0;
    if (k > capacity) { set_error("lsg_step2_allele_queries: capacity %lld < %lld keys", (long long)capacity, (long long)k); return -2; }
    DevBuf dk;
    if (dk.reserve((size_t)k * 8)) return -1;
    hipLaunchKernelGGL(k_query_put, dim3(blocks), dim3(256), 0, st, a, dk.as<int64_t>());
    int rc = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(keys_out, dk.p, (size_t)k * 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = -1;
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    if (rc) set_error("lsg_step2_allele_queries: %s", hipGetErrorString(hipGetLastError()));
    dk.release();
    return rc;
}

// Column kinds of the step-2 text + its surviving rows as table LSG_TABLE_STEP3_ROWS
int run_step2_summary(lsg_ctx* c, int32_t n_cols, uint8_t* kinds, int64_t* n_survivor_bytes) {
    if (n_survivor_bytes) *n_survivor_bytes = 0;
    if (n_cols < 7 || n_cols > 64) { set_error("lsg_step2_summary: %d columns (7 to 64)", n_cols); return -2; }
    if (c->tab_bytes[LSG_TABLE_STEP2] < 0) { set_error("lsg_step2_summary: format table LSG_TABLE_STEP2 first"); return -2; }
    memset(kinds, 0, (size_t)n_cols);
    c->tab_bytes[LSG_TABLE_STEP3_ROWS] = -1;
    if (c->tab_bytes[LSG_TABLE_STEP2] == 0) { c->tab_bytes[LSG_TABLE_STEP3_ROWS] = 0; return 0; }
    if (c->tab_scratch_table != LSG_TABLE_STEP2 || c->tab_scratch_rows != c->n_sites || !c->called) { set_error("lsg_step2_summary: must follow the format of LSG_TABLE_STEP2 directly"); return -2; }
    hipStream_t st = c->stream;
    const int64_t n = c->tab_scratch_rows;
    RowPlaces r, r2;
    row_places(c->tab_scratch, n, c->n_contigs, r, false);            // where run_format_table left the rows' places
    TextRows t{c->tab_text[LSG_TABLE_STEP2].as<char>(), r.len, r.off, r.shift, c->d_calls.as<SiteRec>(), n};
    // second scratch: kinds[64], then the survivors' places (their contigs start where the table's do: its lo)
    if (row_places(c->tab_scratch2, n, c->n_contigs, r2, true, 256)) return -1;
    uint32_t* d_kinds = c->tab_scratch2.as<uint32_t>();
    LSG_HIP(hipMemsetAsync(d_kinds, 0, 256, st));
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(k_text_kinds, dim3(blocks), dim3(256), 0, st, t, (int)n_cols, d_kinds);
    hipLaunchKernelGGL(k_text_survivors, dim3(blocks), dim3(256), 0, st, t, r2.len);
    const int32_t* order = reinterpret_cast<const int32_t*>(c->tab_names.as<char>() + c->tab_order_at);
    uint32_t h_kinds[64];
    int64_t bytes = 0;
    if (finish_places(c, r2, &bytes, [&] {
            hipLaunchKernelGGL(k_contig_shift, dim3(1), dim3(1), 0, st, r.lo, r2.off, order, c->n_contigs, r2.shift);
            LSG_HIP(hipMemcpyAsync(h_kinds, d_kinds, 256, hipMemcpyDeviceToHost, st));
            return 0;
        })) return -1;
    for (int q = 0; q < n_cols; ++q) kinds[q] = (uint8_t)h_kinds[q];
    if (print_table(c, LSG_TABLE_STEP3_ROWS, bytes, [&](char* text) { hipLaunchKernelGGL(k_text_copy_rows, dim3(blocks), dim3(256), 0, st, t, r2.len, r2.off, r2.shift, text); })) return -1;
    if (n_survivor_bytes) *n_survivor_bytes = bytes;
    return 0;
}

static int table_ready(lsg_ctx* c, int32_t table, const char* who) {
    if (table < 0 || table >= LSG_TABLE_ALL_SLOTS || c->tab_bytes[table] < 0) { set_error("%s: table %d is not formatted (lsg_format_table)", who, table); return -2; }
    return 0;
}

int run_copy_table(lsg_ctx* c, int32_t table, char* dst, int64_t capacity) {
    if (int rc = table_ready(c, table, "lsg_copy_table")) return rc;
    const int64_t n = c->tab_bytes[table];
    if (capacity < n) { set_error("lsg_copy_table: capacity %lld < %lld bytes", (long long)capacity, (long long)n); return -2; }
    if (n == 0) return 0;
    LSG_HIP(hipMemcpyAsync(dst, c->tab_text[table].p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// device -> two pinned staging buffers -> pwrite at the file's end; the copy of piece i + 1 runs while piece i is written
int run_append_table(lsg_ctx* c, int32_t table, const char* path) {
    if (int rc = table_ready(c, table, "lsg_append_table")) return rc;
    const int64_t n = c->tab_bytes[table];
    const char* src = c->tab_text[table].as<char>();
    LSG_HIP(hipSetDevice(c->device));
    const int fd = open(path, O_WRONLY | O_CREAT, 0644);
    if (fd < 0) { set_error("lsg_append_table: cannot open %s", path); return -2; }
    off_t at = lseek(fd, 0, SEEK_END);
    if (n == 0) { close(fd); return 0; }
    const int64_t piece = (int64_t)32 << 20;
    hipStream_t st = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; char* buf[2] = {nullptr, nullptr};
    int rc = 0;
    auto fail = [&](const char* what) { set_error("lsg_append_table: %s", what); rc = -1; };
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) fail("no stream");
    for (int b = 0; b < 2 && !rc; ++b)
        if (hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) != hipSuccess || hipHostMalloc((void**)&buf[b], (size_t)std::min(piece, n), hipHostMallocDefault) != hipSuccess) fail("no pinned staging memory");
    const int64_t n_pieces = (n + piece - 1) / piece;
    auto issue = [&](int64_t i) {
        const int64_t b = i * piece, len = std::min(piece, n - b);
        if (hipMemcpyAsync(buf[i & 1], src + b, (size_t)len, hipMemcpyDeviceToHost, st) != hipSuccess || hipEventRecord(ev[i & 1], st) != hipSuccess) fail("device to host copy failed");
    };
    if (!rc) issue(0);
    for (int64_t i = 0; i < n_pieces && !rc; ++i) {
        if (i + 1 < n_pieces) issue(i + 1);
        if (rc) break;
        if (hipEventSynchronize(ev[i & 1]) != hipSuccess) { fail("device to host copy failed"); break; }
        const int64_t b = i * piece, len = std::min(piece, n - b);
        int64_t done = 0;
        while (done < len) {
            const ssize_t w = pwrite(fd, buf[i & 1] + done, (size_t)(len - done), at + (off_t)(b + done));
            if (w <= 0) { fail("write failed"); break; }
            done += w;
        }
    }
    if (st) (void)hipStreamSynchronize(st);
    for (int b = 0; b < 2; ++b) { if (buf[b]) (void)hipHostFree(buf[b]); if (ev[b]) (void)hipEventDestroy(ev[b]); }
    if (st) (void)hipStreamDestroy(st);
    if (close(fd) != 0 && !rc) fail("write failed");
    return rc;
}

int run_free_table(lsg_ctx* c, int32_t table) {
    if (table >= LSG_TABLE_ALL_SLOTS) { set_error("lsg_free_table: no table %d", table); return -2; }
    for (int t = 0; t < LSG_TABLE_ALL_SLOTS; ++t)
        if (table < 0 || t == table) { c->tab_text[t].release(); c->tab_bytes[t] = -1; }
    if (table < 0) {
        for (int ct = 0; ct < LSG_MAX_CELLTYPES; ++ct) { c->tab_keys[ct].release(); c->tab_refs[ct].release(); c->tab_rows[ct].release(); c->tab_rows_serial[ct] = 0; }
        c->tab_scratch.release(); c->tab_scratch2.release(); c->tab_scratch_table = -1;
        c->hccv.release();
    }
    return 0;
}

} // namespace lsg
