// The high-confidence cancer variant filter over the text of a step-2 table, where the text lies.
//
// Replaces HCCV_SNV of workflow/scripts/CellTypeReannotation/HighConfidenceCancerVariants.py:8-88 (pandas reads the whole pass-1 step-2
// table and applies three Python functions to every row) for the fused re-annotation run, where that table was printed on the device
// and is still resident (tables.hip, LSG_TABLE_STEP2), and for a table the caller uploads.  The row rules are hccv_core.h's, shared
// with the host twin (hostio/hccvrows.cpp).  Both entries run the same kernels over the same form of input - the text and the place of
// every row's first byte, found by text_rows.h's newline passes
// (the resident table's rows lie contig after contig in the names' order, which its format's scratch does not index in: reading the
// newlines again costs one pass over the text and leaves that scratch, and lsg_step2_summary's, alone).  Then one lane per row, twice,
// like every table here: decide and measure (text_core.h's counting sink), places from the lengths (text_table.h), print (the storing
// sink).  .HCCV.tsv3 holds its chrM rows last: a row's place there is its place among the rows of its own kind, the chrM rows shifted
// behind all others.
#include "lsg_ctx.h"
#include "hccv_core.h"
#include "text_rows.h"
#include "text_sink.h"
#include "text_table.h"
#include <cstring>

namespace lsg {
void launch_text_kinds(const char* text, const uint32_t* len, const uint64_t* off, int64_t n, int n_cols, uint32_t* kinds, hipStream_t st);      // tables.hip

namespace {

// what the decide pass leaves per row besides the lengths
enum { RF_CHRM = 1, RF_PASS = 2 };
enum { CT_TSV2 = 0, CT_TSV3, CT_PASS, CT_UNDECIDED, CT_WORDS };
struct HccvArgs {
    const char* text; const uint64_t* starts; int64_t n;
    lsg_hccv_params p;
    uint32_t* row_len;                                // the row's bytes, its newline counted (k_text_kinds reads it)
    uint32_t* len2; uint32_t* len3; uint32_t* len3m; uint32_t* lenp; uint32_t* lenpm;      // bytes in .tsv2, .tsv3, .tsv3 if chrM, PASS, PASS if chrM
    const uint64_t* off2; const uint64_t* off3; const uint64_t* off3m; const uint64_t* offp; const uint64_t* offpm;
    uint8_t* flags;
    unsigned long long* counts;                       // CT_* tallies
    unsigned long long* first_bad;                    // min over undecided rows of ordinal << 8 | reason
    char* out2; char* out3; char* outp;
};

__global__ __launch_bounds__(256) void k_hccv_decide(HccvArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t l2 = 0, l3 = 0; int stage = lsgh::DROP_CELL_TYPES; bool is_m = false, pass = false;
    if (i < a.n) {
        const char* r = a.text + a.starts[i];
        const uint64_t span = a.starts[i + 1] - a.starts[i];
        const int n = span > (1u << 30) ? 0 : (int)span - 1;
        a.row_len[i] = (uint32_t)(n + 1);
        lsgh::Row st;
        stage = lsgh::decide(r, n, a.p, st);
        if (span > (1u << 30)) { stage = st.stage = lsgh::UNDECIDED; st.reason = LSG_HCCV_TOO_LONG; }
        is_m = st.is_m != 0;
        if (stage == lsgh::IN_TSV2 || stage == lsgh::IN_TSV3) { LenSink s; lsgh::print_row(s, r, n, a.p, st, false); l2 = s.n; }
        if (stage == lsgh::IN_TSV3) { int k; lsgh::verdict_name(st.verdict, k); l3 = l2 + 1u + (uint32_t)k; pass = st.verdict == lsgh::V_PASS; }
        if (stage == lsgh::UNDECIDED) atomicMin(a.first_bad, ((unsigned long long)i << 8) | st.reason);
    }
    if (i <= a.n) {                                   // (entry n: the scans' total)
        a.len2[i] = l2; a.len3[i] = l3; a.len3m[i] = is_m ? l3 : 0u; a.lenp[i] = pass ? l3 : 0u; a.lenpm[i] = (pass && is_m) ? l3 : 0u;
        if (i < a.n) a.flags[i] = (uint8_t)((is_m ? RF_CHRM : 0) | (pass ? RF_PASS : 0));
    }
    wave_tally(a.counts + CT_TSV2, l2 > 0); wave_tally(a.counts + CT_TSV3, l3 > 0); wave_tally(a.counts + CT_PASS, pass); wave_tally(a.counts + CT_UNDECIDED, stage == lsgh::UNDECIDED);
}

__global__ __launch_bounds__(256) void k_hccv_print(HccvArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || a.len2[i] == 0) return;
    const char* r = a.text + a.starts[i];
    const int n = (int)(a.starts[i + 1] - a.starts[i]) - 1;
    lsgh::Row st;
    lsgh::decide(r, n, a.p, st);
    { PutSink s{a.out2 + (int64_t)a.off2[i]}; lsgh::print_row(s, r, n, a.p, st, false); }
    if (a.len3[i] == 0) return;
    const bool is_m = (a.flags[i] & RF_CHRM) != 0;
    { PutSink s{a.out3 + chrm_last(a.off3, a.off3m, i, a.n, is_m)}; lsgh::print_row(s, r, n, a.p, st, true); }
    if (a.flags[i] & RF_PASS) { PutSink s{a.outp + chrm_last(a.offp, a.offpm, i, a.n, is_m)}; lsgh::print_row(s, r, n, a.p, st, true); }
}

// the filter over n_bytes of text on the device (256-byte aligned, its buffer padded to whole 16 bytes)
int run_hccv_rows(lsg_ctx* c, const char* text, int64_t n_bytes, const lsg_hccv_params* p, lsg_hccv_info* info, bool want_kinds) {
    hipStream_t st = c->stream;
    for (int t : {LSG_TABLE_HCCV2, LSG_TABLE_HCCV3, LSG_TABLE_HCCV_PASS}) c->tab_bytes[t] = -1;
    if (n_bytes == 0) { for (int t : {LSG_TABLE_HCCV2, LSG_TABLE_HCCV3, LSG_TABLE_HCCV_PASS}) c->tab_bytes[t] = 0; return 0; }
    PhaseTimer t_rows(st), t_decide(st), t_print(st);
    // ---- the rows' starts
    t_rows.start();
    int64_t n = 0;
    if (int rc = find_row_starts(c, c->hccv.pieces, c->hccv.starts, text, n_bytes, "lsg_hccv_filter", &n)) return rc;
    t_rows.stop();
    info->rows_in = n;
    // ---- decide and measure
    RowPlaces r[5];
    for (int q = 0; q < 5; ++q) if (row_places(c->hccv.places[q], n, -1, r[q])) return -1;
    const size_t at_flags = align_up((size_t)(n + 1) * 4, 256), at_small = at_flags + align_up((size_t)n, 256);
    if (c->hccv.rows.reserve(at_small + 256 + 64 * 4)) return -1;
    char* rows = c->hccv.rows.as<char>();
    HccvArgs a{};
    a.text = text; a.starts = c->hccv.starts.as<uint64_t>(); a.n = n; a.p = *p;
    a.row_len = reinterpret_cast<uint32_t*>(rows); a.flags = reinterpret_cast<uint8_t*>(rows + at_flags);
    a.counts = reinterpret_cast<unsigned long long*>(rows + at_small); a.first_bad = a.counts + CT_WORDS;
    uint32_t* d_kinds = reinterpret_cast<uint32_t*>(rows + at_small + 256);
    a.len2 = r[0].len; a.len3 = r[1].len; a.len3m = r[2].len; a.lenp = r[3].len; a.lenpm = r[4].len;
    a.off2 = r[0].off; a.off3 = r[1].off; a.off3m = r[2].off; a.offp = r[3].off; a.offpm = r[4].off;
    LSG_HIP(hipMemsetAsync(a.counts, 0, 256 + 64 * 4, st));
    LSG_HIP(hipMemsetAsync(a.first_bad, 0xFF, 8, st));
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    t_decide.start();
    hipLaunchKernelGGL(k_hccv_decide, dim3(blocks), dim3(256), 0, st, a);
    t_decide.stop();
    LSG_HIP(hipGetLastError());
    if (want_kinds) launch_text_kinds(text, a.row_len, a.starts, n, p->n_cols, d_kinds, st);
    int64_t total[5];
    for (int q = 0; q < 5; ++q) if (finish_places(c, r[q], &total[q])) return -1;
    unsigned long long h_small[CT_WORDS + 1]; uint32_t h_kinds[64];
    LSG_HIP(hipMemcpyAsync(h_small, a.counts, sizeof h_small, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(h_kinds, d_kinds, sizeof h_kinds, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipStreamSynchronize(st));
    if (want_kinds) for (int q = 0; q < 64; ++q) info->kinds[q] = (uint8_t)h_kinds[q];
    info->ms_rows = t_rows.ms(); info->ms_decide = t_decide.ms();
    info->n_undecided = (int64_t)h_small[CT_UNDECIDED];
    if (info->n_undecided) { info->first_undecided = (int64_t)(h_small[CT_WORDS] >> 8); info->reason = (int32_t)(h_small[CT_WORDS] & 0xFF); return 0; }
    info->rows_tsv2 = (int64_t)h_small[CT_TSV2]; info->rows_tsv3 = (int64_t)h_small[CT_TSV3]; info->rows_pass = (int64_t)h_small[CT_PASS];
    info->bytes_tsv2 = total[0]; info->bytes_tsv3 = total[1]; info->bytes_pass = total[3];
    // ---- print
    const int tab[3] = {LSG_TABLE_HCCV2, LSG_TABLE_HCCV3, LSG_TABLE_HCCV_PASS};
    const int64_t bytes[3] = {total[0], total[1], total[3]};
    for (int q = 0; q < 3; ++q) if (bytes[q] > 0 && c->tab_text[tab[q]].reserve((size_t)bytes[q])) return -1;
    a.out2 = c->tab_text[tab[0]].as<char>(); a.out3 = c->tab_text[tab[1]].as<char>(); a.outp = c->tab_text[tab[2]].as<char>();
    if (total[0] > 0) {
        t_print.start();
        hipLaunchKernelGGL(k_hccv_print, dim3(blocks), dim3(256), 0, st, a);
        t_print.stop();
        LSG_HIP(hipGetLastError());
        LSG_HIP(hipStreamSynchronize(st));
        info->ms_print = t_print.ms();
    }
    for (int q = 0; q < 3; ++q) c->tab_bytes[tab[q]] = bytes[q];
    return 0;
}

int check_params(const lsg_hccv_params* p, const char* who) {
    if (p->n_cols < 1 || p->n_cols > 64) { set_error("%s: %d columns (1 to 64)", who, p->n_cols); return -2; }
    for (int k = 0; k < LSG_HCCV_COLS; ++k)
        if (p->col[k] < 0 || p->col[k] >= p->n_cols) { set_error("%s: column %d of %d", who, p->col[k], p->n_cols); return -2; }
    return 0;
}

} // namespace

int run_hccv_filter(lsg_ctx* c, const lsg_hccv_params* p, lsg_hccv_info* info) {
    memset(info, 0, sizeof *info);
    info->first_undecided = -1;
    if (int rc = check_params(p, "lsg_hccv_filter")) return rc;
    if (c->tab_bytes[LSG_TABLE_STEP2] < 0) { set_error("lsg_hccv_filter: format table LSG_TABLE_STEP2 first"); return -2; }
    return run_hccv_rows(c, c->tab_text[LSG_TABLE_STEP2].as<char>(), c->tab_bytes[LSG_TABLE_STEP2], p, info, false);
}

int run_hccv_filter_text(lsg_ctx* c, const char* text, int64_t n_bytes, const lsg_hccv_params* p, lsg_hccv_info* info) {
    memset(info, 0, sizeof *info);
    info->first_undecided = -1;
    if (int rc = check_params(p, "lsg_hccv_filter_text")) return rc;
    const int64_t at = skip_comment_lines(text, n_bytes);
    text += at; n_bytes -= at;
    if (int rc = upload_text(c, c->hccv.text, text, n_bytes, "lsg_hccv_filter_text")) return rc;
    return run_hccv_rows(c, c->hccv.text.as<char>(), n_bytes, p, info, true);
}

} // namespace lsg
