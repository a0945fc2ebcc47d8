// Step 3's final filters over the text of a step-2 table, where the text lies.
//
// Replaces BaseCellCalling.step3.py:41-316 (pandas reads the step-2 table, applies four Python functions to every row, string-sorts
// the PASS rows for the cluster test and writes two tables) for the fused run, where the rows step 3 can keep are resident
// (LSG_TABLE_STEP3_ROWS, lsg_step2_summary), and for a whole table the caller uploads.  The row rules are step3_core.h's, shared with the
// host twin (hostio/step3rows.cpp).  The architecture is hccv.hip's: the rows' starts from text_rows.h's newline passes, then one lane
// per row, twice - decide and measure (the counting sink), places from the lengths (text_table.h), print (the storing sink).  Between
// the two lies the cluster round trip: the PASS rows' "ordinal, INDEX" lines are printed into a compact export and copied to the host,
// step3_cluster.h finds the INDEX texts to tag, and they come back as sorted fixed-width records; every kept row's lane then searches
// them for its own INDEX (a row of any STEP3FILTER is tagged, as the reference tags by INDEX text) and corrects its lengths.  An empty
// set skips that kernel.  Both tables hold their chrM rows last (chrm_last).
#include "lsg_ctx.h"
#include "step3_cluster.h"
#include "text_rows.h"
#include "text_sink.h"
#include "text_table.h"
#include <chrono>
#include <cstring>
#include <vector>

namespace lsg {
void launch_text_kinds(const char* text, const uint32_t* len, const uint64_t* off, int64_t n, int n_cols, uint32_t* kinds, hipStream_t st);      // tables.hip

namespace {

enum { RF_KEPT = 1, RF_CHRM = 2, RF_PASS = 4 };       // per row, beside its tags
enum { CT_ALL = 0, CT_PASS, CT_UNDECIDED, CT_CLUSTERED_PASS, CT_WORDS };
enum { P_ALL = 0, P_ALL_M, P_PASS, P_PASS_M, P_EXPORT, P_SCANS };       // the scans: bytes in the unfiltered table, ... if chrM, in the final table, ... if chrM, in the export
struct Step3Args {
    const char* text; const uint64_t* starts; int64_t n;
    lsg_step3_params p;
    uint32_t* row_len;                                // the row's bytes, its newline counted (k_text_kinds reads it)
    uint32_t* len[P_SCANS]; const uint64_t* off[P_SCANS];
    uint8_t* flags; uint16_t* tags;
    unsigned long long* counts;                       // CT_* tallies
    unsigned long long* first_bad;                    // min over undecided rows of ordinal << 8 | reason
    const uint8_t* recs; int64_t n_recs;              // the cluster set
    char* out_all; char* out_pass; char* out_export;
};

__device__ __forceinline__ int row_bytes(const Step3Args& a, int64_t i) { return (int)(a.starts[i + 1] - a.starts[i]) - 1; }

__global__ __launch_bounds__(256) void k_step3_decide(Step3Args a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t la = 0, le = 0; int fate = lsg3::DROPPED; bool is_m = false, pass = false; uint32_t tags = 0;
    if (i < a.n) {
        const char* r = a.text + a.starts[i];
        const uint64_t span = a.starts[i + 1] - a.starts[i];
        const int n = span > (1u << 30) ? 0 : (int)span - 1;
        a.row_len[i] = (uint32_t)(n + 1);
        lsg3::Row st;
        fate = lsg3::decide(r, n, a.p, st);
        if (span > (1u << 30)) { fate = st.fate = lsg3::UNDECIDED; st.reason = LSG_HCCV_TOO_LONG; }
        if (fate == lsg3::KEPT) {
            is_m = st.is_m != 0; tags = st.tags; pass = tags == 0;
            LenSink s; lsg3::print_row(s, r, n, a.p, st, tags); la = s.n;
            if (pass) { LenSink e; lsg3::print_export(e, r, st, i); le = e.n; }
        }
        if (fate == lsg3::UNDECIDED) atomicMin(a.first_bad, ((unsigned long long)i << 8) | st.reason);
    }
    if (i <= a.n) {                                   // (entry n: the scans' total)
        a.len[P_ALL][i] = la; a.len[P_ALL_M][i] = is_m ? la : 0u; a.len[P_PASS][i] = pass ? la : 0u; a.len[P_PASS_M][i] = (pass && is_m) ? la : 0u; a.len[P_EXPORT][i] = le;
        if (i < a.n) { a.flags[i] = (uint8_t)((la ? RF_KEPT : 0) | (is_m ? RF_CHRM : 0) | (pass ? RF_PASS : 0)); a.tags[i] = (uint16_t)tags; }
    }
    wave_tally(a.counts + CT_ALL, la > 0); wave_tally(a.counts + CT_PASS, pass); wave_tally(a.counts + CT_UNDECIDED, fate == lsg3::UNDECIDED);
}

__global__ __launch_bounds__(256) void k_step3_export(Step3Args a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || a.len[P_EXPORT][i] == 0) return;
    const char* r = a.text + a.starts[i];
    lsg3::Row st;
    lsg3::decide(r, row_bytes(a, i), a.p, st);
    PutSink s{a.out_export + (int64_t)a.off[P_EXPORT][i]};
    lsg3::print_export(s, r, st, i);
}

// every kept row whose INDEX is in the cluster set: tagged, no PASS row any more, its lengths corrected
__global__ __launch_bounds__(256) void k_step3_cluster(Step3Args a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool hit = false, was_pass = false;
    if (i < a.n && (a.flags[i] & RF_KEPT)) {
        const char* r = a.text + a.starts[i];
        lsg3::Row st;
        lsg3::decide(r, row_bytes(a, i), a.p, st);
        uint8_t key[lsg3::INDEX_REC];
        hit = lsg3::index_record(r, st, key) && lsg3::in_records(a.recs, a.n_recs, key);
        if (hit) {
            const uint8_t f = a.flags[i];
            const uint32_t tags = a.tags[i];
            const uint32_t la = a.len[P_ALL][i] + lsg3::clust_tag_len(tags, a.p.clust_dist);
            was_pass = (f & RF_PASS) != 0;
            a.tags[i] = (uint16_t)(tags | lsg3::T_CLUST);
            a.flags[i] = (uint8_t)(f & ~RF_PASS);
            a.len[P_ALL][i] = la; if (f & RF_CHRM) a.len[P_ALL_M][i] = la;
            a.len[P_PASS][i] = 0; a.len[P_PASS_M][i] = 0;
        }
    }
    wave_tally(a.counts + CT_CLUSTERED_PASS, hit && was_pass);
}

__global__ __launch_bounds__(256) void k_step3_print(Step3Args a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || !(a.flags[i] & RF_KEPT)) return;
    const char* r = a.text + a.starts[i];
    const int n = row_bytes(a, i);
    lsg3::Row st;
    lsg3::decide(r, n, a.p, st);
    const bool is_m = (a.flags[i] & RF_CHRM) != 0;
    const uint32_t tags = a.tags[i];
    { PutSink s{a.out_all + chrm_last(a.off[P_ALL], a.off[P_ALL_M], i, a.n, is_m)}; lsg3::print_row(s, r, n, a.p, st, tags); }
    if (a.flags[i] & RF_PASS) { PutSink s{a.out_pass + chrm_last(a.off[P_PASS], a.off[P_PASS_M], i, a.n, is_m)}; lsg3::print_row(s, r, n, a.p, st, tags); }
}

// the filter over n_bytes of text on the device (256-byte aligned, its buffer padded to whole 16 bytes)
int run_step3_rows(lsg_ctx* c, const char* text, int64_t n_bytes, const lsg_step3_params* p, lsg_step3_info* info, bool want_kinds) {
    hipStream_t st = c->stream;
    const int tab[2] = {LSG_TABLE_STEP3_ALL, LSG_TABLE_STEP3_PASS};
    for (int t : tab) c->tab_bytes[t] = -1;
    if (n_bytes == 0) { for (int t : tab) c->tab_bytes[t] = 0; return 0; }
    PhaseTimer t_rows(st), t_decide(st), t_print(st);
    // ---- the rows' starts
    t_rows.start();
    int64_t n = 0;
    if (int rc = find_row_starts(c, c->hccv.pieces, c->hccv.starts, text, n_bytes, "lsg_step3_filter", &n)) return rc;
    t_rows.stop();
    info->rows_in = n;
    // ---- decide and measure
    RowPlaces r[P_SCANS];
    for (int q = 0; q < P_SCANS; ++q) if (row_places(c->hccv.places[q], n, -1, r[q])) return -1;
    const size_t at_flags = align_up((size_t)(n + 1) * 4, 256), at_tags = at_flags + align_up((size_t)n, 256), at_small = at_tags + align_up((size_t)n * 2, 256);
    if (c->hccv.rows.reserve(at_small + 256 + 64 * 4)) return -1;
    char* rows = c->hccv.rows.as<char>();
    Step3Args a{};
    a.text = text; a.starts = c->hccv.starts.as<uint64_t>(); a.n = n; a.p = *p;
    a.row_len = reinterpret_cast<uint32_t*>(rows); a.flags = reinterpret_cast<uint8_t*>(rows + at_flags); a.tags = reinterpret_cast<uint16_t*>(rows + at_tags);
    a.counts = reinterpret_cast<unsigned long long*>(rows + at_small); a.first_bad = a.counts + CT_WORDS;
    uint32_t* d_kinds = reinterpret_cast<uint32_t*>(rows + at_small + 256);
    for (int q = 0; q < P_SCANS; ++q) { a.len[q] = r[q].len; a.off[q] = r[q].off; }
    LSG_HIP(hipMemsetAsync(a.counts, 0, 256 + 64 * 4, st));
    LSG_HIP(hipMemsetAsync(a.first_bad, 0xFF, 8, st));
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    t_decide.start();
    hipLaunchKernelGGL(k_step3_decide, dim3(blocks), dim3(256), 0, st, a);
    t_decide.stop();
    LSG_HIP(hipGetLastError());
    if (want_kinds) launch_text_kinds(text, a.row_len, a.starts, n, p->n_cols, d_kinds, st);
    int64_t total[P_SCANS];
    if (finish_places(c, r[P_EXPORT], &total[P_EXPORT])) return -1;
    unsigned long long h_small[CT_WORDS + 1]; uint32_t h_kinds[64];
    LSG_HIP(hipMemcpyAsync(h_small, a.counts, sizeof h_small, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(h_kinds, d_kinds, sizeof h_kinds, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipStreamSynchronize(st));
    if (want_kinds) for (int q = 0; q < 64; ++q) info->kinds[q] = (uint8_t)h_kinds[q];
    info->ms_rows = t_rows.ms(); info->ms_decide = t_decide.ms();
    info->n_undecided = (int64_t)h_small[CT_UNDECIDED];
    if (info->n_undecided) { info->first_undecided = (int64_t)(h_small[CT_WORDS] >> 8); info->reason = (int32_t)(h_small[CT_WORDS] & 0xFF); return 0; }
    info->rows_pass_unclustered = (int64_t)h_small[CT_PASS];
    // ---- the cluster round trip: the PASS rows' INDEX texts out, the set of those to tag back
    const auto t0 = std::chrono::steady_clock::now();
    int64_t n_clustered_pass = 0;
    if (total[P_EXPORT] > 0) {
        if (c->hccv.exported.reserve((size_t)total[P_EXPORT])) return -1;
        a.out_export = c->hccv.exported.as<char>();
        hipLaunchKernelGGL(k_step3_export, dim3(blocks), dim3(256), 0, st, a);
        LSG_HIP(hipGetLastError());
        std::vector<char> h_export((size_t)total[P_EXPORT]);
        LSG_HIP(hipMemcpyAsync(h_export.data(), a.out_export, h_export.size(), hipMemcpyDeviceToHost, st));
        LSG_HIP(hipStreamSynchronize(st));
        std::vector<uint8_t> recs;
        int64_t bad = -1; int why = 0;
        if (lsg3::cluster_records(h_export.data(), h_export.size(), p->clust_dist, recs, &bad, &why)) {
            info->n_undecided = 1; info->first_undecided = bad; info->reason = why;
            return 0;
        }
        info->n_clustered = (int64_t)(recs.size() / lsg3::INDEX_REC);
        if (!recs.empty()) {
            if (c->hccv.cluster_set.reserve(recs.size())) return -1;
            LSG_HIP(hipMemcpyAsync(c->hccv.cluster_set.p, recs.data(), recs.size(), hipMemcpyHostToDevice, st));
            a.recs = c->hccv.cluster_set.as<uint8_t>(); a.n_recs = info->n_clustered;
            hipLaunchKernelGGL(k_step3_cluster, dim3(blocks), dim3(256), 0, st, a);
            LSG_HIP(hipGetLastError());
            unsigned long long h_hit = 0;
            LSG_HIP(hipMemcpyAsync(&h_hit, a.counts + CT_CLUSTERED_PASS, 8, hipMemcpyDeviceToHost, st));
            LSG_HIP(hipStreamSynchronize(st));         // (recs and h_hit are this frame's)
            n_clustered_pass = (int64_t)h_hit;
        }
    }
    info->ms_cluster = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // ---- places
    for (int q = 0; q < P_EXPORT; ++q) if (finish_places(c, r[q], &total[q])) return -1;
    info->rows_all = (int64_t)h_small[CT_ALL]; info->rows_pass = (int64_t)h_small[CT_PASS] - n_clustered_pass;
    info->bytes_all = total[P_ALL]; info->bytes_pass = total[P_PASS];
    // ---- print
    const int64_t bytes[2] = {total[P_ALL], total[P_PASS]};
    for (int q = 0; q < 2; ++q) if (bytes[q] > 0 && c->tab_text[tab[q]].reserve((size_t)bytes[q])) return -1;
    a.out_all = c->tab_text[tab[0]].as<char>(); a.out_pass = c->tab_text[tab[1]].as<char>();
    if (total[P_ALL] > 0) {
        t_print.start();
        hipLaunchKernelGGL(k_step3_print, dim3(blocks), dim3(256), 0, st, a);
        t_print.stop();
        LSG_HIP(hipGetLastError());
        LSG_HIP(hipStreamSynchronize(st));
        info->ms_print = t_print.ms();
    }
    for (int q = 0; q < 2; ++q) c->tab_bytes[tab[q]] = bytes[q];
    return 0;
}

int check_params(const lsg_step3_params* p, const char* who) {
    if (p->n_cols < 1 || p->n_cols > 64) { set_error("%s: %d columns (1 to 64)", who, p->n_cols); return -2; }
    for (int k = 0; k < LSG_STEP3_COLS; ++k)
        if (p->col[k] >= p->n_cols || (p->col[k] < 0 && !(k == lsg3::C_NONCANCER && p->col[k] == -1))) { set_error("%s: column %d of %d", who, p->col[k], p->n_cols); return -2; }
    return 0;
}

} // namespace

int run_step3_filter(lsg_ctx* c, const lsg_step3_params* p, lsg_step3_info* info) {
    memset(info, 0, sizeof *info);
    info->first_undecided = -1;
    if (int rc = check_params(p, "lsg_step3_filter")) return rc;
    if (c->tab_bytes[LSG_TABLE_STEP3_ROWS] < 0) { set_error("lsg_step3_filter: lsg_step2_summary first (table LSG_TABLE_STEP3_ROWS)"); return -2; }
    return run_step3_rows(c, c->tab_text[LSG_TABLE_STEP3_ROWS].as<char>(), c->tab_bytes[LSG_TABLE_STEP3_ROWS], p, info, false);
}

int run_step3_filter_text(lsg_ctx* c, const char* text, int64_t n_bytes, const lsg_step3_params* p, lsg_step3_info* info) {
    memset(info, 0, sizeof *info);
    info->first_undecided = -1;
    if (int rc = check_params(p, "lsg_step3_filter_text")) return rc;
    const int64_t at = skip_comment_lines(text, n_bytes);
    text += at; n_bytes -= at;
    if (int rc = upload_text(c, c->hccv.text, text, n_bytes, "lsg_step3_filter_text")) return rc;
    return run_step3_rows(c, c->hccv.text.as<char>(), n_bytes, p, info, true);
}

} // namespace lsg
