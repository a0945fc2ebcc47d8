// The host twin of lsg_step3_filter_text (csrc/step3.hip; the semantics are in include/longsom_hip.h): the same row code (step3_core.h)
// and the same cluster test (step3_cluster.h) over a step-2 table in host memory, the same two row sets and the same undecided report.
// What pins the row code where there is no GPU, and what the device's tables are compared with.  Two passes like the device's: every
// row decided and measured, the cluster set from the PASS rows' INDEX texts, the places from the lengths, every kept row printed at its
// place; rows are shared out over threads in contiguous pieces.  (tsvstep3.cpp's lsio_step3_rows is the older native step 3 that
// calling.step3 runs; it keeps its own row functions.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../step3_cluster.h"

extern "C" int lsio_step3_column_kinds(const char* text, int64_t n_bytes, int32_t n_cols, uint8_t* kinds);

namespace {
thread_local char g_s3c_err[256];

struct Measured { uint32_t len; uint16_t tags; uint8_t fate, is_m, reason; };

template <class F> void over_rows(size_t n, F fn) {
    const unsigned T = n < 4096 ? 1u : std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (T == 1) { fn(0, n); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back([=] { fn(n * t / T, n * (t + 1) / T); });
    for (auto& x : th) x.join();
}
} // namespace

extern "C" {

const char* lsio_step3_core_last_error(void) { return g_s3c_err; }

// text: the step-2 table (leading lines that start with '#' are skipped).  *out_all, *out_pass: the rows of calling.step3.unfiltered.tsv
// and calling.step3.tsv, malloc'd (lsio_free_text), their sizes in info; none is made when info->n_undecided > 0.  0, or < 0.
int lsio_step3_core_rows(const char* text, int64_t n_bytes, const lsg_step3_params* p, lsg_step3_info* info, char** out_all, char** out_pass) {
    if (!text || n_bytes < 0 || !p || !info || !out_all || !out_pass || p->n_cols < 1 || p->n_cols > 64) {
        snprintf(g_s3c_err, sizeof g_s3c_err, "lsio_step3_core_rows: bad arguments"); return -1;
    }
    for (int k = 0; k < LSG_STEP3_COLS; ++k)
        if (p->col[k] >= p->n_cols || (p->col[k] < 0 && !(k == lsg3::C_NONCANCER && p->col[k] == -1))) { snprintf(g_s3c_err, sizeof g_s3c_err, "lsio_step3_core_rows: column %d of %d", p->col[k], p->n_cols); return -1; }
    *out_all = *out_pass = nullptr;
    memset(info, 0, sizeof *info);
    info->first_undecided = -1;
    try {
        int64_t at = 0;
        while (at < n_bytes && text[at] == '#') { const void* e = memchr(text + at, '\n', (size_t)(n_bytes - at)); at = e ? (const char*)e - text + 1 : n_bytes; }
        const char* t = text + at; const int64_t nb = n_bytes - at;
        if (lsio_step3_column_kinds(t, nb, p->n_cols, info->kinds) != 0) { snprintf(g_s3c_err, sizeof g_s3c_err, "lsio_step3_core_rows: column kinds failed"); return -2; }
        std::vector<int64_t> start;
        for (int64_t a = 0; a < nb;) { start.push_back(a); const void* e = memchr(t + a, '\n', (size_t)(nb - a)); a = e ? (const char*)e - t + 1 : nb; }
        const size_t n = start.size();
        start.push_back(nb + ((nb > 0 && t[nb - 1] != '\n') ? 1 : 0));           // (every row then ends one byte before the next one's start)
        for (size_t i = 0; i < n; ++i) if (start[i + 1] - start[i] - 1 > (int64_t)1 << 30) { snprintf(g_s3c_err, sizeof g_s3c_err, "lsio_step3_core_rows: a row of more than 2^30 bytes"); return -1; }
        info->rows_in = (int64_t)n;
        std::vector<Measured> m(n);
        over_rows(n, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                const char* r = t + start[i]; const int len = (int)(start[i + 1] - start[i] - 1);
                lsg3::Row st;
                lsg3::decide(r, len, *p, st);
                Measured& o = m[i];
                o = Measured{0, st.tags, st.fate, st.is_m, st.reason};
                if (st.fate == lsg3::KEPT) { lsg3::LenSink s; lsg3::print_row(s, r, len, *p, st, st.tags); o.len = s.n; }
            }
        });
        for (size_t i = 0; i < n; ++i)
            if (m[i].fate == lsg3::UNDECIDED && !info->n_undecided++) { info->first_undecided = (int64_t)i; info->reason = m[i].reason; }
        if (info->n_undecided) return 0;
        // the cluster test over the PASS rows' export, and every kept row looked up in its answer
        std::string exported;
        for (size_t i = 0; i < n; ++i) {
            if (m[i].fate != lsg3::KEPT || m[i].tags) continue;
            ++info->rows_pass_unclustered;
            const char* r = t + start[i];
            lsg3::Row st;
            lsg3::decide(r, (int)(start[i + 1] - start[i] - 1), *p, st);
            lsg3::LenSink k; lsg3::print_export(k, r, st, (int64_t)i);
            const size_t w = exported.size();
            exported.resize(w + k.n);
            lsg3::PutSink s{&exported[w]}; lsg3::print_export(s, r, st, (int64_t)i);
        }
        std::vector<uint8_t> recs;
        if (!exported.empty()) {
            int64_t bad = -1; int why = 0;
            if (lsg3::cluster_records(exported.data(), exported.size(), p->clust_dist, recs, &bad, &why)) { info->n_undecided = 1; info->first_undecided = bad; info->reason = why; return 0; }
        }
        info->n_clustered = (int64_t)(recs.size() / lsg3::INDEX_REC);
        if (!recs.empty())
            over_rows(n, [&](size_t lo, size_t hi) {
                for (size_t i = lo; i < hi; ++i) {
                    Measured& o = m[i];
                    if (o.fate != lsg3::KEPT) continue;
                    const char* r = t + start[i];
                    lsg3::Row st;
                    lsg3::decide(r, (int)(start[i + 1] - start[i] - 1), *p, st);
                    uint8_t key[lsg3::INDEX_REC];
                    if (!lsg3::index_record(r, st, key) || !lsg3::in_records(recs.data(), info->n_clustered, key)) continue;
                    o.len += lsg3::clust_tag_len(o.tags, p->clust_dist);
                    o.tags |= lsg3::T_CLUST;
                }
            });
        // places: both tables hold the chrM rows last
        std::vector<int64_t> at_all(n), at_pass(n);
        int64_t b_all = 0, b_pass = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (size_t i = 0; i < n; ++i) {
                const Measured& o = m[i];
                if (o.fate != lsg3::KEPT || (o.is_m != 0) != (pass == 1)) continue;
                at_all[i] = b_all; b_all += o.len; ++info->rows_all;
                at_pass[i] = b_pass; if (!o.tags) { b_pass += o.len; ++info->rows_pass; }
            }
        info->bytes_all = b_all; info->bytes_pass = b_pass;
        *out_all = (char*)malloc((size_t)b_all + 1); *out_pass = (char*)malloc((size_t)b_pass + 1);
        if (!*out_all || !*out_pass) { free(*out_all); free(*out_pass); *out_all = *out_pass = nullptr; snprintf(g_s3c_err, sizeof g_s3c_err, "lsio_step3_core_rows: out of memory"); return -3; }
        over_rows(n, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                const Measured& o = m[i];
                if (o.fate != lsg3::KEPT) continue;
                const char* r = t + start[i]; const int len = (int)(start[i + 1] - start[i] - 1);
                lsg3::Row st;
                lsg3::decide(r, len, *p, st);
                { lsg3::PutSink s{*out_all + at_all[i]}; lsg3::print_row(s, r, len, *p, st, o.tags); }
                if (!o.tags) { lsg3::PutSink s{*out_pass + at_pass[i]}; lsg3::print_row(s, r, len, *p, st, o.tags); }
            }
        });
        return 0;
    } catch (...) { snprintf(g_s3c_err, sizeof g_s3c_err, "lsio_step3_core_rows: failed"); return -2; }
}

} // extern "C"
