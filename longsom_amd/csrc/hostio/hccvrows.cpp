// The host twin of lsg_hccv_filter_text (csrc/hccv.hip; the semantics are in include/longsom_hip.h): the same row code (hccv_core.h) over
// a step-2 table in host memory, the same three row sets and the same undecided report.  What runs where there is no GPU, and what the
// device's tables are compared with.  Two passes like the device's: every row decided and measured, the places from the lengths, every
// kept row printed at its place; rows are shared out over threads in contiguous pieces.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../hccv_core.h"

extern "C" int lsio_step3_column_kinds(const char* text, int64_t n_bytes, int32_t n_cols, uint8_t* kinds);

namespace {
thread_local char g_hccv_err[256];

struct Measured { uint32_t len2, len3; uint8_t stage, verdict, is_m, reason; };

template <class F> void over_rows(size_t n, F fn) {
    const unsigned T = n < 4096 ? 1u : std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (T == 1) { fn(0, n); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back([=] { fn(n * t / T, n * (t + 1) / T); });
    for (auto& x : th) x.join();
}
} // namespace

extern "C" {

const char* lsio_hccv_last_error(void) { return g_hccv_err; }

// text: the step-2 table (leading lines that start with '#' are skipped).  *out2, *out3, *out_pass: the rows of .HCCV.tsv2, .HCCV.tsv3 and
// the PASS rows of .HCCV.tsv3, malloc'd (lsio_free_text), their sizes in info; none is made when info->n_undecided > 0.  0, or < 0.
int lsio_hccv_rows(const char* text, int64_t n_bytes, const lsg_hccv_params* p, lsg_hccv_info* info, char** out2, char** out3, char** out_pass) {
    if (!text || n_bytes < 0 || !p || !info || !out2 || !out3 || !out_pass || p->n_cols < 1 || p->n_cols > 64) {
        snprintf(g_hccv_err, sizeof g_hccv_err, "lsio_hccv_rows: bad arguments"); return -1;
    }
    *out2 = *out3 = *out_pass = nullptr;
    memset(info, 0, sizeof *info);
    info->first_undecided = -1;
    try {
        int64_t at = 0;
        while (at < n_bytes && text[at] == '#') { const void* e = memchr(text + at, '\n', (size_t)(n_bytes - at)); at = e ? (const char*)e - text + 1 : n_bytes; }
        const char* t = text + at; const int64_t nb = n_bytes - at;
        if (lsio_step3_column_kinds(t, nb, p->n_cols, info->kinds) != 0) { snprintf(g_hccv_err, sizeof g_hccv_err, "lsio_hccv_rows: column kinds failed"); return -2; }
        std::vector<int64_t> start;
        for (int64_t a = 0; a < nb;) { start.push_back(a); const void* e = memchr(t + a, '\n', (size_t)(nb - a)); a = e ? (const char*)e - t + 1 : nb; }
        const size_t n = start.size();
        start.push_back(nb + ((nb > 0 && t[nb - 1] != '\n') ? 1 : 0));           // (every row then ends one byte before the next one's start)
        for (size_t i = 0; i < n; ++i) if (start[i + 1] - start[i] - 1 > (int64_t)1 << 30) { snprintf(g_hccv_err, sizeof g_hccv_err, "lsio_hccv_rows: a row of more than 2^30 bytes"); return -1; }
        info->rows_in = (int64_t)n;
        std::vector<Measured> m(n);
        over_rows(n, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                const char* r = t + start[i]; const int len = (int)(start[i + 1] - start[i] - 1);
                lsgh::Row st;
                const int stage = lsgh::decide(r, len, *p, st);
                Measured& o = m[i];
                o = Measured{0, 0, st.stage, st.verdict, st.is_m, st.reason};
                if (stage == lsgh::IN_TSV2 || stage == lsgh::IN_TSV3) { lsgh::LenSink s; lsgh::print_row(s, r, len, *p, st, false); o.len2 = s.n; }
                if (stage == lsgh::IN_TSV3) { lsgh::LenSink s; lsgh::print_row(s, r, len, *p, st, true); o.len3 = s.n; }
            }
        });
        // places: .tsv3 holds the chrM rows last
        std::vector<int64_t> at2(n), at3(n), atp(n);
        int64_t b2 = 0, b3 = 0, bp = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (size_t i = 0; i < n; ++i) {
                const Measured& o = m[i];
                if (pass == 0) {
                    if (o.stage == lsgh::UNDECIDED) { if (!info->n_undecided++) { info->first_undecided = (int64_t)i; info->reason = o.reason; } }
                    at2[i] = b2; b2 += o.len2; info->rows_tsv2 += o.len2 > 0;
                }
                if ((o.is_m != 0) != (pass == 1)) continue;
                at3[i] = b3; b3 += o.len3; info->rows_tsv3 += o.len3 > 0;
                const bool ok = o.len3 > 0 && o.verdict == lsgh::V_PASS;
                atp[i] = bp; if (ok) { bp += o.len3; ++info->rows_pass; }
            }
        if (info->n_undecided) { info->rows_tsv2 = info->rows_tsv3 = info->rows_pass = 0; return 0; }
        info->bytes_tsv2 = b2; info->bytes_tsv3 = b3; info->bytes_pass = bp;
        *out2 = (char*)malloc((size_t)b2 + 1); *out3 = (char*)malloc((size_t)b3 + 1); *out_pass = (char*)malloc((size_t)bp + 1);
        if (!*out2 || !*out3 || !*out_pass) { free(*out2); free(*out3); free(*out_pass); *out2 = *out3 = *out_pass = nullptr; snprintf(g_hccv_err, sizeof g_hccv_err, "lsio_hccv_rows: out of memory"); return -3; }
        over_rows(n, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                const Measured& o = m[i];
                if (!o.len2) continue;
                const char* r = t + start[i]; const int len = (int)(start[i + 1] - start[i] - 1);
                lsgh::Row st;
                lsgh::decide(r, len, *p, st);
                { lsgh::PutSink s{*out2 + at2[i]}; lsgh::print_row(s, r, len, *p, st, false); }
                if (!o.len3) continue;
                { lsgh::PutSink s{*out3 + at3[i]}; lsgh::print_row(s, r, len, *p, st, true); }
                if (o.verdict == lsgh::V_PASS) { lsgh::PutSink s{*out_pass + atp[i]}; lsgh::print_row(s, r, len, *p, st, true); }
            }
        });
        return 0;
    } catch (...) { snprintf(g_hccv_err, sizeof g_hccv_err, "lsio_hccv_rows: failed"); return -2; }
}

} // extern "C"
