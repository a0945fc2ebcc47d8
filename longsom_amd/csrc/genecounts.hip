// Cell-by-gene read counts over the resident load: the expression matrix inferCNV reads, as table LSG_TABLE_GENE_COUNTS
// (include/longsom_hip.h lsg_gene_counts has the semantics; longsom_amd/genecounts.py states the contract in numpy).
//
// Replaces, of workflow/rules/CNACalling.smk,
//   rule split_per_bc         :11-27   one BAM per barcode - a read's barcode is resident (read_cb), nothing is split
//   rule featureCount         :29-44   featureCounts -L -a <gtf> over those BAMs                 (k_gc_segments, k_gc_reads)
//   rule format_featureCount  :46-75   names for ids, unnamed ids dropped, groupby().sum()       (row_of_gene: several genes add to one row)
//                                      DataFrame.to_csv                                          (k_gc_print)
//   k_gc_segments  a lane per segment, whatever the order of the segment arrays: a binary search over the 64-bit keys of the elementary
//                  intervals for the first that ends after the segment's start, a walk while one starts before its end, the labels
//                  folded (genecounts_core.h) and then into the owning read's two state words with atomicMin / atomicMax
//   k_gc_reads     a lane per read: its outcome from the two words; atomicAdd into matrix[row_of_gene][cb] and the barcode's tallies;
//                  the call's totals one atomic per wave and outcome
//   k_gc_print     a wave per line (the header is line 0): lanes stride the columns, a wave prefix sum of the fields' lengths places
//                  them; run twice as in tables.hip - lengths, a hipcub scan to 64-bit offsets, then the bytes
// The interval table is 16 bytes an interval, tens of MB for GENCODE: it is read through L2 / Infinity Cache, the segments stream.
#include "lsg_ctx.h"
#include "genecounts_core.h"
#include "text_sink.h"
#include "text_table.h"
#include <chrono>
#include <cstring>
#include <vector>

namespace lsg {
namespace {

struct GcArgs {
    const lsgc::Interval* iv; int64_t n_iv;
    const int32_t* read_tid; const uint16_t* read_flag; const uint8_t* read_mapq; const int32_t* read_cb;
    const uint32_t* seg_read; const int32_t* seg_start; const int32_t* seg_len;
    int64_t n_reads, n_segs;
    int32_t n_cb, min_mapq; uint32_t flag_exclude;
    uint32_t* lo; uint32_t* hi;                       // per read (genecounts_core.h)
    const int32_t* row_of_gene; int32_t n_genes, n_rows;
    uint32_t* matrix; unsigned long long* tallies;    // [n_rows][n_cb], [n_cb][4]
    unsigned long long* small;                        // [0..4]: this call's reads per outcome + unlisted, [5]: a cell passed 2^32 - 1
};

__device__ __forceinline__ bool gc_considered(const GcArgs& a, int64_t r) {
    return lsgc::considered(a.read_flag[r], a.read_mapq[r], a.flag_exclude, a.min_mapq);
}

__global__ __launch_bounds__(256) void k_gc_segments(GcArgs a) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_segs) return;
    const int64_t r = a.seg_read[s];
    if (r >= a.n_reads) return;
    const int32_t cb = a.read_cb[r];
    if (cb < 0 || cb >= a.n_cb || !gc_considered(a, r)) return;
    const int32_t tid = a.read_tid[r], start = a.seg_start[s], len = a.seg_len[s];
    if (tid < 0 || start < 0 || len <= 0) return;
    const uint64_t ks = ((uint64_t)(uint32_t)tid << 32) | (uint32_t)start;
    uint32_t lo = lsgc::LO_NONE, hi = lsgc::HI_NONE;
    if (lsgc::fold_block(a.iv, a.n_iv, ks, ks + (uint32_t)len, lo, hi)) { atomicMin(a.lo + r, lo); atomicMax(a.hi + r, hi); }
}

__global__ __launch_bounds__(256) void k_gc_reads(GcArgs a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int cls = -1;                                     // 0..3 the outcomes, 4 no listed barcode
    if (r < a.n_reads) {
        const int32_t cb = a.read_cb[r];
        if (cb < 0 || cb >= a.n_cb) cls = 4;
        else {
            cls = lsgc::FILTERED;
            if (gc_considered(a, r)) {
                const uint32_t lo = a.lo[r];
                cls = lsgc::outcome(lo, a.hi[r]);
                if (cls == lsgc::ASSIGNED && lo < (uint32_t)a.n_genes) {
                    const int32_t row = a.row_of_gene[lo];
                    if (row >= 0 && row < a.n_rows && atomicAdd(a.matrix + (size_t)row * (size_t)a.n_cb + (size_t)cb, 1u) == 0xFFFFFFFFu) atomicOr(a.small + 5, 1ull);
                }
            }
            atomicAdd(a.tallies + (size_t)cb * 4 + (size_t)cls, 1ull);
        }
    }
    for (int k = 0; k < 5; ++k) {
        const unsigned long long m = __ballot(cls == k);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(a.small + k, (unsigned long long)__popcll(m));
    }
}

struct GcPrint {
    const uint32_t* matrix; int32_t n_rows, n_cb, n_cols; char sep;
    const uint32_t* row_off; const char* row_txt; const int32_t* col_src; const uint32_t* col_off; const char* col_txt;
    uint32_t* len; const uint64_t* off; char* text;
};
// line 0 is "Geneid<sep><barcode>...", line 1 + r is "<name r><sep><count>..."; PUT = false: the line's length only (line n_rows + 1: the scan's end marker)
template <bool PUT> __global__ __launch_bounds__(256) void k_gc_print(GcPrint a) {
    const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (line > (int64_t)a.n_rows) { if (!PUT && line == (int64_t)a.n_rows + 1 && lane == 0) a.len[line] = 0; return; }
    const bool head = line == 0;
    const char* name = head ? "Geneid" : a.row_txt + a.row_off[line - 1];
    const uint32_t n_name = head ? 6u : a.row_off[line] - a.row_off[line - 1];
    char* out = PUT ? a.text + a.off[line] : nullptr;
    if (PUT) for (uint32_t q = lane; q < n_name; q += 64u) out[q] = name[q];
    const uint32_t* row = head ? nullptr : a.matrix + (size_t)(line - 1) * (size_t)a.n_cb;
    uint32_t base = n_name;
    for (int32_t c0 = 0; c0 < a.n_cols; c0 += 64) {           // (uniform over the wave: every lane takes part in the shuffles)
        const int32_t col = c0 + (int32_t)lane;
        const bool in = col < a.n_cols;
        uint32_t v = 0, n = 0;
        if (in) {
            if (head) n = 1u + (a.col_off[col + 1] - a.col_off[col]);
            else { v = row[a.col_src[col]]; n = 1u + (uint32_t)n_digits(v); }
        }
        uint32_t x = n;                                       // inclusive prefix sum over the wave
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if ((int)lane >= o) x += y; }
        const uint32_t total = __shfl(x, 63, 64);
        if (PUT && in) {
            PutSink s{out + base + (x - n)};
            s.ch(a.sep);
            if (head) s.str(a.col_txt + a.col_off[col], (int)(n - 1u)); else s.u64(v);
        }
        base += total;
    }
    if (lane == 0) { if (PUT) out[base] = '\n'; else a.len[line] = base + 1u; }
}

void drop_matrix(lsg_ctx* c) {
    GeneCounts& g = c->gc;
    g.matrix.release(); g.tallies.release(); g.state.release(); g.text.release(); g.scratch.release();
    g.mat_valid = g.text_valid = false; g.n_cb = 0; g.n_cols = 0;
    c->tab_text[LSG_TABLE_GENE_COUNTS].release(); c->tab_bytes[LSG_TABLE_GENE_COUNTS] = -1;
}

} // namespace

int run_format_gene_table(lsg_ctx* c, int64_t* n_bytes) {
    const char* who = "lsg_format_table";
    if (n_bytes) *n_bytes = 0;
    GeneCounts& g = c->gc;
    c->tab_bytes[LSG_TABLE_GENE_COUNTS] = -1;
    if (!g.mat_valid || !g.text_valid) { set_error("%s: table %d needs lsg_gene_counts and lsg_gene_counts_set_text first", who, (int)LSG_TABLE_GENE_COUNTS); return -2; }
    hipStream_t st = c->stream;
    const char* tx = g.text.as<char>();
    GcPrint a{};
    a.matrix = g.matrix.as<uint32_t>(); a.n_rows = g.n_rows; a.n_cb = g.n_cb; a.n_cols = g.n_cols; a.sep = g.sep;
    a.row_off = reinterpret_cast<const uint32_t*>(tx + g.row_off_at); a.row_txt = tx + g.row_txt_at;
    a.col_src = reinterpret_cast<const int32_t*>(tx + g.col_src_at); a.col_off = reinterpret_cast<const uint32_t*>(tx + g.col_off_at); a.col_txt = tx + g.col_txt_at;
    const int64_t lines = (int64_t)g.n_rows + 1;
    RowPlaces r;
    if (row_places(g.scratch, lines, -1, r)) return -1;
    a.len = r.len; a.off = r.off;
    hipLaunchKernelGGL(k_gc_print<false>, dim3((unsigned)((lines + 1 + 3) / 4)), dim3(256), 0, st, a);
    int64_t bytes = 0;
    if (finish_places(c, r, &bytes)) return -1;
    if (print_table(c, LSG_TABLE_GENE_COUNTS, bytes, [&](char* text) { a.text = text; hipLaunchKernelGGL(k_gc_print<true>, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, st, a); })) return -1;
    if (n_bytes) *n_bytes = bytes;
    return 0;
}

} // namespace lsg

using namespace lsg;

extern "C" int lsg_load_annotation(lsg_ctx* c, int64_t n_iv, const uint64_t* keys, const uint32_t* lens, const uint32_t* labels, int32_t n_genes,
                                   const int32_t* row_of_gene, int32_t n_rows) {
    const char* who = "lsg_load_annotation";
    if (!c || n_iv < 0 || n_genes < 0 || n_rows < 0 || (n_iv > 0 && (!keys || !lens || !labels)) || (n_genes > 0 && !row_of_gene)) { set_error("%s: bad arguments", who); return -2; }
    if ((uint32_t)n_genes > lsgc::MAX_GENES || n_iv >= ((int64_t)1 << 40)) { set_error("%s: %d genes, %lld intervals", who, n_genes, (long long)n_iv); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    LSG_HIP(hipStreamSynchronize(c->stream));
    GeneCounts& g = c->gc;
    drop_matrix(c);                                   // a matrix belongs to the annotation it was counted under
    g.ann_valid = false;
    // every index a kernel follows is checked here
    std::vector<lsgc::Interval> iv((size_t)n_iv);
    for (int64_t i = 0; i < n_iv; ++i) {
        if (lens[i] == 0 || (keys[i] & 0xFFFFFFFFull) + lens[i] > 0x100000000ull) { set_error("%s: interval %lld is empty or ends past position 2^32", who, (long long)i); return -2; }
        if (i > 0 && keys[i - 1] + lens[i - 1] > keys[i]) { set_error("%s: intervals %lld and %lld are not sorted and disjoint", who, (long long)i - 1, (long long)i); return -2; }
        if (labels[i] != lsgc::AMBIG && labels[i] >= (uint32_t)n_genes) { set_error("%s: interval %lld is labelled gene %u of %d", who, (long long)i, labels[i], n_genes); return -2; }
        iv[(size_t)i] = lsgc::Interval{keys[i], lens[i], labels[i]};
    }
    for (int32_t q = 0; q < n_genes; ++q)
        if (row_of_gene[q] < -1 || row_of_gene[q] >= n_rows) { set_error("%s: gene %d adds to row %d of %d", who, q, row_of_gene[q], n_rows); return -2; }
    if (g.iv.reserve(((size_t)n_iv + 1) * sizeof(lsgc::Interval)) || g.row_of_gene.reserve(((size_t)n_genes + 1) * 4)) return -1;
    if (n_iv) LSG_HIP(hipMemcpyAsync(g.iv.p, iv.data(), (size_t)n_iv * sizeof(lsgc::Interval), hipMemcpyHostToDevice, c->stream));
    if (n_genes) LSG_HIP(hipMemcpyAsync(g.row_of_gene.p, row_of_gene, (size_t)n_genes * 4, hipMemcpyHostToDevice, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    g.n_iv = n_iv; g.n_genes = n_genes; g.n_rows = n_rows; g.ann_valid = true;
    return 0;
}

extern "C" int lsg_gene_counts(lsg_ctx* c, const lsg_gene_count_params* p, lsg_gene_count_info* info) {
    const char* who = "lsg_gene_counts";
    if (!c || !p || !info) { set_error("%s: bad arguments", who); return -2; }
    *info = lsg_gene_count_info{};
    GeneCounts& g = c->gc;
    if (!g.ann_valid) { set_error("%s: no annotation loaded (lsg_load_annotation)", who); return -2; }
    if (!c->rd.on_device) { set_error("%s: no reads resident (lsg_load_reads or lsg_load_bam)", who); return -2; }
    if (c->n_cb <= 0) { set_error("%s: no barcodes set", who); return -2; }
    if (g.mat_valid && g.n_cb != c->n_cb) { set_error("%s: the matrix was started with %d barcodes, the handle has %d now: lsg_gene_counts_reset first", who, g.n_cb, c->n_cb); return -2; }
    const int64_t R = c->rd.n_reads, S = c->rd.n_segs;
    if ((R > 0 && (!c->rd.read_tid || !c->rd.read_flag || !c->rd.read_mapq || !c->rd.read_cb)) || (S > 0 && (!c->rd.seg_read || !c->rd.seg_start || !c->rd.seg_len))) {
        set_error("%s: the resident load has no per-read arrays", who); return -2;
    }
    LSG_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const auto t_all = std::chrono::steady_clock::now();
    const size_t cells = (size_t)g.n_rows * (size_t)c->n_cb;
    if (!g.mat_valid) {
        if (g.matrix.reserve((cells + 1) * 4) || g.tallies.reserve((size_t)c->n_cb * 32)) return -1;
        LSG_HIP(hipMemsetAsync(g.matrix.p, 0, (cells + 1) * 4, st));
        LSG_HIP(hipMemsetAsync(g.tallies.p, 0, (size_t)c->n_cb * 32, st));
        g.n_cb = c->n_cb; g.mat_valid = true;
    }
    c->tab_bytes[LSG_TABLE_GENE_COUNTS] = -1;          // the text is a snapshot of a matrix that changes now
    if (g.state.reserve(((size_t)R + 1) * 8) || g.small.reserve(64)) return -1;
    GcArgs a{};
    a.iv = g.iv.as<lsgc::Interval>(); a.n_iv = g.n_iv;
    a.read_tid = c->rd.read_tid; a.read_flag = c->rd.read_flag; a.read_mapq = c->rd.read_mapq; a.read_cb = c->rd.read_cb;
    a.seg_read = c->rd.seg_read; a.seg_start = c->rd.seg_start; a.seg_len = c->rd.seg_len;
    a.n_reads = R; a.n_segs = S; a.n_cb = g.n_cb; a.min_mapq = p->min_mapq; a.flag_exclude = p->flag_exclude;
    a.lo = g.state.as<uint32_t>(); a.hi = a.lo + R;
    a.row_of_gene = g.row_of_gene.as<int32_t>(); a.n_genes = g.n_genes; a.n_rows = g.n_rows;
    a.matrix = g.matrix.as<uint32_t>(); a.tallies = g.tallies.as<unsigned long long>(); a.small = g.small.as<unsigned long long>();
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto done = [&](int rc) { for (auto& e : ev) if (e) (void)hipEventDestroy(e); return rc; };
    for (auto& e : ev) LSG_HIP_OR(hipEventCreate(&e), done(-1));
    if (R) { LSG_HIP_OR(hipMemsetAsync(a.lo, 0xff, (size_t)R * 4, st), done(-1)); LSG_HIP_OR(hipMemsetAsync(a.hi, 0, (size_t)R * 4, st), done(-1)); }
    LSG_HIP_OR(hipMemsetAsync(a.small, 0, 64, st), done(-1));
    LSG_HIP_OR(hipEventRecord(ev[0], st), done(-1));
    if (S && R && g.n_iv) hipLaunchKernelGGL(k_gc_segments, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, a);
    LSG_HIP_OR(hipEventRecord(ev[1], st), done(-1));
    if (R) hipLaunchKernelGGL(k_gc_reads, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, a);
    LSG_HIP_OR(hipEventRecord(ev[2], st), done(-1));
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipMemcpyAsync(c->h_pin, a.small, 48, hipMemcpyDeviceToHost, st), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    unsigned long long h[6];
    memcpy(h, c->h_pin, sizeof(h));
    info->n_reads = R; info->n_segs = S;
    info->n_assigned = (int64_t)h[0]; info->n_no_features = (int64_t)h[1]; info->n_ambiguity = (int64_t)h[2]; info->n_filtered = (int64_t)h[3]; info->n_unlisted = (int64_t)h[4];
    (void)hipEventElapsedTime(&info->ms_segments, ev[0], ev[1]); (void)hipEventElapsedTime(&info->ms_reads, ev[1], ev[2]);
    info->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    if (h[5]) { set_error("%s: a cell of the matrix passed 2^32 - 1 reads", who); return done(-1); }
    return done(0);
}

extern "C" int lsg_gene_counts_fetch(lsg_ctx* c, uint32_t* matrix, uint64_t* tallies) {
    if (!c) { set_error("lsg_gene_counts_fetch: NULL handle"); return -2; }
    GeneCounts& g = c->gc;
    if (!g.mat_valid) { set_error("lsg_gene_counts_fetch: nothing counted (lsg_gene_counts first)"); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    const size_t cells = (size_t)g.n_rows * (size_t)g.n_cb;
    if (matrix && cells) LSG_HIP(hipMemcpyAsync(matrix, g.matrix.p, cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (tallies) LSG_HIP(hipMemcpyAsync(tallies, g.tallies.p, (size_t)g.n_cb * 32, hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int lsg_gene_counts_set_text(lsg_ctx* c, const char* row_names, const uint32_t* row_off, int32_t n_cols, const int32_t* col_src,
                                        const char* col_names, const uint32_t* col_off, int32_t separator) {
    const char* who = "lsg_gene_counts_set_text";
    if (!c || !row_off || !col_off || n_cols < 0 || (n_cols > 0 && !col_src) || separator <= 0 || separator > 127) { set_error("%s: bad arguments", who); return -2; }
    GeneCounts& g = c->gc;
    g.text_valid = false;
    c->tab_bytes[LSG_TABLE_GENE_COUNTS] = -1;
    if (!g.mat_valid) { set_error("%s: nothing counted (lsg_gene_counts first)", who); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    const int32_t N = g.n_rows;
    auto offsets_ok = [](const uint32_t* off, int64_t n) { if (off[0] != 0) return false; for (int64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return false; return true; };
    if (!offsets_ok(row_off, N) || !offsets_ok(col_off, n_cols)) { set_error("%s: string offsets must start at 0 and ascend", who); return -2; }
    for (int32_t i = 0; i < n_cols; ++i) if (col_src[i] < 0 || col_src[i] >= g.n_cb) { set_error("%s: col_src[%d] is not a barcode", who, i); return -2; }
    const size_t n_row_txt = row_off[N], n_col_txt = col_off[n_cols];
    if ((n_row_txt && !row_names) || (n_col_txt && !col_names)) { set_error("%s: bad arguments", who); return -2; }
    HostBlob b;
    g.row_off_at = b.add(row_off, (size_t)(N + 1) * 4); g.col_src_at = b.add(col_src, (size_t)n_cols * 4); g.col_off_at = b.add(col_off, (size_t)(n_cols + 1) * 4);
    g.row_txt_at = b.add(row_names, n_row_txt); g.col_txt_at = b.add(col_names, n_col_txt);
    if (b.upload(g.text, c->stream)) return -1;
    g.n_cols = n_cols; g.sep = (char)separator; g.text_valid = true;
    return 0;
}

extern "C" int lsg_gene_counts_reset(lsg_ctx* c) {
    if (!c) { set_error("lsg_gene_counts_reset: NULL handle"); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    LSG_HIP(hipStreamSynchronize(c->stream));
    c->gc.release();
    c->tab_text[LSG_TABLE_GENE_COUNTS].release(); c->tab_bytes[LSG_TABLE_GENE_COUNTS] = -1;
    return 0;
}
