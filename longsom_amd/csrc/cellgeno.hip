// Per-cell verdicts at the final SNVs and the cell-by-variant matrices, everything after the counts.
//
// Replaces, of workflow/scripts/CellClustering/SingleCellGenotype.py (rule SingleCellGenotype, rules/CellClustering.smk:4-103),
//   the per-cell loop of run_interval        :181-224   VAF, BetaBin, MutationStatus, BinMutationStatus (k_cell_classify; the tallies per
//                                                       barcode are what CellTypeReannotation.py:9-18 counts off such a table)
//   the rows of <id>.SingleCellGenotype.tsv  :222-224,305-317   16 columns, one row per (site, barcode)              (k_cell_row_len / _put)
//   pivot_long_dataframe + sort_chr_index    :342-379   the rows of DpMatrix / AltMatrix / VAFMatrix / BinaryMatrix    (k_cell_matrix)
// The counts themselves (:84-178) are genotype.hip's k_geno_sites with the depth cap of lsg_genotype_cells_grouped; they are classified
// where they lie.  The orders (long table: windows by chromosome text; matrices: natsorted INDEX; columns: sorted CB) and every string a
// row prints are the host's (longsom_amd/cellclust.py), uploaded once: the device prints n_sites x n_cb rows and four matrices from them.
// The text is printed twice, as in tables.hip: lengths, a scan, then the bytes.
//
// Replaces, of workflow/scripts/CellClustering/FormatInputBnpC.py (rule FormatInputBnpC, rules/CellClustering.smk:105-133),
//   the read with 3 and "." as NA             :7-8     the resident bin (3) and vaf4 (-1) already say it
//   the row filter, the column filter         :16,19   k_bnpc_row_count, k_bnpc_col_count, k_bnpc_col_flags, two hipcub selects
//   loc / concat / to_csv of both matrices    :21-34   k_cell_matrix over the kept rows and columns (kinds M_BNPC_BIN, M_BNPC_VAF)
// The fusion rows (:11-13,27) and Barcodes.tsv (:9,26,30,35) are the host's (longsom_amd/cellclust.py).
#include "lsg_ctx.h"
#include "bb_tail.h"
#include "text_sink.h"
#include "text_table.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace lsg {
int run_genotype(lsg_ctx* c, const lsg_genotype_params* p, int64_t n_sites, const int64_t* site_keys, const uint8_t* alt_sym,
                 uint32_t* dp, uint32_t* alt, int on_device, int32_t max_depth, int64_t n_groups, const int64_t* group_off);

namespace {

// round(a / b, 4) * 1e4 as Python rounds the double quotient (text_sink.h put_ratio states the rule); b > 0
__device__ __forceinline__ int32_t ratio4(uint32_t a, uint32_t b) {
    const double x = (double)a / (double)b;
    const double hi = x * 10000.0, lo = fma(x, 10000.0, -hi);
    const double fl = floor(hi);
    int64_t k = (int64_t)fl;
    const double t = ((hi - fl) - 0.5) + lo;
    if (t > 0.0 || (t == 0.0 && (k & 1))) ++k;
    return (int32_t)k;
}

// SingleCellGenotype.py:188-218 for every cell; the tail is evaluated for cells with ALT > 0 outside the flagged sites only
__global__ __launch_bounds__(256) void k_cell_classify(const uint32_t* dp, const uint32_t* alt, const uint8_t* is_chrm, int64_t n_cells, int32_t n_cb,
                                                       double al, double be, double lgc0, double lgcn, double pvalue,
                                                       int32_t* vaf4, int32_t* p4, uint8_t* status, uint8_t* bin) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t DP = dp[i], ALT = alt[i];
        int32_t v = -1, p = -1;
        int st = LSG_CELL_NOCOVERAGE;
        if (DP > 0) {
            v = ratio4(ALT, DP);                                                           // :194
            if (ALT == 0) st = LSG_CELL_NOALT;                                             // :211
            else if (is_chrm[i / n_cb]) st = v < 3000 ? LSG_CELL_LOWVAF_CHRM : LSG_CELL_PASS;      // :197-201
            else {
                p = round4(bb_upper_tail(ALT, DP, al, be, bb_pm0(DP, al, be, lgc0), lgcn));        // :204
                st = (double)p / 10000.0 < pvalue ? LSG_CELL_PASS : LSG_CELL_BETABIN_PROBLEM;       // :206-209
            }
        }
        vaf4[i] = v; p4[i] = p; status[i] = (uint8_t)st;
        bin[i] = (uint8_t)(st == LSG_CELL_PASS ? 1 : st == LSG_CELL_NOCOVERAGE ? 3 : 0);   // :213-218
    }
}

// per barcode: sites with coverage, sites with PASS (a thread per barcode walks the sites: neighbours read neighbouring bytes)
__global__ __launch_bounds__(256) void k_cell_tally(const uint8_t* status, int64_t n_sites, int32_t n_cb, int64_t* n_cov, int64_t* n_pass) {
    const int cb = blockIdx.x * blockDim.x + threadIdx.x;
    if (cb >= n_cb) return;
    int64_t cov = 0, pass = 0;
    for (int64_t s = 0; s < n_sites; ++s) {
        const int st = status[s * n_cb + cb];
        cov += st != LSG_CELL_NOCOVERAGE; pass += st == LSG_CELL_PASS;
    }
    n_cov[cb] = cov; n_pass[cb] = pass;
}

// FormatInputBnpC.py:16 - bin.replace(0, nan).count(axis = 1) > min_cells_per_mut: per row of mat_order the cells equal to 1 (3 is NA,
// a column no barcode stands behind is NA).  A wave per row, its lanes along the columns: with col_src ascending, as the sorted columns
// of a sample's sorted barcodes are, a wave reads 64 neighbouring bytes of the row at a time.
__global__ __launch_bounds__(256) void k_bnpc_row_count(const uint8_t* bin, const int32_t* mat_order, const int32_t* col_src, int64_t n_mat, int32_t n_cols,
                                                        int32_t n_cb, int32_t min_mut, int32_t* row_mut, uint8_t* row_keep) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_mat) return;
    const uint8_t* row = bin + (int64_t)mat_order[r] * n_cb;
    int cnt = 0;
    for (int col = lane; col < n_cols; col += 64) {
        const int src = col_src[col];
        if (src >= 0) cnt += row[src] == 1;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if (lane == 0) { row_mut[r] = cnt; row_keep[r] = (uint8_t)(cnt > min_mut); }
}
// :19 - bin.count() > min_pos_cov over the rows :16 kept, and the same count over all rows (a column with an NA anywhere was read as
// float64, :7).  A lane per column, so that neighbours read neighbouring bytes of a row; the rows are split over the workgroups of
// blockIdx.y, `share` rows each, and a workgroup adds its two sums with ONE atomic per column: integer sums do not depend on the order
// they arrive in, a wave's 64 adds go to 256 contiguous bytes, and a second pass would need a slab of workgroups x columns partial
// sums for what is two words per column.  cov_kept / cov_all are zeroed by the caller.
__global__ __launch_bounds__(256) void k_bnpc_col_count(const uint8_t* bin, const int32_t* mat_order, const int32_t* col_src, const uint8_t* row_keep, int64_t n_mat,
                                                        int32_t n_cols, int32_t n_cb, int64_t share, int32_t* cov_kept, int32_t* cov_all) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= n_cols) return;
    const int src = col_src[col];
    if (src < 0) return;                                             // nobody behind the column: it counts 0
    const int64_t r0 = (int64_t)blockIdx.y * share, r1 = r0 + share < n_mat ? r0 + share : n_mat;
    int kept = 0, all = 0;
    for (int64_t r = r0; r < r1; ++r) {
        const int covered = bin[(int64_t)mat_order[r] * n_cb + src] != 3;
        all += covered; kept += covered & row_keep[r];
    }
    if (all) atomicAdd(cov_all + col, all);
    if (kept) atomicAdd(cov_kept + col, kept);
}
__global__ __launch_bounds__(256) void k_bnpc_col_flags(const int32_t* cov_kept, const int32_t* cov_all, const uint8_t* col_ok, int32_t n_cols, int32_t n_mat,
                                                        int32_t min_cov, uint8_t* col_keep, uint8_t* col_int) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= n_cols) return;
    col_keep[col] = (uint8_t)(cov_kept[col] > min_cov);
    col_int[col] = (uint8_t)(col_ok[col] != 0 && cov_all[col] == n_mat);
}
// lsg_cellgeno_load_cells: the verdict a parsed Binary cell stands for
__global__ __launch_bounds__(256) void k_cells_status(const uint8_t* bin, int64_t n_cells, uint8_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * blockDim.x)
        status[i] = (uint8_t)(bin[i] == 3 ? LSG_CELL_NOCOVERAGE : bin[i] == 1 ? LSG_CELL_PASS : LSG_CELL_NOALT);
}

struct CellArgs {
    const uint32_t* dp; const uint32_t* alt; const int32_t* vaf4; const int32_t* p4; const uint8_t* status; const uint8_t* bin;
    int32_t n_cb, n_cols, float_cells, kind;
    const char* head; const char* index; const char* label; const char* cb; const char* ct;
    const uint32_t* head_off; const uint32_t* index_off; const uint32_t* label_off; const uint32_t* cb_off; const uint32_t* ct_off;
    const int32_t* order; int64_t n;                  // the sites in the table's order; n = rows of the table (long: sites x n_cb)
    const int32_t* col_src;
    const int32_t* col_sel; const uint8_t* col_int;   // the BnpC tables: the kept columns (n_cols of them) and which print as integers; else null
    uint32_t* len; const uint64_t* off; char* text;
};

template <class S> __device__ __forceinline__ void put_str(S& s, const char* txt, const uint32_t* off, int64_t i) {
    s.str(txt + off[i], (int)(off[i + 1] - off[i]));
}
__device__ __forceinline__ const char* status_name(int st, int& n) {
    switch (st) {
        case LSG_CELL_NOCOVERAGE: n = 10; return "NoCoverage";
        case LSG_CELL_NOALT: n = 10; return "NoAltReads";
        case LSG_CELL_LOWVAF_CHRM: n = 10; return "LowVAFChrM";
        case LSG_CELL_BETABIN_PROBLEM: n = 15; return "BetaBin_problem";
        default: n = 4; return "PASS";
    }
}

// one row of <id>.SingleCellGenotype.tsv (:222): row r = (r / n_cb)-th site of the order, barcode r % n_cb
template <class S> __device__ void long_row(S& s, const CellArgs& a, int64_t r) {
    const int64_t j = r / a.n_cb;
    const int cb = (int)(r - j * a.n_cb);
    const int64_t site = a.order[j], cell = site * a.n_cb + cb;
    put_str(s, a.head, a.head_off, site); s.ch('\t');
    put_str(s, a.cb, a.cb_off, cb); s.ch('\t'); put_str(s, a.ct, a.ct_off, cb); s.ch('\t');
    s.u64(a.dp[cell]); s.ch('\t'); s.u64(a.alt[cell]); s.ch('\t');
    const int st = a.status[cell];
    if (st == LSG_CELL_NOCOVERAGE) s.ch('.'); else put_p4(s, a.vaf4[cell]);
    s.ch('\t');
    if (a.p4[cell] < 0) s.ch('.'); else put_p4(s, a.p4[cell]);
    s.ch('\t');
    int n; const char* name = status_name(st, n); s.str(name, n);
    s.ch('\t'); s.ch((char)('0' + a.bin[cell])); s.ch('\t');
    put_str(s, a.index, a.index_off, site); s.ch('\n');
}
__global__ __launch_bounds__(256) void k_cell_row_len(CellArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.n) return;
    LenSink s;
    if (i < a.n) long_row(s, a, i);
    a.len[i] = s.n;
}
__global__ __launch_bounds__(256) void k_cell_row_put(CellArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    PutSink s{a.text + a.off[i]};
    long_row(s, a, i);
}

enum { M_DP = 0, M_ALT, M_VAF, M_BIN, M_BNPC_BIN, M_BNPC_VAF };
// one cell of a matrix, with the tab before it: the value of (site, barcode of the column), nothing for a column no barcode of the
// sample stands behind (a barcode of the fusion file alone); float_cells: pandas prints the integer matrices of a pivot with gaps as floats
template <class S> __device__ __forceinline__ void mat_cell(S& s, const CellArgs& a, int64_t site, int col) {
    s.ch('\t');
    const int src = a.col_src[col];
    if (src < 0) return;
    const int64_t cell = site * a.n_cb + src;
    if (a.kind == M_BNPC_BIN) {                                      // FormatInputBnpC.py:33 - NA empty, the value as its column's dtype prints it
        const int b = a.bin[cell];
        if (b == 3) return;
        s.ch((char)('0' + b));
        if (!a.col_int[col]) LIT(s, ".0");
        return;
    }
    if (a.kind == M_BNPC_VAF) {                                      // :34 - a float column: NA empty
        if (a.vaf4[cell] >= 0) put_p4(s, a.vaf4[cell]);
        return;
    }
    if (a.kind == M_VAF) {                                           // the long table's own string
        if (a.status[cell] == LSG_CELL_NOCOVERAGE) s.ch('.'); else put_p4(s, a.vaf4[cell]);
        return;
    }
    s.u64(a.kind == M_DP ? a.dp[cell] : a.kind == M_ALT ? a.alt[cell] : (uint32_t)a.bin[cell]);
    if (a.float_cells) LIT(s, ".0");
}
// a workgroup per matrix row: label, then the cells 256 at a time, a block scan of their lengths giving each its place.  PUT = false:
// the row's length only (block n: the scan's end marker)
template <bool PUT> __global__ __launch_bounds__(256) void k_cell_matrix(CellArgs a) {
    using Scan = hipcub::BlockScan<uint32_t, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t r = blockIdx.x;
    if (r >= a.n) { if (!PUT && r == a.n && threadIdx.x == 0) a.len[r] = 0; return; }
    const int64_t site = a.order[r];
    const uint32_t l0 = a.label_off[site], lab = a.label_off[site + 1] - l0;
    char* out = PUT ? a.text + a.off[r] : nullptr;
    if (PUT) for (uint32_t q = threadIdx.x; q < lab; q += blockDim.x) out[q] = a.label[l0 + q];
    uint32_t base = lab;
    for (int c0 = 0; c0 < a.n_cols; c0 += 256) {
        const bool in = c0 + (int)threadIdx.x < a.n_cols;
        const int col = !in ? 0 : a.col_sel ? a.col_sel[c0 + (int)threadIdx.x] : c0 + (int)threadIdx.x;
        LenSink ls;
        if (in) mat_cell(ls, a, site, col);
        uint32_t excl, total;
        Scan(tmp).ExclusiveSum(ls.n, excl, total);
        __syncthreads();
        if (PUT && in) { PutSink ps{out + base + excl}; mat_cell(ps, a, site, col); }
        base += total;
    }
    if (threadIdx.x == 0) { if (PUT) out[base] = '\n'; else a.len[r] = base + 1; }
}

int reserve_cells(lsg_ctx* c, int64_t n_sites, int32_t n_cb) {
    CellGeno& g = c->cg;
    const size_t cells = (size_t)(n_sites > 0 ? n_sites : 1) * (size_t)n_cb;
    if (g.dp.reserve(cells * 4) || g.alt.reserve(cells * 4) || g.vaf4.reserve(cells * 4) || g.p4.reserve(cells * 4) || g.status.reserve(cells) ||
        g.bin.reserve(cells) || g.is_chrm.reserve((size_t)(n_sites > 0 ? n_sites : 1)) || g.n_cov.reserve((size_t)n_cb * 8) || g.n_pass.reserve((size_t)n_cb * 8)) return -1;
    return 0;
}

// the verdicts and tallies of the resident dp / alt
int classify(lsg_ctx* c, const char* who, int64_t n_sites, int32_t n_cb, const uint8_t* is_chrm, double al, double be, double pvalue) {
    CellGeno& g = c->cg;
    hipStream_t st = c->stream;
    const int64_t cells = n_sites * (int64_t)n_cb;
    if (n_sites > 0) {
        LSG_HIP(hipMemcpyAsync(g.is_chrm.p, is_chrm, (size_t)n_sites, hipMemcpyHostToDevice, st));
        unsigned blocks = (unsigned)((cells + 255) / 256); if (blocks > (unsigned)(c->n_cus * 32)) blocks = (unsigned)(c->n_cus * 32);
        hipLaunchKernelGGL(k_cell_classify, dim3(blocks), dim3(256), 0, st, g.dp.as<uint32_t>(), g.alt.as<uint32_t>(), g.is_chrm.as<uint8_t>(), cells, n_cb, al, be,
                           lgamma(al + be) - lgamma(be), lgamma(al + be) - lgamma(al), pvalue, g.vaf4.as<int32_t>(), g.p4.as<int32_t>(), g.status.as<uint8_t>(), g.bin.as<uint8_t>());
    }
    hipLaunchKernelGGL(k_cell_tally, dim3((unsigned)((n_cb + 255) / 256)), dim3(256), 0, st, g.status.as<uint8_t>(), n_sites, n_cb, g.n_cov.as<int64_t>(), g.n_pass.as<int64_t>());
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { set_error("%s: kernel failed", who); return -1; }
    g.n_sites = n_sites; g.n_cb = n_cb; g.valid = true; g.cells_only = false;
    return 0;
}

int check_tail_params(const char* who, double al, double be, double pvalue) {
    if (!(al > 0.0) || !(be > 0.0) || !(pvalue == pvalue)) { set_error("%s: alpha2 and beta2 must be positive, pvalue a number", who); return -2; }
    return 0;
}

} // namespace

int run_cellgeno_count(lsg_ctx* c, const lsg_genotype_params* p, int32_t max_depth, int64_t n_sites, const int64_t* site_keys, const uint8_t* alt_sym,
                       const uint8_t* is_chrm, int64_t n_groups, const int64_t* group_off, double alpha2, double beta2, double pvalue) {
    const char* who = "lsg_cellgeno_count";
    CellGeno& g = c->cg;
    g.valid = g.text_valid = g.filt_valid = false;
    for (int t = LSG_TABLE_CELL_LONG; t <= LSG_TABLE_BNPC_VAF; ++t) c->tab_bytes[t] = -1;
    if (int rc = check_tail_params(who, alpha2, beta2, pvalue)) return rc;
    if (c->n_contigs <= 0) { set_error("%s: no contigs set", who); return -2; }
    if (c->n_cb <= 0) { set_error("%s: no barcodes set", who); return -2; }
    if (!keeps_store(c->load_form)) { set_error("%s: the load kept no store (lsg_set_store_policy): load the reads again with LSG_STORE_KEEP", who); return -2; }
    if (!c->tm_valid) { set_error("%s: no reads loaded", who); return -2; }
    for (int64_t i = 1; i < n_sites; ++i)
        if (site_keys[i] <= site_keys[i - 1]) { set_error("%s: site keys must be strictly ascending", who); return -2; }
    if ((double)n_sites * (double)c->n_cb >= 2147483648.0) { set_error("%s: %lld sites x %d barcodes", who, (long long)n_sites, c->n_cb); return -2; }
    if (reserve_cells(c, n_sites, c->n_cb) || g.keys.reserve((size_t)(n_sites > 0 ? n_sites : 1) * 8) || g.alt_sym.reserve((size_t)(n_sites > 0 ? n_sites : 1))) return -1;
    if (n_sites > 0) {
        LSG_HIP(hipMemcpyAsync(g.keys.p, site_keys, (size_t)n_sites * 8, hipMemcpyHostToDevice, c->stream));
        LSG_HIP(hipMemcpyAsync(g.alt_sym.p, alt_sym, (size_t)n_sites, hipMemcpyHostToDevice, c->stream));
        // the counts land in the arrays the verdicts are made from: no host copy in between
        if (int rc = run_genotype(c, p, n_sites, g.keys.as<int64_t>(), g.alt_sym.as<uint8_t>(), g.dp.as<uint32_t>(), g.alt.as<uint32_t>(), 1, max_depth, n_groups, group_off)) return rc;
    }
    return classify(c, who, n_sites, c->n_cb, is_chrm, alpha2, beta2, pvalue);
}

int run_cellgeno_load_counts(lsg_ctx* c, int64_t n_sites, int32_t n_cb, const uint32_t* dp, const uint32_t* alt, const uint8_t* is_chrm, double alpha2, double beta2, double pvalue) {
    const char* who = "lsg_cellgeno_load_counts";
    CellGeno& g = c->cg;
    g.valid = g.text_valid = g.filt_valid = false;
    for (int t = LSG_TABLE_CELL_LONG; t <= LSG_TABLE_BNPC_VAF; ++t) c->tab_bytes[t] = -1;
    if (int rc = check_tail_params(who, alpha2, beta2, pvalue)) return rc;
    if ((double)n_sites * (double)n_cb >= 2147483648.0) { set_error("%s: %lld sites x %d barcodes", who, (long long)n_sites, n_cb); return -2; }
    if (reserve_cells(c, n_sites, n_cb)) return -1;
    if (n_sites > 0) {
        const size_t bytes = (size_t)n_sites * (size_t)n_cb * 4;
        LSG_HIP(hipMemcpyAsync(g.dp.p, dp, bytes, hipMemcpyHostToDevice, c->stream));
        LSG_HIP(hipMemcpyAsync(g.alt.p, alt, bytes, hipMemcpyHostToDevice, c->stream));
    }
    return classify(c, who, n_sites, n_cb, is_chrm, alpha2, beta2, pvalue);
}

int run_cellgeno_fetch(lsg_ctx* c, uint32_t* dp, uint32_t* alt, int32_t* vaf4, int32_t* p4, uint8_t* status, uint8_t* bin, int64_t* n_covered, int64_t* n_pass) {
    CellGeno& g = c->cg;
    if (!g.valid) { set_error("lsg_cellgeno_fetch: nothing classified (lsg_cellgeno_count first)"); return -2; }
    if (g.cells_only && (dp || alt || p4)) { set_error("lsg_cellgeno_fetch: the cells were loaded by lsg_cellgeno_load_cells: there are no dp, alt or p4"); return -2; }
    const size_t cells = (size_t)g.n_sites * (size_t)g.n_cb;
    auto get = [&](void* dst, const DevBuf& src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess; };
    LSG_HIP(get(dp, g.dp, cells * 4)); LSG_HIP(get(alt, g.alt, cells * 4)); LSG_HIP(get(vaf4, g.vaf4, cells * 4)); LSG_HIP(get(p4, g.p4, cells * 4));
    LSG_HIP(get(status, g.status, cells)); LSG_HIP(get(bin, g.bin, cells));
    LSG_HIP(get(n_covered, g.n_cov, (size_t)g.n_cb * 8)); LSG_HIP(get(n_pass, g.n_pass, (size_t)g.n_cb * 8));
    LSG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int run_cellgeno_set_text(lsg_ctx* c, const lsg_cellgeno_text* t) {
    const char* who = "lsg_cellgeno_set_text";
    CellGeno& g = c->cg;
    g.text_valid = g.filt_valid = false;
    for (int q = LSG_TABLE_CELL_LONG; q <= LSG_TABLE_BNPC_VAF; ++q) c->tab_bytes[q] = -1;
    if (!g.valid) { set_error("%s: nothing classified (lsg_cellgeno_count first)", who); return -2; }
    const int64_t S = g.n_sites; const int32_t B = g.n_cb;
    if (t->n_long < 0 || t->n_long > S || t->n_mat < 0 || t->n_mat > S || t->n_cols < 0 || (t->n_long > 0 && !t->long_order) || (t->n_mat > 0 && !t->mat_order) ||
        (t->n_cols > 0 && !t->col_src) || !t->head_off || !t->index_off || !t->label_off || !t->cb_off || !t->ct_off) { set_error("%s: bad arguments", who); return -2; }
    // every index a kernel follows is checked here
    auto offsets_ok = [](const uint32_t* off, int64_t n) { if (off[0] != 0) return false; for (int64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return false; return true; };
    if (!offsets_ok(t->head_off, S) || !offsets_ok(t->index_off, S) || !offsets_ok(t->label_off, S) || !offsets_ok(t->cb_off, B) || !offsets_ok(t->ct_off, B)) { set_error("%s: string offsets must start at 0 and ascend", who); return -2; }
    for (int64_t i = 0; i < t->n_long; ++i) if (t->long_order[i] < 0 || t->long_order[i] >= S) { set_error("%s: long_order[%lld] is not a site", who, (long long)i); return -2; }
    for (int64_t i = 0; i < t->n_mat; ++i) if (t->mat_order[i] < 0 || t->mat_order[i] >= S) { set_error("%s: mat_order[%lld] is not a site", who, (long long)i); return -2; }
    for (int32_t i = 0; i < t->n_cols; ++i) if (t->col_src[i] < -1 || t->col_src[i] >= B) { set_error("%s: col_src[%d] is not a barcode", who, i); return -2; }
    if ((double)t->n_long * (double)B >= 2147483648.0) { set_error("%s: %lld x %d rows", who, (long long)t->n_long, B); return -2; }
    const size_t n_head = t->head_off[S], n_index = t->index_off[S], n_label = t->label_off[S], n_cbt = t->cb_off[B], n_ctt = t->ct_off[B];
    if ((n_head && !t->head) || (n_index && !t->index) || (n_label && !t->label) || (n_cbt && !t->cb) || (n_ctt && !t->ct)) { set_error("%s: bad arguments", who); return -2; }
    HostBlob b;
    g.head_off_at = b.add(t->head_off, (size_t)(S + 1) * 4); g.index_off_at = b.add(t->index_off, (size_t)(S + 1) * 4); g.label_off_at = b.add(t->label_off, (size_t)(S + 1) * 4);
    g.cb_off_at = b.add(t->cb_off, (size_t)(B + 1) * 4); g.ct_off_at = b.add(t->ct_off, (size_t)(B + 1) * 4);
    g.long_order_at = b.add(t->long_order, (size_t)t->n_long * 4); g.mat_order_at = b.add(t->mat_order, (size_t)t->n_mat * 4); g.col_src_at = b.add(t->col_src, (size_t)t->n_cols * 4);
    g.head_at = b.add(t->head, n_head); g.index_at = b.add(t->index, n_index); g.label_at = b.add(t->label, n_label); g.cb_at = b.add(t->cb, n_cbt); g.ct_at = b.add(t->ct, n_ctt);
    if (b.upload(g.text, c->stream)) return -1;
    g.n_long = t->n_long; g.n_mat = t->n_mat; g.n_cols = t->n_cols; g.float_cells = t->float_cells ? 1 : 0;
    g.text_valid = true;
    return 0;
}

int run_cellgeno_load_cells(lsg_ctx* c, int64_t n_sites, int32_t n_cb, const uint8_t* bin, const int32_t* vaf4) {
    const char* who = "lsg_cellgeno_load_cells";
    CellGeno& g = c->cg;
    g.valid = g.text_valid = g.filt_valid = false;
    for (int t = LSG_TABLE_CELL_LONG; t <= LSG_TABLE_BNPC_VAF; ++t) c->tab_bytes[t] = -1;
    if ((double)n_sites * (double)n_cb >= 2147483648.0) { set_error("%s: %lld sites x %d barcodes", who, (long long)n_sites, n_cb); return -2; }
    const int64_t cells = n_sites * (int64_t)n_cb;
    for (int64_t i = 0; i < cells; ++i) {
        if (bin[i] != 0 && bin[i] != 1 && bin[i] != 3) { set_error("%s: bin[%lld] = %d is not 0, 1 or 3", who, (long long)i, (int)bin[i]); return -2; }
        if (vaf4[i] < -1) { set_error("%s: vaf4[%lld] = %d", who, (long long)i, vaf4[i]); return -2; }
    }
    const size_t room = (size_t)(cells > 0 ? cells : 1);
    if (g.bin.reserve(room) || g.status.reserve(room) || g.vaf4.reserve(room * 4) || g.n_cov.reserve((size_t)n_cb * 8) || g.n_pass.reserve((size_t)n_cb * 8)) return -1;
    hipStream_t st = c->stream;
    if (cells > 0) {
        LSG_HIP(hipMemcpyAsync(g.bin.p, bin, (size_t)cells, hipMemcpyHostToDevice, st));
        LSG_HIP(hipMemcpyAsync(g.vaf4.p, vaf4, (size_t)cells * 4, hipMemcpyHostToDevice, st));
        unsigned blocks = (unsigned)((cells + 255) / 256); if (blocks > (unsigned)(c->n_cus * 32)) blocks = (unsigned)(c->n_cus * 32);
        hipLaunchKernelGGL(k_cells_status, dim3(blocks), dim3(256), 0, st, g.bin.as<uint8_t>(), cells, g.status.as<uint8_t>());
    }
    hipLaunchKernelGGL(k_cell_tally, dim3((unsigned)((n_cb + 255) / 256)), dim3(256), 0, st, g.status.as<uint8_t>(), n_sites, n_cb, g.n_cov.as<int64_t>(), g.n_pass.as<int64_t>());
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { set_error("%s: kernel failed", who); return -1; }
    g.n_sites = n_sites; g.n_cb = n_cb; g.valid = true; g.cells_only = true;
    return 0;
}

int run_cellgeno_filter(lsg_ctx* c, int32_t min_mut, int32_t min_cov, const uint8_t* col_int_ok, int64_t* n_rows_kept, int32_t* n_cols_kept) {
    const char* who = "lsg_cellgeno_filter";
    if (n_rows_kept) *n_rows_kept = 0;
    if (n_cols_kept) *n_cols_kept = 0;
    CellGeno& g = c->cg;
    g.filt_valid = false;
    c->tab_bytes[LSG_TABLE_BNPC_BIN] = c->tab_bytes[LSG_TABLE_BNPC_VAF] = -1;
    if (!g.valid || !g.text_valid) { set_error("%s: needs the cells (lsg_cellgeno_count, _load_counts or _load_cells) and lsg_cellgeno_set_text first", who); return -2; }
    const int64_t R = g.n_mat; const int32_t N = g.n_cols;            // (every mat_order and col_src entry was checked by lsg_cellgeno_set_text)
    if (N > 0 && !col_int_ok) { set_error("%s: bad arguments", who); return -2; }
    size_t at = 0;
    auto place = [&](size_t bytes) { const size_t here = at; at = align_up(at + bytes, 256); return here; };
    g.f_row_mut_at = place((size_t)R * 4); g.f_cov_kept_at = place((size_t)N * 4); g.f_cov_all_at = place((size_t)N * 4);      // (the two counts adjacent: one memset)
    g.f_rows_at = place((size_t)R * 4); g.f_cols_at = place((size_t)N * 4); g.f_nsel_at = place(8);
    g.f_row_keep_at = place((size_t)R); g.f_col_keep_at = place((size_t)N); g.f_col_int_at = place((size_t)N); g.f_col_ok_at = place((size_t)N);
    if (g.filt.reserve(at + 256)) return -1;
    hipStream_t st = c->stream;
    char* f = g.filt.as<char>();
    const char* tx = g.text.as<char>();
    const int32_t* mat_order = reinterpret_cast<const int32_t*>(tx + g.mat_order_at);
    const int32_t* col_src = reinterpret_cast<const int32_t*>(tx + g.col_src_at);
    int32_t* row_mut = reinterpret_cast<int32_t*>(f + g.f_row_mut_at);
    int32_t* cov_kept = reinterpret_cast<int32_t*>(f + g.f_cov_kept_at); int32_t* cov_all = reinterpret_cast<int32_t*>(f + g.f_cov_all_at);
    int32_t* rows = reinterpret_cast<int32_t*>(f + g.f_rows_at); int32_t* cols = reinterpret_cast<int32_t*>(f + g.f_cols_at);
    int32_t* nsel = reinterpret_cast<int32_t*>(f + g.f_nsel_at);
    uint8_t* row_keep = reinterpret_cast<uint8_t*>(f + g.f_row_keep_at); uint8_t* col_keep = reinterpret_cast<uint8_t*>(f + g.f_col_keep_at);
    uint8_t* col_int = reinterpret_cast<uint8_t*>(f + g.f_col_int_at); uint8_t* col_ok = reinterpret_cast<uint8_t*>(f + g.f_col_ok_at);
    if (N > 0) LSG_HIP(hipMemsetAsync(cov_kept, 0, g.f_rows_at - g.f_cov_kept_at, st));
    LSG_HIP(hipMemsetAsync(nsel, 0, 8, st));
    if (N > 0) LSG_HIP(hipMemcpyAsync(col_ok, col_int_ok, (size_t)N, hipMemcpyHostToDevice, st));
    if (R > 0) hipLaunchKernelGGL(k_bnpc_row_count, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, g.bin.as<uint8_t>(), mat_order, col_src, R, N, g.n_cb, min_mut, row_mut, row_keep);
    if (R > 0 && N > 0) {
        const int64_t share = (R + 32767) / 32768 > 128 ? (R + 32767) / 32768 : 128;      // rows per workgroup: 128, more only to keep gridDim.y small
        hipLaunchKernelGGL(k_bnpc_col_count, dim3((unsigned)((N + 255) / 256), (unsigned)((R + share - 1) / share)), dim3(256), 0, st, g.bin.as<uint8_t>(), mat_order, col_src,
                           row_keep, R, N, g.n_cb, share, cov_kept, cov_all);
    }
    if (N > 0) hipLaunchKernelGGL(k_bnpc_col_flags, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, cov_kept, cov_all, col_ok, N, (int32_t)R, min_cov, col_keep, col_int);
    LSG_HIP(hipGetLastError());
    // the kept rows (as sites) and the kept columns, compacted in input order
    hipcub::CountingInputIterator<int32_t> iota(0);
    if (R > 0 && with_cub_tmp(c->d_cub_tmp, "hipcub::DeviceSelect::Flagged", [&](void* p, size_t& tb) { return hipcub::DeviceSelect::Flagged(p, tb, mat_order, row_keep, rows, nsel, (int)R, st); })) return -1;
    if (N > 0 && with_cub_tmp(c->d_cub_tmp, "hipcub::DeviceSelect::Flagged", [&](void* p, size_t& tb) { return hipcub::DeviceSelect::Flagged(p, tb, iota, col_keep, cols, nsel + 1, (int)N, st); })) return -1;
    LSG_HIP(hipMemcpyAsync(c->h_pin, nsel, 8, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipStreamSynchronize(st));
    int32_t got[2];
    memcpy(got, c->h_pin, 8);
    if (got[0] < 0 || got[0] > R || got[1] < 0 || got[1] > N) { set_error("%s: the selects kept %d of %lld rows, %d of %d columns", who, got[0], (long long)R, got[1], N); return -1; }
    g.n_rows_kept = got[0]; g.n_cols_kept = got[1]; g.filt_valid = true;
    if (n_rows_kept) *n_rows_kept = got[0];
    if (n_cols_kept) *n_cols_kept = got[1];
    return 0;
}

int run_cellgeno_filter_fetch(lsg_ctx* c, uint8_t* row_keep, uint8_t* col_keep, int32_t* row_mut, int32_t* col_cov_kept, int32_t* col_cov_all, uint8_t* col_int) {
    CellGeno& g = c->cg;
    if (!g.filt_valid) { set_error("lsg_cellgeno_filter_fetch: nothing filtered (lsg_cellgeno_filter first)"); return -2; }
    const char* f = g.filt.as<char>();
    auto get = [&](void* dst, size_t where, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, f + where, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess; };
    const size_t R = (size_t)g.n_mat, N = (size_t)g.n_cols;
    LSG_HIP(get(row_keep, g.f_row_keep_at, R)); LSG_HIP(get(col_keep, g.f_col_keep_at, N)); LSG_HIP(get(row_mut, g.f_row_mut_at, R * 4));
    LSG_HIP(get(col_cov_kept, g.f_cov_kept_at, N * 4)); LSG_HIP(get(col_cov_all, g.f_cov_all_at, N * 4)); LSG_HIP(get(col_int, g.f_col_int_at, N));
    LSG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int run_format_cell_table(lsg_ctx* c, int32_t table, int64_t* n_bytes) {
    if (n_bytes) *n_bytes = 0;
    CellGeno& g = c->cg;
    if (!g.valid || !g.text_valid) { set_error("lsg_format_table: table %d needs lsg_cellgeno_count and lsg_cellgeno_set_text first", table); return -2; }
    if (g.cells_only && (table == LSG_TABLE_CELL_LONG || table == LSG_TABLE_CELL_DP || table == LSG_TABLE_CELL_ALT)) {
        set_error("lsg_format_table: table %d needs counts, and the cells were loaded by lsg_cellgeno_load_cells", table); return -2;
    }
    const bool is_bnpc = table == LSG_TABLE_BNPC_BIN || table == LSG_TABLE_BNPC_VAF;
    if (is_bnpc && !g.filt_valid) { set_error("lsg_format_table: table %d needs lsg_cellgeno_filter first", table); return -2; }
    hipStream_t st = c->stream;
    const bool is_long = table == LSG_TABLE_CELL_LONG;
    const char* tx = g.text.as<char>();
    CellArgs a{};
    a.dp = g.dp.as<uint32_t>(); a.alt = g.alt.as<uint32_t>(); a.vaf4 = g.vaf4.as<int32_t>(); a.p4 = g.p4.as<int32_t>(); a.status = g.status.as<uint8_t>(); a.bin = g.bin.as<uint8_t>();
    a.n_cb = g.n_cb; a.n_cols = g.n_cols; a.float_cells = g.float_cells;
    a.kind = table == LSG_TABLE_CELL_DP ? M_DP : table == LSG_TABLE_CELL_ALT ? M_ALT : table == LSG_TABLE_CELL_VAF ? M_VAF : table == LSG_TABLE_BNPC_BIN ? M_BNPC_BIN :
             table == LSG_TABLE_BNPC_VAF ? M_BNPC_VAF : M_BIN;
    a.head = tx + g.head_at; a.index = tx + g.index_at; a.label = tx + g.label_at; a.cb = tx + g.cb_at; a.ct = tx + g.ct_at;
    a.head_off = reinterpret_cast<const uint32_t*>(tx + g.head_off_at); a.index_off = reinterpret_cast<const uint32_t*>(tx + g.index_off_at);
    a.label_off = reinterpret_cast<const uint32_t*>(tx + g.label_off_at); a.cb_off = reinterpret_cast<const uint32_t*>(tx + g.cb_off_at);
    a.ct_off = reinterpret_cast<const uint32_t*>(tx + g.ct_off_at);
    a.order = reinterpret_cast<const int32_t*>(tx + (is_long ? g.long_order_at : g.mat_order_at));
    a.col_src = reinterpret_cast<const int32_t*>(tx + g.col_src_at);
    a.n = is_long ? g.n_long * (int64_t)g.n_cb : g.n_mat;
    if (is_bnpc) {                                                   // the kept rows over the kept columns, both in input order (FormatInputBnpC.py:21-27)
        const char* f = g.filt.as<char>();
        a.order = reinterpret_cast<const int32_t*>(f + g.f_rows_at); a.n = g.n_rows_kept;
        a.col_sel = reinterpret_cast<const int32_t*>(f + g.f_cols_at); a.n_cols = g.n_cols_kept;
        a.col_int = reinterpret_cast<const uint8_t*>(f + g.f_col_int_at);
    }
    c->tab_bytes[table] = -1;
    if (a.n == 0) { c->tab_bytes[table] = 0; return 0; }
    RowPlaces r;
    if (row_places(g.scratch, a.n, -1, r)) return -1;
    a.len = r.len; a.off = r.off;
    const unsigned row_blocks = (unsigned)((a.n + 1 + 255) / 256);
    if (is_long) hipLaunchKernelGGL(k_cell_row_len, dim3(row_blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_cell_matrix<false>, dim3((unsigned)(a.n + 1)), dim3(256), 0, st, a);
    int64_t bytes = 0;
    if (finish_places(c, r, &bytes)) return -1;
    if (print_table(c, table, bytes, [&](char* text) {
            a.text = text;
            if (is_long) hipLaunchKernelGGL(k_cell_row_put, dim3(row_blocks), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(k_cell_matrix<true>, dim3((unsigned)a.n), dim3(256), 0, st, a);
        })) return -1;
    if (n_bytes) *n_bytes = bytes;
    return 0;
}

} // namespace lsg
