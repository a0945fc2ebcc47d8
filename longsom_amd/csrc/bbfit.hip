// The beta-binomial fit of the panel-of-normals branch (scripts/PoN/BetaBinEstimation.py) over the resident count rows: one pass per
// cell type that bins the six values of every kept row (k_bbfit_accumulate), and the maximum-likelihood solve over the bins
// (k_bbfit_solve).  The arithmetic, the start, the step rule and the stop are stated in longsom_amd/bbfit.py, whose numpy twin these
// kernels are held to.  (Compiled like the rest of the library, without fast-math: the filter's two proportions are IEEE double
// divisions compared against 0.10 and 0.15, as Python computes them.)
#include "lsg_ctx.h"
#include "philox.h"
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace lsg {

constexpr int BB_HISTS = 6;               // Alt_CC, Ref_CC, NC, Alt_BC, Ref_BC, DP
constexpr int BB_LDS_BINS = 1024;         // values below it are binned in LDS (32-bit bins, 24 KB a workgroup), flushed once per workgroup
enum { BB_SEEN = 0, BB_KEPT, BB_TOO_BIG, BB_BAD, BB_OUT_WORDS = 8 };      // BB_TOO_BIG: 1 + the largest value that did not fit; BB_BAD: bit 0 a row with DP or NC zero, bit 1 a row outside its table

struct BbAccArgs {
    const uint32_t* rows; uint64_t row_cap;
    const int2* geom; const uint64_t* mask; const uint32_t* rowbase; const uint32_t* rowoff;
    const uint8_t* const* ref_ptr; const uint8_t* ref_rows;
    uint32_t n_ne; int32_t ct; int64_t n_rows;
    unsigned long long* hist; int64_t cap; unsigned long long* out;
    uint64_t seed; uint32_t table; int32_t thin; double p_keep;
    int32_t probe;               // LSG_BBFIT_PROBE (measurement only, the histograms are left incomplete): 1 = read and filter, bin nothing; 2 = bin in LDS alone
};

struct __attribute__((packed, aligned(4))) BbQuad { uint32_t x, y, z, w; };

__device__ __forceinline__ void bb_bin(const BbAccArgs& a, uint32_t* bins, int h, int64_t v) {
    if (v >= a.cap || v < 0) atomicMax(&a.out[BB_TOO_BIG], (unsigned long long)(v < 0 ? 0 : v) + 1ull);
    else if (v < BB_LDS_BINS) atomicAdd(&bins[h * BB_LDS_BINS + (int)v], 1u);
    else if (a.probe != 2) atomicAdd(&a.hist[(int64_t)h * a.cap + v], 1ull);
}

// One wave per unit (the rows of one cell type in one 64-position tile, consecutive from the unit's row base), a lane per position.
// The lane's four 16-byte loads (planes 0-15: DP, NC, CC[0..7], BC[0..5] - quads 0-3 of the row's 9) are issued together and sit in no
// branch: a lane without a row reads the unit's first row.  A narrow unit (ROW_NARROW) holds the same planes as 16-bit values, 8
// bytes a quad at 512-byte steps.  The alleles summed are the six a BaseCellCounter table prints (A C T G I D, BaseCellCounter.py:300):
// the reference's script names eight but reads tables, so counts of N and O never reach its sums - they stay on the Ref side of
// DP - Alt here as there.
__global__ __launch_bounds__(256) void k_bbfit_accumulate(BbAccArgs a) {
    __shared__ uint32_t bins[BB_HISTS * BB_LDS_BINS];
    __shared__ unsigned long long s_cnt[2];
    for (int i = threadIdx.x; i < BB_HISTS * BB_LDS_BINS; i += 256) bins[i] = 0;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t stride = gridDim.x * 4u;
    uint32_t n_seen = 0, n_kept = 0;
    for (uint32_t w0 = blockIdx.x * 4u + (threadIdx.x >> 6); w0 < a.n_ne; w0 += stride) {
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)w0);
        const int2 geom = a.geom[w];
        if ((int)((uint32_t)geom.y >> 24) != a.ct) continue;
        const uint64_t em = a.mask[w];
        if (!em) continue;
        const uint32_t rb = a.rowbase[w];
        const bool narrow = (rb & ROW_NARROW) != 0;
        bool has = (em >> lane) & 1ull;
        const uint32_t rank = has ? (uint32_t)__popcll(em & below) : 0u;
        uint64_t row = (uint64_t)(rb & ~ROW_NARROW) + rank;
        uint64_t r = (uint64_t)a.rowoff[w] + rank;
        bool outside = row >= a.row_cap || (int64_t)r >= a.n_rows;
        if (outside) { row = 0; r = 0; }
        outside = outside && has;
        has = has && !outside;
        const char* R = reinterpret_cast<const char*>(a.rows + (row >> 6) * ROW_BLOCK_WORDS) + (narrow ? (row & 63) * 8 : (row & 63) * 16);
        const uint32_t step = narrow ? 512u : 1024u;
        BbQuad q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = *reinterpret_cast<const BbQuad*>(R + k * step);
        const int tid = geom.y & 0xffffff;
        const int64_t pos = (int64_t)geom.x + (has ? lane : (int)__builtin_ctzll(em));
        const uint8_t refb = a.ref_rows ? a.ref_rows[r] : a.ref_ptr[tid][pos];
        uint32_t v[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (narrow) { v[4 * k] = q[k].x & 0xffffu; v[4 * k + 1] = q[k].x >> 16; v[4 * k + 2] = q[k].y & 0xffffu; v[4 * k + 3] = q[k].y >> 16; }
            else { v[4 * k] = q[k].x; v[4 * k + 1] = q[k].y; v[4 * k + 2] = q[k].z; v[4 * k + 3] = q[k].w; }
        }
        // thinning comes before the filter, as the reference samples lines before it filters them
        bool seen = has;
        if (a.thin) {
            uint32_t pw[4];
            philox4x32(a.seed, a.table, (uint32_t)r, (uint32_t)(r >> 32), 0u, pw);
            seen = has && to_double(pw[0], pw[1]) < a.p_keep;
        }
        const int rsym = refb == 'A' ? 0 : refb == 'C' ? 1 : refb == 'T' ? 2 : refb == 'G' ? 3 : refb == 'I' ? 4 : refb == 'D' ? 5 : -1;
        const int64_t dp = v[0], nc = v[1];
        int64_t alt_cc = 0, alt_bc = 0;
#pragma unroll
        for (int s = 0; s < 6; ++s) { if (s != rsym) { alt_cc += v[2 + s]; alt_bc += v[10 + s]; } }
        const bool zero = seen && (dp == 0 || nc == 0);
        const bool keep = seen && !zero && (double)alt_cc / (double)nc < 0.10 && (double)alt_bc / (double)dp < 0.15;
        if (__ballot(zero || outside)) { if (zero) atomicOr(&a.out[BB_BAD], 1ull); if (outside) atomicOr(&a.out[BB_BAD], 2ull); }
        n_seen += (uint32_t)__popcll(__ballot(seen));
        const uint64_t km = __ballot(keep);
        if (!km || a.probe == 1) { n_kept += (uint32_t)__popcll(km); continue; }
        n_kept += (uint32_t)__popcll(km);
        // most kept rows have no alternative count at all: one LDS add per wave for those, not 64 to one address
        const uint64_t z0 = __ballot(keep && alt_cc == 0), z3 = __ballot(keep && alt_bc == 0);
        if (lane == 0) {
            if (z0) atomicAdd(&bins[0], (uint32_t)__popcll(z0));
            if (z3) atomicAdd(&bins[3 * BB_LDS_BINS], (uint32_t)__popcll(z3));
        }
        if (keep) {
            if (alt_cc) bb_bin(a, bins, 0, alt_cc);
            bb_bin(a, bins, 1, nc - alt_cc);
            bb_bin(a, bins, 2, nc);
            if (alt_bc) bb_bin(a, bins, 3, alt_bc);
            bb_bin(a, bins, 4, dp - alt_bc);
            bb_bin(a, bins, 5, dp);
        }
    }
    if (lane == 0 && n_seen) atomicAdd(&s_cnt[0], (unsigned long long)n_seen);
    if (lane == 0 && n_kept) atomicAdd(&s_cnt[1], (unsigned long long)n_kept);
    __syncthreads();
    for (int i = threadIdx.x; i < BB_HISTS * BB_LDS_BINS; i += 256) {
        const uint32_t n = bins[i];
        const int h = i / BB_LDS_BINS, val = i % BB_LDS_BINS;
        if (n && val < a.cap) atomicAdd(&a.hist[(int64_t)h * a.cap + val], (unsigned long long)n);
    }
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&a.out[threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ void k_bbfit_add(unsigned long long* hist, const unsigned long long* other, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hist[i] += other[i];
}

// ---- the solve -----------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 per fit.  Every sum is taken in the same order on every run: thread t adds the terms j = t, t + 256, ... in
// ascending j, the 256 partial sums are added pairwise in LDS (t with t + 128, t + 64, ...).  The three sums of the gradient, which
// cancel to nothing at the root, are carried as unevaluated pairs of doubles (quotient and the quotient of its remainder).
struct DD { double hi, lo; };
__device__ __forceinline__ DD two_sum(double a, double b) { const double s = a + b, bb = s - a; return DD{s, (a - (s - bb)) + (b - bb)}; }
__device__ __forceinline__ DD dd_add(DD a, DD b) { DD s = two_sum(a.hi, b.hi); const double e = s.lo + (a.lo + b.lo); const double h = s.hi + e; return DD{h, e - (h - s.hi)}; }

struct BbSolveArgs { const unsigned long long* hist; double* tails; int64_t cap; int32_t max_iter; double* est; lsg_bbfit_info* info; };

__device__ double bb_reduce(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) sh[t] += sh[t + o]; __syncthreads(); }
    return sh[0];
}
__device__ DD bb_reduce_dd(DD v, double* sh, double* sl) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v.hi; sl[t] = v.lo;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { const DD s = dd_add(DD{sh[t], sl[t]}, DD{sh[t + o], sl[t + o]}); sh[t] = s.hi; sl[t] = s.lo; }
        __syncthreads();
    }
    return DD{sh[0], sl[0]};
}
// sum_j T[j] / (v + v_lo + j) over j < n
__device__ DD bb_quot_sum(const double* T, int64_t n, double v, double v_lo, double* sh, double* sl) {
    DD acc{0.0, 0.0};
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        const double t = T[j];
        const DD d = two_sum(v, (double)j);
        const double e = d.lo + v_lo;
        const double q = t / d.hi;
        const double q2 = (fma(-q, d.hi, t) - q * e) / d.hi;
        const DD s = two_sum(acc.hi, q);
        acc.hi = s.hi; acc.lo += s.lo + q2;
    }
    const double h = acc.hi + acc.lo;
    return bb_reduce_dd(DD{h, acc.lo - (h - acc.hi)}, sh, sl);
}
__device__ double bb_sq_sum(const double* T, int64_t n, double v, double* sh) {
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) { const double r = 1.0 / (v + (double)j); acc += T[j] * r * r; }
    return bb_reduce(acc, sh);
}
__device__ double bb_loglik(const double* A, int64_t na, const double* B, int64_t nb, const double* Cc, int64_t nc, double a, double b, double* sh) {
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < na; j += 256) acc += A[j] * log(a + (double)j);
    double acc2 = 0.0;
    for (int64_t j = threadIdx.x; j < nb; j += 256) acc2 += B[j] * log(b + (double)j);
    double acc3 = 0.0;
    for (int64_t j = threadIdx.x; j < nc; j += 256) acc3 += Cc[j] * log(a + b + (double)j);
    return bb_reduce(acc, sh) + bb_reduce(acc2, sh) - bb_reduce(acc3, sh);
}

__global__ __launch_bounds__(256) void k_bbfit_solve(BbSolveArgs a) {
    __shared__ double sh[256], sl[256];
    __shared__ unsigned long long s_chunk[256];
    __shared__ long long s_len;
    const int f = blockIdx.x, t = threadIdx.x;
    int64_t len[3];                      // tail counts of histogram k: T[j], j < len[k] = its largest value
    double mom[3][3];                    // rows, sum of values, sum of squares
    for (int k = 0; k < 3; ++k) {
        const unsigned long long* h = a.hist + (int64_t)(3 * f + k) * a.cap;
        double* T = a.tails + (int64_t)(3 * f + k) * a.cap;
        if (t == 0) s_len = -1;
        __syncthreads();
        long long top = -1;
        for (int64_t i = t; i < a.cap; i += 256) if (h[i]) top = i;
        if (top >= 0) atomicMax(&s_len, top);
        __syncthreads();
        const int64_t n = s_len < 0 ? 0 : (int64_t)s_len;         // values 0..n are occupied; T[j] for j < n
        len[k] = n;
        // suffix sums: thread t owns the values [t * chunk, (t + 1) * chunk) of 0..n
        const int64_t chunk = (n + 1 + 255) / 256, lo = (int64_t)t * chunk, hi = lo + chunk < n + 1 ? lo + chunk : n + 1;
        unsigned long long own = 0;
        double m1 = 0.0, m2 = 0.0;
        for (int64_t i = lo; i < hi; ++i) own += h[i];
        s_chunk[t] = s_len < 0 ? 0ull : own;
        __syncthreads();
        unsigned long long after = 0, rows = 0;
        for (int u = 0; u < 256; ++u) { if (u > t) after += s_chunk[u]; rows += s_chunk[u]; }
        if (s_len >= 0)
            for (int64_t i = hi - 1; i >= lo; --i) { if (i < n) T[i] = (double)after; after += h[i]; }
        for (int64_t i = t; i <= n && s_len >= 0; i += 256) { const double c = (double)h[i], x = (double)i; m1 += c * x; m2 += c * x * x; }
        mom[k][0] = (double)rows; mom[k][1] = bb_reduce(m1, sh); mom[k][2] = bb_reduce(m2, sh);
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    const double* A = a.tails + (int64_t)(3 * f) * a.cap;
    const double* B = A + a.cap;
    const double* Cc = B + a.cap;
    int32_t iterations = 0, status = LSG_BBFIT_NO_DATA;
    double last_step = 0.0, grad_norm = 0.0, al = NAN, be = NAN;
    const double rows = mom[2][0], sx = mom[0][1], sxx = mom[0][2], sn = mom[2][1], snn = mom[2][2];
    if (rows > 0 && sn > 0) {
        // the start: method of moments from the marginal moments of x and n
        const double ex = sx / rows, ex2 = sxx / rows, en = sn / rows, en2 = snn / rows;
        const double p = fmin(fmax(ex / en, 1e-6), 1.0 - 1e-6), q = 1.0 - p, den = en2 - en;
        double rho = den > 0 ? ((ex2 - ex * ex - p * p * (en2 - en * en)) / (p * q) - en) / den : 0.0;
        if (!(rho > 1e-4)) rho = 1e-4;
        if (rho > 0.9999) rho = 0.9999;
        const double s = 1.0 / rho - 1.0;
        al = fmin(fmax(p * s, 1e-6), 1e6); be = fmin(fmax(q * s, 1e-6), 1e6);
        status = LSG_BBFIT_ITERATION_CAP;
        for (int it = 1; it <= a.max_iter; ++it) {
            const double a2 = bb_sq_sum(A, len[0], al, sh), b2 = bb_sq_sum(B, len[1], be, sh), c2 = bb_sq_sum(Cc, len[2], al + be, sh);
            const double l0 = bb_loglik(A, len[0], B, len[1], Cc, len[2], al, be, sh);
            const DD ab = two_sum(al, be);
            const DD qa = bb_quot_sum(A, len[0], al, 0.0, sh, sl), qb = bb_quot_sum(B, len[1], be, 0.0, sh, sl), qc = bb_quot_sum(Cc, len[2], ab.hi, ab.lo, sh, sl);
            const DD nqc{-qc.hi, -qc.lo};
            const DD ga = dd_add(qa, nqc), gb = dd_add(qb, nqc);
            const double g1 = al * (ga.hi + ga.lo), g2 = be * (gb.hi + gb.lo);
            double h11 = al * al * (c2 - a2) + g1, h22 = be * be * (c2 - b2) + g2;
            const double h12 = al * be * c2;
            const double disc = sqrt((h11 - h22) * (h11 - h22) + 4.0 * h12 * h12);
            const double lmax = 0.5 * (h11 + h22 + disc), lmin = 0.5 * (h11 + h22 - disc);      // H's eigenvalues
            if (!(lmax < 0)) {                    // not negative definite (a start far out on the ridge): shifted until it is
                const double shift = lmax + 0.01 * fmax(fabs(lmin), fabs(lmax));
                h11 -= shift; h22 -= shift;
            }
            const double det = h11 * h22 - h12 * h12;
            double d1 = -(h22 * g1 - h12 * g2) / det, d2 = -(h11 * g2 - h12 * g1) / det;
            double m = fmax(fabs(d1), fabs(d2));
            if (m > 2.0) { d1 *= 2.0 / m; d2 *= 2.0 / m; m = 2.0; }
            iterations = it; last_step = m; grad_norm = hypot(g1, g2);
            if (!(m == m) || d1 != d1 || d2 != d2) { last_step = NAN; status = LSG_BBFIT_NO_FINITE_MAXIMUM; break; }
            if (m < 1e-12) { al *= exp(d1); be *= exp(d2); status = LSG_BBFIT_CONVERGED; break; }
            double step = 1.0, na = al, nb = be;
            for (int hv = 0; hv < 30; ++hv) {
                na = al * exp(step * d1); nb = be * exp(step * d2);
                const double l1 = bb_loglik(A, len[0], B, len[1], Cc, len[2], na, nb, sh);
                if (l1 >= l0 - 1e-10 * fabs(l0)) break;
                step *= 0.5;
            }
            al = na; be = nb;
            if (!(al >= 1e-8 && al <= 1e8 && be >= 1e-8 && be <= 1e8)) { status = LSG_BBFIT_NO_FINITE_MAXIMUM; break; }
        }
    }
    if (t == 0) {
        a.est[2 * f] = al; a.est[2 * f + 1] = be;
        a.info->iterations[f] = iterations; a.info->status[f] = status; a.info->last_step[f] = last_step; a.info->grad_norm[f] = grad_norm;
    }
}

static int bb_ready(lsg_ctx* c, const char* who) {
    if (!c) { set_error("%s: NULL handle", who); return -2; }
    if (!c->bb.valid) { set_error("%s: call lsg_bbfit_reset first", who); return -2; }
    return 0;
}

} // namespace lsg

using namespace lsg;

extern "C" {

int lsg_bbfit_reset(lsg_ctx* c, int64_t capacity) {
    if (!c) { set_error("lsg_bbfit_reset: NULL handle"); return -2; }
    if (capacity < 1 || capacity > ((int64_t)1 << 28)) { set_error("lsg_bbfit_reset: capacity %lld not in [1, 2^28]", (long long)capacity); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    Bbfit& b = c->bb;
    b.valid = false;
    const size_t bytes = (size_t)BB_HISTS * (size_t)capacity * 8;
    if (b.hist.reserve(bytes) || b.tails.reserve(bytes) || b.out.reserve(BB_OUT_WORDS * 8 + 4 * 8 + sizeof(lsg_bbfit_info))) return -1;
    LSG_HIP(hipMemsetAsync(b.hist.p, 0, bytes, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    b.cap = capacity; b.valid = true;
    return 0;
}

int lsg_bbfit_accumulate(lsg_ctx* c, int32_t ct, const uint8_t* ref_or_null, int32_t table, int64_t sample_n, uint64_t seed, int64_t* n_rows_seen, int64_t* n_rows_kept) {
    if (int rc = bb_ready(c, "lsg_bbfit_accumulate")) return rc;
    if (!c->counted) { set_error("lsg_bbfit_accumulate: no count rows are resident (lsg_pileup_count or lsg_load_counts first)"); return -2; }
    if (ct < 0 || ct >= c->n_ct) { set_error("lsg_bbfit_accumulate: bad cell type %d", ct); return -2; }
    if (table < 0) { set_error("lsg_bbfit_accumulate: bad table index %d", table); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    if (n_rows_seen) *n_rows_seen = 0;
    if (n_rows_kept) *n_rows_kept = 0;
    const int64_t n = c->n_rows[ct];
    if (n == 0 || c->n_ne == 0) return 0;
    if (!ref_or_null)
        for (int t = 0; t < c->n_contigs; ++t)
            if (!c->ref_ptr[t]) { set_error("lsg_bbfit_accumulate: reference of contig %d not loaded and no REF column given", t); return -2; }
    hipStream_t st = c->stream;
    Bbfit& b = c->bb;
    BbAccArgs a{};
    if (ref_or_null) {
        if (b.ref.reserve((size_t)n)) return -1;
        LSG_HIP(hipMemcpyAsync(b.ref.p, ref_or_null, (size_t)n, hipMemcpyHostToDevice, st));
        a.ref_rows = b.ref.as<uint8_t>();
    }
    const uint32_t* off = nullptr;
    if (int rc = unit_row_offsets(c, ct, &off)) return rc;
    LSG_HIP(hipMemsetAsync(b.out.p, 0, BB_OUT_WORDS * 8, st));
    a.rows = c->d_rows[ct].as<uint32_t>(); a.row_cap = c->row_cap;
    a.geom = c->ws[WS_NE_GEOM].as<int2>(); a.mask = c->d_ne_mask.as<uint64_t>(); a.rowbase = c->d_ne_rowbase.as<uint32_t>(); a.rowoff = off;
    a.ref_ptr = c->d_ref_ptrs.as<const uint8_t*>();
    a.n_ne = c->n_ne; a.ct = ct; a.n_rows = n;
    a.hist = b.hist.as<unsigned long long>(); a.cap = b.cap; a.out = b.out.as<unsigned long long>();
    a.seed = seed; a.table = (uint32_t)table;
    a.thin = sample_n > 0 && n > sample_n; a.p_keep = a.thin ? (double)sample_n / (double)n : 1.0;
    const char* probe = getenv("LSG_BBFIT_PROBE");
    a.probe = probe && *probe ? atoi(probe) : 0;
    const uint32_t want = (c->n_ne + 3) / 4, most = (uint32_t)c->n_cus * 4u;
    hipLaunchKernelGGL(k_bbfit_accumulate, dim3(want < most ? want : most), dim3(256), 0, st, a);
    LSG_HIP(hipGetLastError());
    LSG_HIP(hipMemcpyAsync(c->h_pin, b.out.p, BB_OUT_WORDS * 8, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipStreamSynchronize(st));
    unsigned long long out[BB_OUT_WORDS];
    memcpy(out, c->h_pin, sizeof(out));
    if (out[BB_BAD] || out[BB_TOO_BIG]) {
        b.valid = false;                  // (some of the pass's rows are in the bins already)
        if (out[BB_BAD] & 2ull) set_error("lsg_bbfit_accumulate: a row of cell type %d lies outside its table", ct);
        else if (out[BB_BAD]) set_error("lsg_bbfit_accumulate: a count row of cell type %d has DP or NC zero", ct);
        else set_error("lsg_bbfit_accumulate: value %llu does not fit the histograms' capacity %lld", out[BB_TOO_BIG] - 1ull, (long long)b.cap);
        return -2;
    }
    if (n_rows_seen) *n_rows_seen = (int64_t)out[BB_SEEN];
    if (n_rows_kept) *n_rows_kept = (int64_t)out[BB_KEPT];
    if (a.probe) b.valid = false;         // (a probe's histograms are not the data's: nothing may read them)
    return 0;
}

int lsg_bbfit_fetch(lsg_ctx* c, uint64_t* hist) {
    if (int rc = bb_ready(c, "lsg_bbfit_fetch")) return rc;
    if (!hist) { set_error("lsg_bbfit_fetch: hist is NULL"); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    LSG_HIP(hipMemcpyAsync(hist, c->bb.hist.p, (size_t)BB_HISTS * (size_t)c->bb.cap * 8, hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int lsg_bbfit_add(lsg_ctx* c, const uint64_t* hist) {
    if (int rc = bb_ready(c, "lsg_bbfit_add")) return rc;
    if (!hist) { set_error("lsg_bbfit_add: hist is NULL"); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    Bbfit& b = c->bb;
    const int64_t n = (int64_t)BB_HISTS * b.cap;
    if (b.tmp.reserve((size_t)n * 8)) return -1;
    LSG_HIP(hipMemcpyAsync(b.tmp.p, hist, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_bbfit_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, b.hist.as<unsigned long long>(), b.tmp.as<unsigned long long>(), n);
    LSG_HIP(hipGetLastError());
    LSG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int lsg_bbfit_solve(lsg_ctx* c, double* est, lsg_bbfit_info* info, int32_t max_iter) {
    if (int rc = bb_ready(c, "lsg_bbfit_solve")) return rc;
    if (!est || !info) { set_error("lsg_bbfit_solve: est or info is NULL"); return -2; }
    if (max_iter < 0 || max_iter > 100000) { set_error("lsg_bbfit_solve: max_iter %d not in [0, 100000]", max_iter); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    Bbfit& b = c->bb;
    BbSolveArgs a{};
    char* res = b.out.as<char>() + BB_OUT_WORDS * 8;
    a.hist = b.hist.as<unsigned long long>(); a.tails = b.tails.as<double>(); a.cap = b.cap; a.max_iter = max_iter ? max_iter : 100;
    a.est = reinterpret_cast<double*>(res); a.info = reinterpret_cast<lsg_bbfit_info*>(res + 4 * 8);
    hipLaunchKernelGGL(k_bbfit_solve, dim3(2), dim3(256), 0, c->stream, a);
    LSG_HIP(hipGetLastError());
    LSG_HIP(hipMemcpyAsync(c->h_pin, res, 4 * 8 + sizeof(lsg_bbfit_info), hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    memcpy(est, c->h_pin, 4 * 8);
    memcpy(info, reinterpret_cast<char*>(c->h_pin) + 4 * 8, sizeof(lsg_bbfit_info));
    return 0;
}

} // extern "C"
