// The BAM index on the device: a coordinate-sorted BAM's .bai - bins, chunks, the pseudo-bins, the linear index, n_no_coor - as the bytes of
// the file (include/longsom_hip.h lsg_bam_index has the contract, DESIGN.md section 16 the reasons).  Replaces samtools index / pysam.index
// (SplitBamCellTypes.py:189-192, rule IndexBarcodedBam_PoN); the host twin is lsio_build_bai_full (hostio/bamio.cpp).  What both share
// is bamindex_core.h.
//   k_bai_facts     one LANE per record: refID, pos, flag 0x4, the interval's end from the CIGAR; a CIGAR of more than 64 operations is
//                   summed by the whole wave (65 535 operations: 1 024 rounds of 64 lanes instead of one lane's 65 535)
//   k_bai_check     the order (a record's key against its predecessor's), pos < 0, an end beyond 2^29: the smallest (ordinal << 3 | kind)
//                   by a 64-bit atomicMin; the placed records; per reference the last window touched, one atomicMax per wave where the
//                   wave's records lie on one reference
//   k_bai_voff      every record's virtual offset: its stream offset looked up in the table of the file's non-empty blocks
//   k_bai_keys      (refID, bin) per record, and (refID, last window) for the running maximum the linear index reads
//   scans, k_bai_runs   head flags where (refID, bin) changes -> the run list: key, first record's start, last record's end
//   radix sort      the runs by (refID, bin), stable: file order breaks ties (hipcub)
//   scans           chunk heads (a run that does not merge into its predecessor), bin heads -> chunk and bin numbers
//   k_bai_refs      per reference: its records, runs, bins, chunks, windows by binary search over the sorted arrays; its bytes
//   k_bai_lin       one thread per window: the first record whose running-maximum window reaches it (a binary search, no atomics: in a
//                   sorted file that record has the smallest start of all that overlap the window, however many do); a max-scan fills
//                   the unset windows
//   k_bai_print_*   the file's bytes at the places the scans give
#include "bamindex.h"
#include "bamindex_core.h"
#include "ingest_front.h"
#include "bamrec_core.h"
#include "cub_tmp.h"
#include <chrono>

namespace lsg {

constexpr uint32_t BAI_LONG_CIGAR = 64;       // operations up to which a lane sums its own CIGAR

struct BaiFactArgs {
    const uint8_t* u; uint64_t total; const uint64_t* rec_off; const uint32_t* sel; uint64_t n; int32_t n_ref;
    const unsigned long long* g_src; unsigned long long g_sub;
    int32_t* tid; int32_t* pos; int32_t* end; uint8_t* unm; unsigned long long* g; uint32_t* status;
};
__global__ __launch_bounds__(256) void k_bai_facts(BaiFactArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = j < a.n;
    int32_t tid = -1, pos = -1;
    uint32_t n_cigar = 0, flag = 0;
    const uint8_t* cg = nullptr;
    unsigned long long g = 0;
    bool ok = false;
    if (live) {
        const uint64_t i = a.sel ? (uint64_t)a.sel[j] : j;
        const uint64_t p = a.rec_off[i];
        g = a.g_src ? a.g_src[i] - a.g_sub : (unsigned long long)p;
        if (p + 4 > a.total) atomicOr(a.status, 2u);
        else {
            const uint32_t bs = lsr::rd32(a.u + p);
            const uint8_t* rec = a.u + p + 4;
            if (p + 4ull + bs > a.total) atomicOr(a.status, 2u);
            else if (bs < 32) { atomicOr(a.status, 8u); atomicMin(a.status + 2, (uint32_t)lsr::REC_SHORT); }
            else {
                const uint64_t l_name = rec[8], l_seq = lsr::rd32(rec + 16);
                n_cigar = lsr::rd16(rec + 12);
                if (32 + l_name + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq > (uint64_t)bs) { atomicOr(a.status, 8u); atomicMin(a.status + 2, (uint32_t)lsr::REC_FIELDS); }
                else if ((int32_t)lsr::rd32(rec) >= a.n_ref) { atomicOr(a.status, 8u); atomicMin(a.status + 2, (uint32_t)lsr::REC_TID); }
                else { ok = true; tid = (int32_t)lsr::rd32(rec); pos = (int32_t)lsr::rd32(rec + 4); flag = lsr::rd16(rec + 14); cg = rec + 32 + l_name; }
            }
        }
    }
    long long rlen = 0;
    if (ok && n_cigar <= BAI_LONG_CIGAR) rlen = lsb::cigar_rlen(cg, n_cigar, 0, 1);
    // the long CIGARs of this wave, one after the other, 64 operations a round (every lane of the wave is here: nothing above returns)
    unsigned long long m = __ballot(ok && n_cigar > BAI_LONG_CIGAR);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const unsigned long long cp = __shfl((unsigned long long)reinterpret_cast<uintptr_t>(cg), src);
        const uint32_t nc = (uint32_t)__shfl((int)n_cigar, src);
        long long part = lsb::cigar_rlen(reinterpret_cast<const uint8_t*>((uintptr_t)cp), nc, lane, 64u);
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if ((int)lane == src) rlen = part;
    }
    if (live) {
        const int64_t end = lsb::interval_end(pos, rlen);
        a.tid[j] = tid; a.pos[j] = pos; a.end[j] = (int32_t)(end > lsb::MAX_END + 1 ? lsb::MAX_END + 1 : end);
        a.unm[j] = (uint8_t)((flag >> 2) & 1u); a.g[j] = g;
    }
}

// small[0]: the smallest (ordinal << 3 | kind) refused (~0: none); small[1]: the placed records
__global__ __launch_bounds__(256) void k_bai_check(const int32_t* tid, const int32_t* pos, const int32_t* end, uint64_t n, uint32_t* n_intv, unsigned long long* small) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    int32_t t = -1;
    uint32_t w = 0;
    bool has = false;
    if (j < n) {
        t = tid[j];
        const int32_t ps = pos[j];
        int kind = j > 0 && lsb::sort_key(t, ps) < lsb::sort_key(tid[j - 1], pos[j - 1]) ? (int)lsb::ERR_UNSORTED : lsb::record_error(t, ps, (int64_t)end[j]);
        if (kind) atomicMin(small, (unsigned long long)((j << 3) | (uint64_t)kind));
        has = t >= 0 && !kind;
        if (has) w = (uint32_t)((end[j] - 1) >> lsb::WIN_SHIFT) + 1u;
    }
    const unsigned long long placed = __ballot(t >= 0), mh = __ballot(has);
    if (lane == 0 && placed) atomicAdd(small + 1, (unsigned long long)__popcll(placed));
    if (mh) {                                                    // one atomic a wave where its records lie on one reference (the usual case)
        const int first = __ffsll((long long)mh) - 1;
        const int32_t t0 = __shfl(t, first);
        if (__all(!has || t == t0)) {
            uint32_t wm = w;
            for (int o = 32; o > 0; o >>= 1) { const uint32_t x = (uint32_t)__shfl_xor((int)wm, o); wm = x > wm ? x : wm; }
            if ((int)lane == first) atomicMax(n_intv + t0, wm);
        } else if (has) atomicMax(n_intv + t, w);
    }
}

// vs[j] (j < n): the virtual offset of stream offset g[j], by the non-empty blocks' starts (ustart ascending, ustart[0] = 0); vs[n] = v_eof
__global__ void k_bai_voff(const unsigned long long* g, uint64_t n, const unsigned long long* ustart, const unsigned long long* coff, uint32_t n_blk, unsigned long long v_eof,
                           unsigned long long* vs) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) { vs[n] = v_eof; return; }
    const unsigned long long x = g[j];
    uint32_t lo = 0, hi = n_blk;                                // the last block with ustart <= x
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (ustart[mid] <= x) lo = mid; else hi = mid; }
    vs[j] = (coff[lo] << 16) | (x - ustart[lo]);
}

__global__ void k_bai_keys(const int32_t* tid, const int32_t* pos, const int32_t* end, uint32_t n_placed, unsigned long long* key, unsigned long long* wkey) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_placed) return;
    key[j] = lsb::bin_key(tid[j], lsb::reg2bin(pos[j], end[j]));
    wkey[j] = ((unsigned long long)(uint32_t)tid[j] << 32) | (unsigned long long)(uint32_t)((end[j] - 1) >> lsb::WIN_SHIFT);
}

struct BaiRunHead {
    const unsigned long long* key; uint32_t n;
    __host__ __device__ uint32_t operator()(const uint32_t& i) const { return i < n && (i == 0 || key[i] != key[i - 1]) ? 1u : 0u; }
};
struct BaiChunkHead {                                          // over the sorted runs: a run that does not merge into the one before it
    const unsigned long long* key; const uint32_t* idx; const unsigned long long* vb; const unsigned long long* ve; uint32_t n;
    __host__ __device__ uint32_t operator()(const uint32_t& i) const {
        return i < n && (i == 0 || key[i] != key[i - 1] || !lsb::chunks_merge(ve[idx[i - 1]], vb[idx[i]])) ? 1u : 0u;
    }
};
struct BaiUnmapped { const uint8_t* unm; uint32_t n; __host__ __device__ uint32_t operator()(const uint32_t& i) const { return i < n ? (uint32_t)unm[i] : 0u; } };
using BaiIota = hipcub::CountingInputIterator<uint32_t>;
template <class F> using BaiIt = hipcub::TransformInputIterator<uint32_t, F, BaiIota>;

// rid: exclusive count of run heads (rid[j] of a head: its run; rid[n_placed]: the runs)
__global__ void k_bai_runs(BaiRunHead head, const uint32_t* rid, const unsigned long long* vs, unsigned long long* run_key, unsigned long long* run_vb, unsigned long long* run_ve,
                           uint32_t* run_idx) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= head.n) return;
    if (head(j)) { const uint32_t r = rid[j]; run_key[r] = head.key[j]; run_vb[r] = vs[j]; run_idx[r] = r; }
    if (j + 1 == head.n || head(j + 1)) run_ve[rid[j + 1] - 1u] = vs[j + 1];
}

// bin_c0[b]: the first chunk of bin b; bin_c0[n_bins] = the chunks
__global__ void k_bai_binfirst(BaiRunHead bin_head, const uint32_t* bid, const uint32_t* cid, uint32_t* bin_c0) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > bin_head.n) return;
    if (s == bin_head.n || bin_head(s)) bin_c0[bid[s]] = cid[s];
}

struct BaiRef { uint32_t rec_lo, rec_hi, b0, c0, nb, nc, n_intv, pad_; };
__device__ __forceinline__ uint32_t bai_lower_tid(const int32_t* tid, uint32_t n, int64_t want) {       // the first j with tid[j] >= want
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if ((int64_t)tid[mid] < want) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ uint32_t bai_lower_run(const unsigned long long* key, uint32_t n, uint64_t want_tid) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if ((key[mid] >> 16) < want_tid) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ void k_bai_refs(const int32_t* tid, uint32_t n_placed, const unsigned long long* key_s, uint32_t n_runs, const uint32_t* bid, const uint32_t* cid, const uint32_t* n_intv,
                           int32_t n_ref, BaiRef* refs, unsigned long long* ref_size, unsigned long long* win_n) {
    const int32_t r = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n_ref) return;
    BaiRef x{};
    x.rec_lo = bai_lower_tid(tid, n_placed, r); x.rec_hi = bai_lower_tid(tid, n_placed, (int64_t)r + 1);
    if (n_runs) {
        const uint32_t lo = bai_lower_run(key_s, n_runs, (uint64_t)r), hi = bai_lower_run(key_s, n_runs, (uint64_t)r + 1);
        x.b0 = bid[lo]; x.c0 = cid[lo]; x.nb = bid[hi] - bid[lo]; x.nc = cid[hi] - cid[lo];
    }
    x.n_intv = x.rec_hi > x.rec_lo ? n_intv[r] : 0u;
    refs[r] = x;
    ref_size[r] = lsb::ref_bytes(x.nb, x.nc, x.rec_hi > x.rec_lo, x.n_intv);
    win_n[r] = x.n_intv;
}

// the reference of window x of all: the r with win_off[r] <= x < win_off[r + 1]
__device__ __forceinline__ int32_t bai_ref_of_window(const unsigned long long* win_off, int32_t n_ref, unsigned long long x) {
    int32_t lo = 0, hi = n_ref;                                 // the first r with win_off[r + 1] > x
    while (lo < hi) { const int32_t mid = lo + (hi - lo) / 2; if (win_off[mid + 1] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}
// pm: the running maximum of (refID << 32 | last window) over the records.  Window w of a reference is first reached by the first record
// i whose pm's window is >= w; if that record starts at or before w it overlaps w and, the file being sorted, starts first of all that do.
// Otherwise nothing overlaps w: 0, or the reference's first start where w lies before its first record.
__global__ void k_bai_lin(const unsigned long long* pm, const int32_t* pos, const unsigned long long* vs, const BaiRef* refs, const unsigned long long* win_off, int32_t n_ref,
                          unsigned long long n_win, unsigned long long* lin) {
    const unsigned long long x = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_win) return;
    const int32_t r = bai_ref_of_window(win_off, n_ref, x);
    const BaiRef f = refs[r];
    const uint32_t w = (uint32_t)(x - win_off[r]);
    uint32_t lo = f.rec_lo, hi = f.rec_hi - 1u;                 // (w < n_intv: the last record's running maximum reaches it)
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if ((uint32_t)pm[mid] < w) lo = mid + 1; else hi = mid; }
    unsigned long long v = 0;
    if ((uint32_t)(pos[lo] >> lsb::WIN_SHIFT) <= w) v = vs[lo];
    else if (w < (uint32_t)(pos[f.rec_lo] >> lsb::WIN_SHIFT)) v = vs[f.rec_lo];
    lin[x] = v;
}

struct BaiPrint {
    uint8_t* out; const BaiRef* refs; const unsigned long long* ref_off; int32_t n_ref;
    const unsigned long long* key_s; const uint32_t* idx_s; const unsigned long long* run_vb; const unsigned long long* run_ve; uint32_t n_runs;
    const uint32_t* bid; const uint32_t* cid; const uint32_t* bin_c0;
    const unsigned long long* vs; const uint32_t* pu;           // pu: exclusive count of the unmapped records
    const unsigned long long* win_off; const unsigned long long* lin; unsigned long long n_win, n_no_coor, n_bytes;
};
// one thread per sorted run: a bin head writes the bin's number and chunk count, a chunk's first run its start, its last run its end
__global__ void k_bai_print_runs(BaiPrint a, BaiChunkHead chunk_head, BaiRunHead bin_head) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_runs) return;
    const int32_t r = (int32_t)(a.key_s[s] >> 16);
    const BaiRef f = a.refs[r];
    uint8_t* o = a.out + lsb::HEAD_BYTES + a.ref_off[r];
    const uint32_t b = a.bid[s + 1] - 1u, ch = a.cid[s + 1] - 1u;      // the run's bin and chunk (heads up to and including s)
    if (bin_head(s)) {
        uint8_t* q = o + lsb::bin_at(b - f.b0, ch - f.c0);
        lsb::put32(q, (uint32_t)(a.key_s[s] & 0xffffu)); lsb::put32(q + 4, a.bin_c0[b + 1] - a.bin_c0[b]);
    }
    uint8_t* q = o + lsb::chunk_at(b - f.b0, ch - f.c0);
    if (chunk_head(s)) lsb::put64(q, a.run_vb[a.idx_s[s]]);
    if (s + 1 == a.n_runs || chunk_head(s + 1)) lsb::put64(q + 8, a.run_ve[a.idx_s[s]]);
}
// one thread per reference: n_bin, the pseudo-bin, n_intv; one more: the file's head and n_no_coor
__global__ void k_bai_print_refs(BaiPrint a) {
    const int32_t r = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r > a.n_ref) return;
    if (r == a.n_ref) { lsb::put_head(a.out, (uint32_t)a.n_ref); lsb::put64(a.out + a.n_bytes - lsb::TAIL_BYTES, a.n_no_coor); return; }
    const BaiRef f = a.refs[r];
    const bool has = f.rec_hi > f.rec_lo;
    uint8_t* o = a.out + lsb::HEAD_BYTES + a.ref_off[r];
    lsb::put32(o, f.nb + (has ? 1u : 0u));
    if (has) {
        const uint32_t n_unm = a.pu[f.rec_hi] - a.pu[f.rec_lo];
        lsb::put_meta(o + lsb::meta_at(f.nb, f.nc), a.vs[f.rec_lo], a.vs[f.rec_hi], (uint64_t)(f.rec_hi - f.rec_lo - n_unm), (uint64_t)n_unm);
    }
    lsb::put32(o + lsb::intv_at(f.nb, f.nc, has), f.n_intv);
}
__global__ void k_bai_print_lin(BaiPrint a) {
    const unsigned long long x = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.n_win) return;
    const int32_t r = bai_ref_of_window(a.win_off, a.n_ref, x);
    const BaiRef f = a.refs[r];
    lsb::put64(a.out + lsb::HEAD_BYTES + a.ref_off[r] + lsb::intv_at(f.nb, f.nc, true) + 4 + 8 * (x - a.win_off[r]), a.lin[x]);
}

const char* bai_err_text(int kind) {                    // lsio_build_bai_full's texts
    switch (kind) {
        case lsb::ERR_UNSORTED: return "the file is not coordinate-sorted here";
        case lsb::ERR_NEG_POS: return "it is placed on a reference at a negative position";
        case lsb::ERR_TOO_FAR: return "it ends beyond 2^29, which a .bai cannot hold";
        default: return "?";
    }
}
static int bai_reserve(DevBuf& b, size_t bytes, const char* who, const char* what) {
    if (b.reserve(bytes) == 0) return 0;
    (void)hipGetLastError();
    set_error("%s: no device memory for %s (%zu bytes)", who, what, bytes);
    return -3;
}
static unsigned bai_grid(uint64_t n) { return (unsigned)((n + 255) / 256); }

int bai_facts(lsg_ctx* c, const char* who, const uint8_t* u, uint64_t total, const uint64_t* rec_off, const uint32_t* sel, uint64_t n, int32_t n_ref,
              const unsigned long long* g_src, unsigned long long g_sub, uint32_t* status, BaiFacts& f, lsg_bai_info* info) {
    hipStream_t st = c->stream;
    f.n = n; f.n_ref = n_ref; f.n_placed = 0;
    info->n_records = (int64_t)n;
    if (int rc = bai_reserve(f.tid, (n + 1) * 4, who, "the records' references")) return rc;
    if (int rc = bai_reserve(f.pos, (n + 1) * 4, who, "the records' positions")) return rc;
    if (int rc = bai_reserve(f.end, (n + 1) * 4, who, "the records' ends")) return rc;
    if (int rc = bai_reserve(f.unm, n + 16, who, "the records' flags")) return rc;
    if (int rc = bai_reserve(f.g, (n + 1) * 8, who, "the records' offsets")) return rc;
    if (int rc = bai_reserve(f.n_intv, ((size_t)n_ref + 1) * 4, who, "the references' windows")) return rc;
    if (int rc = bai_reserve(f.small, 16, who, "the counters")) return rc;
    LSG_HIP(hipMemsetAsync(f.n_intv.p, 0, ((size_t)n_ref + 1) * 4, st));
    LSG_HIP(hipMemsetAsync(f.small.p, 0xff, 8, st));
    LSG_HIP(hipMemsetAsync(f.small.as<unsigned long long>() + 1, 0, 8, st));
    if (!n) return 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto done = [&](int rc) { for (auto& e : ev) if (e) (void)hipEventDestroy(e); return rc; };
    for (auto& e : ev) LSG_HIP_OR(hipEventCreate(&e), done(-1));
    LSG_HIP_OR(hipMemsetAsync(status, 0, 4, st), done(-1));
    LSG_HIP_OR(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(status + 2), (int)0x7fffffff, 1, st), done(-1));
    LSG_HIP_OR(hipEventRecord(ev[0], st), done(-1));
    BaiFactArgs a{u, total, rec_off, sel, n, n_ref, g_src, g_sub, f.tid.as<int32_t>(), f.pos.as<int32_t>(), f.end.as<int32_t>(), f.unm.as<uint8_t>(), f.g.as<unsigned long long>(), status};
    hipLaunchKernelGGL(k_bai_facts, dim3(bai_grid(n)), dim3(256), 0, st, a);
    uint32_t hstat[4] = {0, 0, 0, 0};
    LSG_HIP_OR(hipMemcpyAsync(hstat, status, 16, hipMemcpyDeviceToHost, st), done(-1));
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    if (hstat[0]) {
        static const char* why[] = {"", "a record shorter than its fixed fields", "a record whose fields exceed its block_size", "a record on a reference the header does not list"};
        set_error("%s: %s", who, (hstat[0] & 8u) && hstat[2] < 4 ? why[hstat[2]] : "truncated record at the end of the file");
        return done(-1);
    }
    hipLaunchKernelGGL(k_bai_check, dim3(bai_grid(n)), dim3(256), 0, st, f.tid.as<int32_t>(), f.pos.as<int32_t>(), f.end.as<int32_t>(), n, f.n_intv.as<uint32_t>(),
                       f.small.as<unsigned long long>());
    LSG_HIP_OR(hipEventRecord(ev[1], st), done(-1));
    unsigned long long h_small[2] = {~0ull, 0};
    LSG_HIP_OR(hipMemcpyAsync(h_small, f.small.p, 16, hipMemcpyDeviceToHost, st), done(-1));
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    (void)hipEventElapsedTime(&f.ms_facts, ev[0], ev[1]);
    info->ms_facts = f.ms_facts;
    if (h_small[0] != ~0ull) {
        const uint64_t ord = h_small[0] >> 3; const int kind = (int)(h_small[0] & 7u);
        info->bad_ordinal = (int64_t)ord; info->bad_kind = kind;
        set_error("%s: record %llu: %s", who, (unsigned long long)ord, bai_err_text(kind));
        return done(-1);
    }
    f.n_placed = h_small[1];
    return done(0);
}

int bai_build(lsg_ctx* c, const char* who, BaiFacts& f, const std::vector<uint64_t>& blk_ustart, const std::vector<uint64_t>& blk_coff, uint64_t v_eof, int table,
              DevBuf& tmp, lsg_bai_info* info) {
    hipStream_t st = c->stream;
    const uint64_t n = f.n;
    const uint32_t P = (uint32_t)f.n_placed, n_blk = (uint32_t)blk_ustart.size();
    const int32_t n_ref = f.n_ref;
    DevBuf d_bu, d_bc, d_vs, d_key, d_wkey, d_pm, d_pu, d_rid, d_rkey, d_rvb, d_rve, d_ridx, d_skey, d_sidx, d_cid, d_bid, d_bc0, d_refs, d_rsize, d_roff, d_wn, d_woff, d_lin, d_linf;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto done = [&](int rc) {
        for (DevBuf* b : {&d_bu, &d_bc, &d_vs, &d_key, &d_wkey, &d_pm, &d_pu, &d_rid, &d_rkey, &d_rvb, &d_rve, &d_ridx, &d_skey, &d_sidx, &d_cid, &d_bid, &d_bc0, &d_refs, &d_rsize, &d_roff,
                          &d_wn, &d_woff, &d_lin, &d_linf}) b->release();
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        if (rc != 0) { c->tab_text[table].release(); c->tab_bytes[table] = -1; }
        return rc;
    };
    c->tab_text[table].release(); c->tab_bytes[table] = -1;
    if (n && !n_blk) { set_error("%s: records without a BGZF block", who); return done(-1); }
    for (auto& e : ev) LSG_HIP_OR(hipEventCreate(&e), done(-1));
    info->n_records = (int64_t)n; info->n_placed = (int64_t)P; info->n_no_coor = (int64_t)(n - P);
    LSG_HIP_OR(hipEventRecord(ev[0], st), done(-1));
    // ---- 1. virtual offsets, keys, runs, the sort, chunks and bins
    uint32_t R = 0, n_chunks = 0, n_bins = 0;
    if (int rc = bai_reserve(d_vs, (n + 2) * 8, who, "the records' virtual offsets")) return done(rc);
    if (int rc = bai_reserve(d_pu, ((size_t)P + 2) * 4, who, "the unmapped records' counts")) return done(rc);
    if (n) {
        if (int rc = bai_reserve(d_bu, (size_t)n_blk * 8, who, "the block table")) return done(rc);
        if (int rc = bai_reserve(d_bc, (size_t)n_blk * 8, who, "the block table")) return done(rc);
        LSG_HIP_OR(hipMemcpyAsync(d_bu.p, blk_ustart.data(), (size_t)n_blk * 8, hipMemcpyHostToDevice, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(d_bc.p, blk_coff.data(), (size_t)n_blk * 8, hipMemcpyHostToDevice, st), done(-1));
        hipLaunchKernelGGL(k_bai_voff, dim3(bai_grid(n + 1)), dim3(256), 0, st, f.g.as<unsigned long long>(), n, d_bu.as<unsigned long long>(), d_bc.as<unsigned long long>(), n_blk,
                           (unsigned long long)v_eof, d_vs.as<unsigned long long>());
    }
    const unsigned long long* vs = d_vs.as<unsigned long long>();
    BaiIota iota(0);
    if (P) {
        if (int rc = bai_reserve(d_key, (size_t)P * 8, who, "the records' bins")) return done(rc);
        if (int rc = bai_reserve(d_wkey, (size_t)P * 8, who, "the records' windows")) return done(rc);
        if (int rc = bai_reserve(d_pm, (size_t)P * 8, who, "the records' windows")) return done(rc);
        if (int rc = bai_reserve(d_rid, ((size_t)P + 2) * 4, who, "the runs' numbers")) return done(rc);
        hipLaunchKernelGGL(k_bai_keys, dim3(bai_grid(P)), dim3(256), 0, st, f.tid.as<int32_t>(), f.pos.as<int32_t>(), f.end.as<int32_t>(), P, d_key.as<unsigned long long>(),
                           d_wkey.as<unsigned long long>());
        if (with_cub_tmp(tmp, "hipcub::DeviceScan::InclusiveScan", [&](void* p, size_t& b) {
                return hipcub::DeviceScan::InclusiveScan(p, b, d_wkey.as<unsigned long long>(), d_pm.as<unsigned long long>(), hipcub::Max(), (int)P, st); })) return done(-1);
        if (exclusive_sum(tmp, BaiIt<BaiUnmapped>(iota, BaiUnmapped{f.unm.as<uint8_t>(), P}), d_pu.as<uint32_t>(), (int64_t)P + 1, st)) return done(-1);
        const BaiRunHead run_head{d_key.as<unsigned long long>(), P};
        if (exclusive_sum(tmp, BaiIt<BaiRunHead>(iota, run_head), d_rid.as<uint32_t>(), (int64_t)P + 1, st)) return done(-1);
        LSG_HIP_OR(hipMemcpyAsync(&R, d_rid.as<uint32_t>() + P, 4, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipGetLastError(), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        if (R == 0 || R > P) { set_error("%s: %u runs of %u records", who, R, P); return done(-1); }
        for (DevBuf* b : {&d_rkey, &d_rvb, &d_rve, &d_skey}) if (int rc = bai_reserve(*b, (size_t)R * 8, who, "the runs")) return done(rc);
        for (DevBuf* b : {&d_ridx, &d_sidx}) if (int rc = bai_reserve(*b, (size_t)R * 4, who, "the runs")) return done(rc);
        for (DevBuf* b : {&d_cid, &d_bid, &d_bc0}) if (int rc = bai_reserve(*b, ((size_t)R + 2) * 4, who, "the chunks' numbers")) return done(rc);
        hipLaunchKernelGGL(k_bai_runs, dim3(bai_grid(P)), dim3(256), 0, st, run_head, d_rid.as<uint32_t>(), vs, d_rkey.as<unsigned long long>(), d_rvb.as<unsigned long long>(),
                           d_rve.as<unsigned long long>(), d_ridx.as<uint32_t>());
        if (with_cub_tmp(tmp, "hipcub::DeviceRadixSort::SortPairs", [&](void* p, size_t& b) {          // stable: a bin's runs stay in file order
                return hipcub::DeviceRadixSort::SortPairs(p, b, d_rkey.as<unsigned long long>(), d_skey.as<unsigned long long>(), d_ridx.as<uint32_t>(), d_sidx.as<uint32_t>(), (int)R, 0, 48, st); }))
            return done(-1);
        const BaiChunkHead chunk_head{d_skey.as<unsigned long long>(), d_sidx.as<uint32_t>(), d_rvb.as<unsigned long long>(), d_rve.as<unsigned long long>(), R};
        const BaiRunHead bin_head{d_skey.as<unsigned long long>(), R};
        if (exclusive_sum(tmp, BaiIt<BaiChunkHead>(iota, chunk_head), d_cid.as<uint32_t>(), (int64_t)R + 1, st)) return done(-1);
        if (exclusive_sum(tmp, BaiIt<BaiRunHead>(iota, bin_head), d_bid.as<uint32_t>(), (int64_t)R + 1, st)) return done(-1);
        hipLaunchKernelGGL(k_bai_binfirst, dim3(bai_grid((uint64_t)R + 1)), dim3(256), 0, st, bin_head, d_bid.as<uint32_t>(), d_cid.as<uint32_t>(), d_bc0.as<uint32_t>());
        LSG_HIP_OR(hipMemcpyAsync(&n_chunks, d_cid.as<uint32_t>() + R, 4, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(&n_bins, d_bid.as<uint32_t>() + R, 4, hipMemcpyDeviceToHost, st), done(-1));
    } else LSG_HIP_OR(hipMemsetAsync(d_pu.p, 0, 8, st), done(-1));
    LSG_HIP_OR(hipEventRecord(ev[1], st), done(-1));
    // ---- 2. per reference its pieces and bytes; the linear index
    unsigned long long body = 0, W = 0;
    if (int rc = bai_reserve(d_refs, ((size_t)n_ref + 1) * sizeof(BaiRef), who, "the references")) return done(rc);
    for (DevBuf* b : {&d_rsize, &d_roff, &d_wn, &d_woff}) if (int rc = bai_reserve(*b, ((size_t)n_ref + 2) * 8, who, "the references")) return done(rc);
    LSG_HIP_OR(hipMemsetAsync(d_rsize.p, 0, ((size_t)n_ref + 2) * 8, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_wn.p, 0, ((size_t)n_ref + 2) * 8, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_roff.p, 0, 16, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_woff.p, 0, 16, st), done(-1));
    if (n_ref) {
        hipLaunchKernelGGL(k_bai_refs, dim3(bai_grid((uint64_t)n_ref)), dim3(256), 0, st, f.tid.as<int32_t>(), P, d_skey.as<unsigned long long>(), R, d_bid.as<uint32_t>(), d_cid.as<uint32_t>(),
                           f.n_intv.as<uint32_t>(), n_ref, d_refs.as<BaiRef>(), d_rsize.as<unsigned long long>(), d_wn.as<unsigned long long>());
        if (exclusive_sum(tmp, d_rsize.as<unsigned long long>(), d_roff.as<unsigned long long>(), (int64_t)n_ref + 1, st)) return done(-1);
        if (exclusive_sum(tmp, d_wn.as<unsigned long long>(), d_woff.as<unsigned long long>(), (int64_t)n_ref + 1, st)) return done(-1);
        LSG_HIP_OR(hipMemcpyAsync(&body, d_roff.as<unsigned long long>() + n_ref, 8, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(&W, d_woff.as<unsigned long long>() + n_ref, 8, hipMemcpyDeviceToHost, st), done(-1));
    }
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    if (W >= 0x7fffffffull) { set_error("%s: an index of %llu windows is more than the device builder holds (2^31); make it on the host", who, W); return done(-3); }
    if (W) {
        if (int rc = bai_reserve(d_lin, (size_t)W * 8, who, "the linear index")) return done(rc);
        if (int rc = bai_reserve(d_linf, (size_t)W * 8, who, "the linear index")) return done(rc);
        hipLaunchKernelGGL(k_bai_lin, dim3(bai_grid(W)), dim3(256), 0, st, d_pm.as<unsigned long long>(), f.pos.as<int32_t>(), vs, d_refs.as<BaiRef>(), d_woff.as<unsigned long long>(), n_ref, W,
                           d_lin.as<unsigned long long>());
        if (with_cub_tmp(tmp, "hipcub::DeviceScan::InclusiveScan", [&](void* p, size_t& b) {          // an unset window takes the value before it
                return hipcub::DeviceScan::InclusiveScan(p, b, d_lin.as<unsigned long long>(), d_linf.as<unsigned long long>(), hipcub::Max(), (int)W, st); })) return done(-1);
    }
    LSG_HIP_OR(hipEventRecord(ev[2], st), done(-1));
    // ---- 3. the file's bytes
    const unsigned long long n_bytes = lsb::HEAD_BYTES + body + lsb::TAIL_BYTES;
    if (int rc = bai_reserve(c->tab_text[table], (size_t)n_bytes + 16, who, "the index file")) return done(rc);
    BaiPrint pa{};
    pa.out = c->tab_text[table].as<uint8_t>(); pa.refs = d_refs.as<BaiRef>(); pa.ref_off = d_roff.as<unsigned long long>(); pa.n_ref = n_ref;
    pa.key_s = d_skey.as<unsigned long long>(); pa.idx_s = d_sidx.as<uint32_t>(); pa.run_vb = d_rvb.as<unsigned long long>(); pa.run_ve = d_rve.as<unsigned long long>(); pa.n_runs = R;
    pa.bid = d_bid.as<uint32_t>(); pa.cid = d_cid.as<uint32_t>(); pa.bin_c0 = d_bc0.as<uint32_t>(); pa.vs = vs; pa.pu = d_pu.as<uint32_t>();
    pa.win_off = d_woff.as<unsigned long long>(); pa.lin = d_linf.as<unsigned long long>(); pa.n_win = W; pa.n_no_coor = n - P; pa.n_bytes = n_bytes;
    if (R) {
        const BaiChunkHead chunk_head{d_skey.as<unsigned long long>(), d_sidx.as<uint32_t>(), d_rvb.as<unsigned long long>(), d_rve.as<unsigned long long>(), R};
        const BaiRunHead bin_head{d_skey.as<unsigned long long>(), R};
        hipLaunchKernelGGL(k_bai_print_runs, dim3(bai_grid(R)), dim3(256), 0, st, pa, chunk_head, bin_head);
    }
    hipLaunchKernelGGL(k_bai_print_refs, dim3(bai_grid((uint64_t)n_ref + 1)), dim3(256), 0, st, pa);
    if (W) hipLaunchKernelGGL(k_bai_print_lin, dim3(bai_grid(W)), dim3(256), 0, st, pa);
    LSG_HIP_OR(hipEventRecord(ev[3], st), done(-1));
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    (void)hipEventElapsedTime(&info->ms_runs, ev[0], ev[1]); (void)hipEventElapsedTime(&info->ms_linear, ev[1], ev[2]); (void)hipEventElapsedTime(&info->ms_print, ev[2], ev[3]);
    info->n_runs = R; info->n_chunks = n_chunks; info->n_bins = n_bins; info->n_windows = (int64_t)W; info->n_bytes = (int64_t)n_bytes;
    c->tab_bytes[table] = (int64_t)n_bytes;
    return done(0);
}

} // namespace lsg

using namespace lsg;

extern "C" int lsg_bam_index(lsg_ctx* c, const uint8_t* file, int64_t n_bytes, int64_t first_record_offset, lsg_bai_info* info) {
    const char* who = "lsg_bam_index";
    if (!c || !file || n_bytes < 28 || !info || first_record_offset < 12) { set_error("lsg_bam_index: bad arguments"); return -2; }
    *info = lsg_bai_info{};
    info->bad_ordinal = -1;
    LSG_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const auto t_all = std::chrono::steady_clock::now();
    c->tab_text[LSG_TABLE_BAI].release(); c->tab_bytes[LSG_TABLE_BAI] = -1;
    IngestFront fr;
    BaiFacts facts;
    if (const int rc = ingest_front(c, who, file, n_bytes, first_record_offset, 0, fr)) return rc;
    info->ms_h2d = fr.ms_h2d; info->ms_inflate = fr.ms_inflate; info->ms_chain = fr.ms_chain;
    std::vector<int64_t> ref_len;
    {
        std::vector<uint8_t> head((size_t)first_record_offset);
        LSG_HIP(hipMemcpyAsync(head.data(), fr.d_u.p, head.size(), hipMemcpyDeviceToHost, st));
        LSG_HIP(hipStreamSynchronize(st));
        if (!parse_bam_refs(head, ref_len)) { set_error("lsg_bam_index: no BAM header that ends at first_record_offset %lld", (long long)first_record_offset); return -1; }
    }
    if (const int rc = bai_facts(c, who, fr.d_u.as<uint8_t>(), fr.utotal, fr.d_recoff.as<uint64_t>(), nullptr, fr.n_rec, (int32_t)ref_len.size(), nullptr, 0, fr.d_status.as<uint32_t>(), facts, info))
        return rc;
    const std::vector<uint64_t> blk_ustart = std::move(fr.blk_ustart), blk_coff = std::move(fr.blk_coff);      // ingest_front's walk of the block headers
    const uint64_t data_end = fr.data_end;
    DevBuf tmp;
    fr.release();                                               // the inflated stream is not read again
    const int rc = bai_build(c, who, facts, blk_ustart, blk_coff, data_end << 16, LSG_TABLE_BAI, tmp, info);
    tmp.release();
    info->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    return rc;
}

extern "C" int lsg_set_split_index(lsg_ctx* c, int on) {
    if (!c) { set_error("lsg_set_split_index: bad arguments"); return -2; }
    c->split_index = on != 0;
    return 0;
}

extern "C" int lsg_get_split_index_info(lsg_ctx* c, int t, lsg_bai_info* info) {
    if (!c || !info) { set_error("lsg_get_split_index_info: bad arguments"); return -2; }
    if (t < 0 || t >= c->split_bai_n) return -2;                // (the error text stays the failed lsg_split_bam's, which a caller asks for next)
    *info = c->split_bai[t];
    return 0;
}
