// SplitBamCellTypes on the device: a BAM's records routed to one BAM per cell type, BGZF-deflated where they lie (include/longsom_hip.h
// lsg_split_bam has the semantics), and the write half of BGZF for any bytes (lsg_bgzf_compress).
//
// Replaces split_bam (workflow/scripts/SplitBamCellTypes.py:39-192: pysam fetch -> read.opt("CB") -> the filters -> outfile.write, one
// record at a time, htslib's bgzf + zlib behind it on one thread); the host twin is lsio_split_bam_filtered (hostio/bamio.cpp).
//   ingest_front   H2D, k_inflate, k_block_crc, the record chain, k_rec_list: lsg_load_bam's front half (ingest_front.h)
//   k_sp_route     one thread per record (bamrec_core.h): placed on a reference, CB, the barcode table, reason_of, trim_window / trim_check
//                  -> the record's cell type or -1, its bytes, its trim window; the five counters and the 18 reasons with their first
//                  ordinals as k_rec_info tallies them; the smallest ordinal of a read the reference raises on
//   scans          per cell type an exclusive sum of its records' bytes behind the header's (hipcub)
//   the cut        the blocks of every stream as BgzfWriter cuts them (htslib's bgzf_flush_try rule): a walk on the host over the
//                  downloaded lengths and cell types (5 bytes a record down, one pass; the rule is sequential per stream)
//   k_sp_gather    one WAVE per record: its bytes into its cell type's stream, the body as aligned 16-byte stores, the trim window's
//                  qualities as 0
//   k_sp_deflate   one LANE per block (deflate_core.h): hash table in LDS [entry][lane], counts and codes in global memory
//                  [word][lane], the stream into the block's slot of fixed stride
//   k_sp_crc       one wave per block: CRC32 of the uncompressed bytes (crc_core.h, computed here where the ingest compares)
//   scan + k_sp_pack   the blocks' places in their file image; one wave per block writes header, payload, CRC32, ISIZE
// Every launch is sized by its work (a lane per block: ceil(n_blocks / 64) workgroups of 64; a wave per record or block: a quarter of
// a 256-thread workgroup each).
// Under lsg_set_split_index every cell type's .bai is made as well (bamindex.hip): the routed records' facts while the inflated input is
// resident, the index itself once the packed blocks' sizes say where every block lies in its file.
#include "lsg_ctx.h"
#include "ingest_front.h"
#include "bamrec_core.h"
#include "cbtable_host.h"
#include "crc_core.h"
#include "deflate_core.h"
#include "cub_tmp.h"
#include "bamindex.h"
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace lsg {

constexpr uint32_t SP_BLOCK = lsd::MAX_IN;                      // 0xff00: what BgzfWriter (and htslib) put into one block
constexpr uint32_t SP_SLOT = (SP_BLOCK + 5u + 15u) & ~15u;      // a block's compressed bytes: at most stored, n + 5
enum { SP_ERR_TRIM_LONG = 1, SP_ERR_NO_QUAL = 2, SP_ERR_NM_TYPE = 3, SP_ERR_NH_TYPE = 4 };      // lsio_split_bam_filtered's SPLIT_ERR_*
static const char* sp_err_text(int kind) {                     // ... and its texts
    switch (kind) {
        case SP_ERR_TRIM_LONG: return "its --n_trim window is longer than the read (the reference raises IndexError)";
        case SP_ERR_NO_QUAL: return "it has no base qualities to trim (the reference raises TypeError)";
        case SP_ERR_NM_TYPE: return "its nM tag is not a number (the reference raises TypeError)";
        case SP_ERR_NH_TYPE: return "its NH tag is not a number (the reference raises TypeError)";
        default: return "?";
    }
}

struct SpRouteArgs {
    const uint8_t* u; uint64_t total; const uint64_t* rec_off; uint64_t n_rec;
    int32_t n_ref; const int64_t* ref_len;
    lsr::CbTable cbt; int32_t min_mapq, max_nm, max_nh, n_trim;
    uint32_t* len; int8_t* ct; uint2* trim;
    unsigned long long* counters;         // [5] total, pass, cb_not_found, cb_not_matched, mapq
    unsigned long long* rsn_n;            // [N_REASONS]
    unsigned long long* rsn_first;        // [N_REASONS] (~0: none)
    unsigned long long* n_written;        // [LSG_MAX_CELLTYPES]
    unsigned long long* err;              // smallest (ordinal << 3 | kind) of a read the reference raises on (~0: none)
    uint32_t* status;                     // ingest_front's words: bit 2 a record past the stream's end, bit 8 + word 2 lsr::validate's reason
};
__global__ __launch_bounds__(256) void k_sp_route(SpRouteArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t ct = -1;
    uint32_t reason = lsr::N_REASONS;
    bool total = false, nf = false, nm_ = false;
    if (i < a.n_rec) {
        const uint64_t p = a.rec_off[i];
        const uint32_t bs = lsr::rd32(a.u + p);
        const uint8_t* rec = a.u + p + 4;
        lsr::Trim tw{0, 0};
        if (p + 4ull + bs > a.total) atomicOr(a.status, 2u);
        else {
            const int v = lsr::validate(rec, bs, a.n_ref, a.ref_len);
            if (v != lsr::REC_OK) { atomicOr(a.status, 8u); atomicMin(a.status + 2, (uint32_t)v); }
            else if ((int32_t)lsr::rd32(rec) >= 0) {                       // infile.fetch() iterates the reads placed on a reference
                total = true;
                uint32_t cb = 0, raw = 0, clean = 0;
                lsr::AuxNum nm, nh;
                int32_t id;
                if (!lsr::scan_aux(rec, bs, &cb, &raw, &clean, &nm, &nh, true)) nf = true;      // the host splitter's find_cb: the first CB:Z
                else if ((id = lsr::cb_lookup(a.cbt, rec + cb, clean)) < 0) nm_ = true;
                else {
                    int err = 0;                                            // split_reason's order (bamio.cpp): nM type, NH type, then the trim
                    if (a.max_nm >= 0 && nm.kind == lsr::AUX_BAD) err = SP_ERR_NM_TYPE;
                    else if (a.max_nh >= 0 && nh.kind == lsr::AUX_BAD) err = SP_ERR_NH_TYPE;
                    reason = lsr::reason_of(nm, nh, a.max_nm, a.max_nh, (int)rec[9] < a.min_mapq);
                    if (reason == 0) {
                        ct = id;
                        if (a.n_trim > 0) {
                            tw = lsr::trim_window(rec, (uint32_t)a.n_trim);
                            const int tc = lsr::trim_check(rec, tw);
                            if (tc != lsr::TRIM_OK && !err) err = tc == lsr::TRIM_TOO_LONG ? SP_ERR_TRIM_LONG : SP_ERR_NO_QUAL;
                        }
                    }
                    if (err) { atomicMin(a.err, (unsigned long long)((i << 3) | (uint64_t)err)); ct = -1; }
                }
            }
        }
        a.len[i] = ct >= 0 ? 4u + bs : 0u; a.ct[i] = (int8_t)ct; a.trim[i] = make_uint2(tw.start, tw.end);
    }
    const bool lead = (threadIdx.x & 63) == 0;
    {   // SplitBam's counters (SplitBamCellTypes.py:62,117-124): a ballot per wave and counter
        const unsigned long long m_t = __ballot(total), m_p = __ballot(reason == 0), m_f = __ballot(nf), m_m = __ballot(nm_), m_q = __ballot(reason == 1);
        if (lead) {
            if (m_t) atomicAdd(&a.counters[0], (unsigned long long)__popcll(m_t));
            if (m_p) atomicAdd(&a.counters[1], (unsigned long long)__popcll(m_p));
            if (m_f) atomicAdd(&a.counters[2], (unsigned long long)__popcll(m_f));
            if (m_m) atomicAdd(&a.counters[3], (unsigned long long)__popcll(m_m));
            if (m_q) atomicAdd(&a.counters[4], (unsigned long long)__popcll(m_q));
        }
    }
    const uint64_t wave0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u);
    for (uint32_t r = 0; r < lsr::N_REASONS; ++r) {             // the reasons and their first ordinals, as k_rec_info tallies them
        const unsigned long long m = __ballot(reason == r);
        if (m && lead) {
            atomicAdd(&a.rsn_n[r], (unsigned long long)__popcll(m));
            atomicMin(&a.rsn_first[r], (unsigned long long)(wave0 + (uint64_t)(__ffsll((long long)m) - 1)));
        }
    }
    for (int t = 0; t < LSG_MAX_CELLTYPES; ++t) {
        const unsigned long long m = __ballot(ct == t);
        if (m && lead) atomicAdd(&a.n_written[t], (unsigned long long)__popcll(m));
    }
}

struct SpLenOf { const uint32_t* len; const int8_t* ct; int32_t t; __host__ __device__ unsigned long long operator()(const uint32_t& i) const { return ct[i] == t ? (unsigned long long)len[i] : 0ull; } };
struct SpIsOf { const int8_t* ct; int32_t t; uint64_t n; __host__ __device__ uint32_t operator()(const uint32_t& i) const { return i < n && ct[i] == t ? 1u : 0u; } };
// the ordinals of cell type t's records, in file order (rank: the exclusive count of its records)
__global__ void k_sp_select(const int8_t* ct, int32_t t, const uint32_t* rank, uint64_t n_rec, uint32_t* sel) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && ct[i] == t) sel[rank[i]] = (uint32_t)i;
}
__global__ void k_sp_place(const int8_t* ct, int32_t t, const unsigned long long* off_t, unsigned long long base, uint64_t n_rec, unsigned long long* off) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && ct[i] == t) off[i] = base + off_t[i];
}

// n bytes of s to d by one wave: the unaligned head (< 16 bytes) and the tail as byte stores, the body as aligned 16-byte stores
template <class Src> __device__ __forceinline__ void put_bytes(uint8_t* d, uint32_t n, uint32_t lane, const Src& s) {
    const uint32_t mis = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u, head = mis < n ? mis : n;
    if (lane < head) d[lane] = s.byte(lane);
    const uint32_t n_body = (n - head) >> 4;
    for (uint32_t k = lane; k < n_body; k += 64u) *reinterpret_cast<uint4*>(d + head + 16u * k) = s.chunk16(head + 16u * k);
    const uint32_t j = head + 16u * n_body + lane;
    if (j < n) d[j] = s.byte(j);
}
struct PlainSrc {
    const uint8_t* p;
    __device__ __forceinline__ uint8_t byte(uint32_t j) const { return p[j]; }
    __device__ __forceinline__ uint4 chunk16(uint32_t j) const { uint4 v; __builtin_memcpy(&v, p + j, 16); return v; }
};
// a record whose bytes [a0, a1) and [b0, b1) - the trim window's qualities - read as 0 (read.query_qualities = Q, SplitBamCellTypes.py:161-170)
struct TrimSrc {
    const uint8_t* p; uint32_t a0, a1, b0, b1;
    __device__ __forceinline__ bool zero(uint32_t j) const { return (j >= a0 && j < a1) || (j >= b0 && j < b1); }
    __device__ __forceinline__ uint8_t byte(uint32_t j) const { return zero(j) ? (uint8_t)0 : p[j]; }
    __device__ __forceinline__ uint4 chunk16(uint32_t j) const {
        uint32_t x[4];
        __builtin_memcpy(x, p + j, 16);
        if ((j < a1 && j + 16u > a0) || (j < b1 && j + 16u > b0))
            for (uint32_t k = 0; k < 16u; ++k) if (zero(j + k)) x[k >> 2] &= ~(0xffu << (8u * (k & 3u)));
        return make_uint4(x[0], x[1], x[2], x[3]);
    }
};

struct SpGatherArgs { const uint8_t* u; const uint64_t* rec_off; uint64_t n_rec; const uint32_t* len; const int8_t* ct; const uint2* trim; const unsigned long long* off; uint8_t* streams; };
__global__ __launch_bounds__(256) void k_sp_gather(SpGatherArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (i >= a.n_rec || a.ct[i] < 0) return;
    const uint8_t* src = a.u + a.rec_off[i];
    uint8_t* d = a.streams + a.off[i];
    const uint32_t n = a.len[i];
    const uint2 tw = a.trim[i];
    if (tw.x | tw.y) {
        const uint8_t* rec = src + 4;
        const uint32_t l_seq = lsr::rd32(rec + 16);
        const uint32_t q = 4u + 32u + rec[8] + 4u * lsr::rd16(rec + 12) + (l_seq + 1u) / 2u;          // the qualities (trim_check: both ends <= l_seq)
        put_bytes(d, n, lane, TrimSrc{src, q, q + tw.x, q + l_seq - tw.y, q + l_seq});
    } else put_bytes(d, n, lane, PlainSrc{src});
}

// ---- BGZF's write half over streams that lie on the device -------------------------------------------------------------------------
struct SpBlk { uint64_t off; uint32_t n; uint32_t stream; };          // a block: where its bytes lie in the streams' buffer, how many, whose

template <int HB>
__global__ __launch_bounds__(64) void k_sp_deflate(const uint8_t* streams, const SpBlk* blk, uint32_t n_blk, uint8_t* slots, uint32_t* csize, uint16_t* work) {
    __shared__ uint16_t hash[(1u << HB) * 64u];                         // [entry][lane]
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= n_blk) return;
    const lsd::Work w{hash + threadIdx.x, 64, work + (size_t)blockIdx.x * lsd::W_WORDS * 64u + threadIdx.x, 64};
    const SpBlk d = blk[b];
    csize[b] = lsd::deflate_block<HB>(streams + d.off, d.n, slots + (size_t)b * SP_SLOT, d.n + 5u, w);
}

// one wave per block, the arithmetic of ingest.hip's k_block_crc; the CRC is kept
__global__ __launch_bounds__(256) void k_sp_crc(const uint8_t* streams, const SpBlk* blk, uint32_t n_blk, const lsc::CrcTables* tabs, uint32_t* crc_out) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t ops[17][32];
    for (int i = threadIdx.x; i < 256; i += 256) tab[i] = tabs->byte_tab[i];
    for (int i = threadIdx.x; i < 17 * 32; i += 256) (&ops[0][0])[i] = (&tabs->zero_ops[0][0])[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= n_blk) return;
    const SpBlk d = blk[b];
    const uint32_t lo = lane * lsc::CHUNK, hi = lo + lsc::CHUNK < d.n ? lo + lsc::CHUNK : d.n;
    uint32_t c = 0;
    if (lo < d.n) c = lsc::crc_shift(ops, lsc::crc_chunk(tab, streams + d.off, d.off, lo, hi), d.n - hi);
    for (int o = 32; o > 0; o >>= 1) c ^= (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0) crc_out[b] = c ^ lsc::crc_shift(ops, 0xffffffffu, d.n) ^ 0xffffffffu;
}

struct SpSizeOf { const uint32_t* csize; __host__ __device__ unsigned long long operator()(const uint32_t& b) const { return (unsigned long long)csize[b] + 26ull; } };
struct SpPackArgs {
    const SpBlk* blk; uint32_t n_blk; const uint8_t* slots; const uint32_t* csize; const uint32_t* crc; const unsigned long long* pos;
    uint8_t* image[LSG_MAX_CELLTYPES]; unsigned long long pos0[LSG_MAX_CELLTYPES];      // per stream: its file image, the place of its first block in `pos`
};
__global__ __launch_bounds__(256) void k_sp_pack(SpPackArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= a.n_blk) return;
    const SpBlk d = a.blk[b];
    const uint32_t cs = a.csize[b];
    uint8_t* o = a.image[d.stream] + (a.pos[b] - a.pos0[d.stream]);
    if (lane < 18u) {
        const uint8_t hdr[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
        const uint32_t bsize1 = cs + 25u;                                 // BSIZE - 1
        o[lane] = lane < 16u ? hdr[lane] : (uint8_t)(bsize1 >> (8u * (lane - 16u)));
    }
    put_bytes(o + 18, cs, lane, PlainSrc{a.slots + (size_t)b * SP_SLOT});
    if (lane < 8u) o[18u + cs + lane] = (uint8_t)((lane < 4u ? a.crc[b] : d.n) >> (8u * (lane & 3u)));
}

// the match finder's table: 128 entries, 16 KiB of LDS a wave.  Measured beside 256 and 512 entries: the smallest table is
// the fastest (5.2 / 3.4 / 2.7 GB/s) and its files are 1.4 % / 6 % larger
constexpr int SP_HASH_BITS = 7;

// the library's out-of-memory code: -3 (what ingest_front returns when its tables find no room)
static int sp_reserve(DevBuf& b, size_t bytes, const char* who, const char* what) {
    if (b.reserve(bytes) == 0) return 0;
    (void)hipGetLastError();
    set_error("%s: no device memory for %s (%zu bytes)", who, what, bytes);
    return -3;
}

struct SpTimes { float deflate = 0, crc = 0, pack = 0; };
// The streams' blocks -> one file image per stream in the tables `table0 + s`: deflate, CRC32, scan, pack, the EOF block.  `blocks` is
// sorted by stream.  `streams` is released once the blocks are compressed.  file_bytes[s]: the image's size.
// csize_out: every block's compressed bytes (its place in its file follows from them: 26 bytes of framing a block).
static int sp_compress(lsg_ctx* c, const char* who, DevBuf& streams, const std::vector<SpBlk>& blocks, int n_streams, int table0, int64_t* file_bytes, SpTimes* times,
                       std::vector<uint32_t>* csize_out = nullptr) {
    hipStream_t st = c->stream;
    const uint32_t n_blk = (uint32_t)blocks.size();
    static const uint8_t eof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf d_blk, d_slots, d_csize, d_crc, d_pos, d_work, d_tabs, d_tmp;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto done = [&](int rc) {
        for (DevBuf* b : {&d_blk, &d_slots, &d_csize, &d_crc, &d_pos, &d_work, &d_tabs, &d_tmp}) b->release();
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        return rc;
    };
    for (auto& e : ev) LSG_HIP_OR(hipEventCreate(&e), done(-1));
    std::vector<unsigned long long> h_pos((size_t)n_streams + 1, 0);       // per stream: the place of its first block in the scan
    std::vector<uint32_t> first((size_t)n_streams + 1, n_blk);
    for (uint32_t b = n_blk; b-- > 0;) first[blocks[b].stream] = b;
    for (int s = n_streams - 1; s >= 0; --s) if (first[(size_t)s] == n_blk) first[(size_t)s] = first[(size_t)s + 1];      // a stream without blocks
    if (n_blk) {
        const uint32_t g = (n_blk + 63u) / 64u;
        if (int rc = sp_reserve(d_blk, (size_t)n_blk * sizeof(SpBlk), who, "the block list")) return done(rc);
        if (int rc = sp_reserve(d_csize, ((size_t)n_blk + 1) * 4, who, "the block sizes")) return done(rc);
        if (int rc = sp_reserve(d_crc, ((size_t)n_blk + 1) * 4, who, "the block CRCs")) return done(rc);
        if (int rc = sp_reserve(d_pos, ((size_t)n_blk + 2) * 8, who, "the block places")) return done(rc);
        if (int rc = sp_reserve(d_work, (size_t)g * lsd::W_WORDS * 64 * 2, who, "the encoder's tables")) return done(rc);
        if (int rc = sp_reserve(d_slots, (size_t)n_blk * SP_SLOT, who, "the compressed blocks")) return done(rc);
        if (int rc = sp_reserve(d_tabs, sizeof(lsc::CrcTables), who, "the CRC tables")) return done(rc);
        static const lsc::CrcTables h_tabs = [] { lsc::CrcTables t; lsc::make_crc_tables(t); return t; }();      // (made once, by one thread: a local static's rule)
        LSG_HIP_OR(hipMemcpyAsync(d_tabs.p, &h_tabs, sizeof(lsc::CrcTables), hipMemcpyHostToDevice, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(d_blk.p, blocks.data(), (size_t)n_blk * sizeof(SpBlk), hipMemcpyHostToDevice, st), done(-1));
        LSG_HIP_OR(hipMemsetAsync(d_csize.as<uint32_t>() + n_blk, 0, 4, st), done(-1));
        LSG_HIP_OR(hipEventRecord(ev[0], st), done(-1));
        const uint8_t* s8 = streams.as<uint8_t>();
        hipLaunchKernelGGL(k_sp_deflate<SP_HASH_BITS>, dim3(g), dim3(64), 0, st, s8, d_blk.as<SpBlk>(), n_blk, d_slots.as<uint8_t>(), d_csize.as<uint32_t>(), d_work.as<uint16_t>());
        LSG_HIP_OR(hipEventRecord(ev[1], st), done(-1));
        hipLaunchKernelGGL(k_sp_crc, dim3((n_blk + 3u) / 4u), dim3(256), 0, st, s8, d_blk.as<SpBlk>(), n_blk, d_tabs.as<lsc::CrcTables>(), d_crc.as<uint32_t>());
        LSG_HIP_OR(hipEventRecord(ev[2], st), done(-1));
        hipcub::CountingInputIterator<uint32_t> iota(0);
        hipcub::TransformInputIterator<unsigned long long, SpSizeOf, hipcub::CountingInputIterator<uint32_t>> it(iota, SpSizeOf{d_csize.as<uint32_t>()});
        if (exclusive_sum(d_tmp, it, d_pos.as<unsigned long long>(), (int64_t)n_blk + 1, st)) return done(-1);
        for (int s = 0; s <= n_streams; ++s)
            LSG_HIP_OR(hipMemcpyAsync(&h_pos[(size_t)s], d_pos.as<unsigned long long>() + first[(size_t)s], 8, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipGetLastError(), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        std::vector<uint32_t> h_cs(n_blk);
        LSG_HIP_OR(hipMemcpy(h_cs.data(), d_csize.p, (size_t)n_blk * 4, hipMemcpyDeviceToHost), done(-1));
        for (uint32_t b = 0; b < n_blk; ++b)
            if (h_cs[b] == 0 || h_cs[b] > blocks[b].n + 5u) { set_error("%s: block %u of %u bytes was not compressed (%u)", who, b, blocks[b].n, h_cs[b]); return done(-1); }
        if (csize_out) *csize_out = h_cs;
    }
    streams.release();
    SpPackArgs pa{};
    pa.blk = d_blk.as<SpBlk>(); pa.n_blk = n_blk; pa.slots = d_slots.as<uint8_t>(); pa.csize = d_csize.as<uint32_t>(); pa.crc = d_crc.as<uint32_t>(); pa.pos = d_pos.as<unsigned long long>();
    for (int s = 0; s < n_streams; ++s) {
        const int64_t bytes = (int64_t)(h_pos[(size_t)s + 1] - h_pos[(size_t)s]) + 28;
        if (int rc = sp_reserve(c->tab_text[table0 + s], (size_t)bytes + 16, who, "a file image")) return done(rc);
        pa.image[s] = c->tab_text[table0 + s].as<uint8_t>(); pa.pos0[s] = h_pos[(size_t)s];
        LSG_HIP_OR(hipMemcpyAsync(pa.image[s] + bytes - 28, eof, 28, hipMemcpyHostToDevice, st), done(-1));
        file_bytes[s] = bytes;
    }
    if (n_blk) {
        hipLaunchKernelGGL(k_sp_pack, dim3((n_blk + 3u) / 4u), dim3(256), 0, st, pa);
        LSG_HIP_OR(hipEventRecord(ev[3], st), done(-1));
    }
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    if (n_blk && times) { (void)hipEventElapsedTime(&times->deflate, ev[0], ev[1]); (void)hipEventElapsedTime(&times->crc, ev[1], ev[2]); (void)hipEventElapsedTime(&times->pack, ev[2], ev[3]); }
    for (int s = 0; s < n_streams; ++s) c->tab_bytes[table0 + s] = file_bytes[s];
    return done(0);
}

// BgzfWriter's cuts (bamio.cpp): write() fills the open block to 0xff00 and spills; write_record() closes an open block the record does not fit
struct SpCutter {
    std::vector<SpBlk>* out; uint64_t base; uint32_t stream; uint64_t start = 0; uint32_t open = 0;
    void close() { out->push_back(SpBlk{base + start, open, stream}); start += open; open = 0; }
    void write(uint64_t n) { while (n) { const uint64_t room = SP_BLOCK - open, take = n < room ? n : room; open += (uint32_t)take; n -= take; if (open >= SP_BLOCK) close(); } }
    void write_record(uint64_t n) { if (open && open + n > SP_BLOCK) close(); write(n); }
    void finish() { if (open) close(); }
};

} // namespace lsg

using namespace lsg;

extern "C" int lsg_bgzf_compress(lsg_ctx* c, const uint8_t* data, int64_t n, int64_t* n_bytes_out) {
    if (n_bytes_out) *n_bytes_out = 0;
    if (!c || n < 0 || (n > 0 && !data)) { set_error("lsg_bgzf_compress: bad arguments"); return -2; }
    if (((uint64_t)n + SP_BLOCK - 1) / SP_BLOCK >= 0x7fffffffull) { set_error("lsg_bgzf_compress: %lld bytes are more than 2^31 blocks", (long long)n); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    c->tab_text[LSG_TABLE_BGZF].release(); c->tab_bytes[LSG_TABLE_BGZF] = -1;
    DevBuf streams;
    if (int rc = sp_reserve(streams, (size_t)n + 64, "lsg_bgzf_compress", "the bytes")) return rc;
    if (n) LSG_HIP_OR(hipMemcpyAsync(streams.p, data, (size_t)n, hipMemcpyHostToDevice, c->stream), (streams.release(), -1));
    std::vector<SpBlk> blocks;
    SpCutter cut{&blocks, 0, 0};
    cut.write((uint64_t)n); cut.finish();
    int64_t bytes = 0;
    const int rc = sp_compress(c, "lsg_bgzf_compress", streams, blocks, 1, LSG_TABLE_BGZF, &bytes, nullptr);
    streams.release();
    if (rc != 0) { c->tab_text[LSG_TABLE_BGZF].release(); c->tab_bytes[LSG_TABLE_BGZF] = -1; }      // (it may have failed behind the image's reserve)
    if (rc == 0 && n_bytes_out) *n_bytes_out = bytes;
    return rc;
}

extern "C" int lsg_split_bam(lsg_ctx* c, const uint8_t* file, int64_t n_bytes, int64_t first_record_offset, const char* barcodes, int32_t n_barcodes,
                             const int32_t* celltype_of, int32_t n_celltypes, int32_t min_mapq, lsg_split_info* info) {
    const char* who = "lsg_split_bam";
    if (!c || !file || n_bytes < 28 || !info || first_record_offset < 12 || !barcodes || n_barcodes <= 0 || !celltype_of) { set_error("lsg_split_bam: bad arguments"); return -2; }
    if (n_celltypes <= 0 || n_celltypes > LSG_MAX_CELLTYPES) { set_error("lsg_split_bam: 1..%d cell types", LSG_MAX_CELLTYPES); return -2; }
    for (int32_t i = 0; i < n_barcodes; ++i)
        if (celltype_of[i] < 0 || celltype_of[i] >= n_celltypes) { set_error("lsg_split_bam: barcode %d has cell type %d of %d", i, celltype_of[i], n_celltypes); return -2; }
    *info = lsg_split_info{};
    info->bad_ordinal = -1;
    for (auto& f : info->reasons_first) f = -1;
    LSG_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const auto t_all = std::chrono::steady_clock::now();
    auto drop_tables = [&] {
        for (int t = 0; t < LSG_MAX_CELLTYPES; ++t)
            for (int tab : {LSG_TABLE_SPLIT_BAM + t, LSG_TABLE_SPLIT_BAI + t}) { c->tab_text[tab].release(); c->tab_bytes[tab] = -1; }
    };
    drop_tables();                                                 // whatever fails below: no table is kept, and none of an earlier call's
    c->split_bai_n = 0;
    const bool with_index = c->split_index;
    lsr::CbTableHost cbt;
    cbt.build(barcodes, n_barcodes, celltype_of);                  // the table's "id" of a barcode is its cell type
    IngestFront fr;
    DevBuf d_h, d_id, d_so, d_sl, d_str, d_reflen, d_len, d_ct, d_trim, d_offt, d_off, d_small, d_streams, d_sel, d_bai_tmp;
    BaiFacts bai_f[LSG_MAX_CELLTYPES];                             // lsg_set_split_index: what the indexes need of the records, kept across the compression
    lsg_bai_info bai_i[LSG_MAX_CELLTYPES] = {};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto done = [&](int rc) {
        for (DevBuf* b : {&d_h, &d_id, &d_so, &d_sl, &d_str, &d_reflen, &d_len, &d_ct, &d_trim, &d_offt, &d_off, &d_small, &d_streams, &d_sel, &d_bai_tmp}) b->release();
        for (auto& f : bai_f) f.release();
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        fr.release();
        return rc;
    };
    for (auto& e : ev) LSG_HIP_OR(hipEventCreate(&e), done(-1));
    if (sp_reserve(d_h, cbt.hash.size() * 8, who, "the barcode table") || sp_reserve(d_id, cbt.id.size() * 4, who, "the barcode table") || sp_reserve(d_so, cbt.str_off.size() * 4, who, "the barcode table") ||
        sp_reserve(d_sl, cbt.str_len.size() * 4, who, "the barcode table") || sp_reserve(d_str, cbt.strs.size() + 16, who, "the barcode table"))
        return done(-3);
    LSG_HIP_OR(hipMemcpyAsync(d_h.p, cbt.hash.data(), cbt.hash.size() * 8, hipMemcpyHostToDevice, st), done(-1));
    LSG_HIP_OR(hipMemcpyAsync(d_id.p, cbt.id.data(), cbt.id.size() * 4, hipMemcpyHostToDevice, st), done(-1));
    LSG_HIP_OR(hipMemcpyAsync(d_so.p, cbt.str_off.data(), cbt.str_off.size() * 4, hipMemcpyHostToDevice, st), done(-1));
    LSG_HIP_OR(hipMemcpyAsync(d_sl.p, cbt.str_len.data(), cbt.str_len.size() * 4, hipMemcpyHostToDevice, st), done(-1));
    LSG_HIP_OR(hipMemcpyAsync(d_str.p, cbt.strs.data(), cbt.strs.size(), hipMemcpyHostToDevice, st), done(-1));
    // ---- 1. the front: H2D, inflate, CRC, the record chain, every record's offset (-4: the chain did not settle)
    if (const int rc = ingest_front(c, who, file, n_bytes, first_record_offset, 0, fr)) return done(rc);
    const uint64_t n_rec = fr.n_rec, utotal = fr.utotal, H = (uint64_t)first_record_offset;
    const uint8_t* u = fr.d_u.as<uint8_t>();
    uint32_t* status = fr.d_status.as<uint32_t>();
    info->n_records = (int64_t)n_rec; info->ms_h2d = fr.ms_h2d; info->ms_inflate = fr.ms_inflate; info->ms_chain = fr.ms_chain;
    std::vector<int64_t> ref_len;
    {
        std::vector<uint8_t> head((size_t)H);
        LSG_HIP_OR(hipMemcpyAsync(head.data(), u, head.size(), hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        if (!parse_bam_refs(head, ref_len)) { set_error("lsg_split_bam: no BAM header that ends at first_record_offset %lld", (long long)first_record_offset); return done(-1); }
    }
    constexpr int N_SMALL = 1 + 5 + 2 * lsr::N_REASONS + LSG_MAX_CELLTYPES;      // err, counters, reasons, first ordinals, records per cell type
    if (sp_reserve(d_reflen, (ref_len.size() + 1) * 8, who, "the reference lengths") || sp_reserve(d_small, N_SMALL * 8, who, "the counters")) return done(-3);
    if (int rc = sp_reserve(d_len, (n_rec + 2) * 4, who, "the records' lengths")) return done(rc);
    if (int rc = sp_reserve(d_ct, n_rec + 16, who, "the records' cell types")) return done(rc);
    if (int rc = sp_reserve(d_trim, (n_rec + 1) * 8, who, "the records' trim windows")) return done(rc);
    if (int rc = sp_reserve(d_offt, (n_rec + 2) * 8, who, "the records' offsets")) return done(rc);
    if (int rc = sp_reserve(d_off, (n_rec + 2) * 8, who, "the records' offsets")) return done(rc);
    if (!ref_len.empty()) LSG_HIP_OR(hipMemcpyAsync(d_reflen.p, ref_len.data(), ref_len.size() * 8, hipMemcpyHostToDevice, st), done(-1));
    unsigned long long* d_err = d_small.as<unsigned long long>();
    unsigned long long* d_cnt = d_err + 1; unsigned long long* d_rn = d_cnt + 5; unsigned long long* d_rf = d_rn + lsr::N_REASONS; unsigned long long* d_nw = d_rf + lsr::N_REASONS;
    LSG_HIP_OR(hipMemsetAsync(d_small.p, 0, N_SMALL * 8, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_err, 0xff, 8, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_rf, 0xff, lsr::N_REASONS * 8, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(status, 0, 4, st), done(-1));
    LSG_HIP_OR(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(status + 2), (int)0x7fffffff, 1, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_len.as<uint32_t>() + n_rec, 0, 4, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_ct.as<int8_t>() + n_rec, 0xff, 1, st), done(-1));
    // ---- 2. route
    LSG_HIP_OR(hipEventRecord(ev[0], st), done(-1));
    unsigned long long h_small[N_SMALL];
    h_small[0] = ~0ull; for (int i = 1; i < N_SMALL; ++i) h_small[i] = 0;
    for (int r = 0; r < lsr::N_REASONS; ++r) h_small[1 + 5 + lsr::N_REASONS + r] = ~0ull;
    if (n_rec) {
        SpRouteArgs a{};
        a.u = u; a.total = utotal; a.rec_off = fr.d_recoff.as<uint64_t>(); a.n_rec = n_rec; a.n_ref = (int32_t)ref_len.size(); a.ref_len = d_reflen.as<int64_t>();
        a.cbt = lsr::CbTable{d_h.as<uint64_t>(), d_id.as<int32_t>(), d_so.as<uint32_t>(), d_sl.as<uint32_t>(), d_str.as<uint8_t>(), cbt.mask};
        a.min_mapq = min_mapq; a.max_nm = c->split_max_nm; a.max_nh = c->split_max_nh; a.n_trim = c->split_n_trim;
        a.len = d_len.as<uint32_t>(); a.ct = d_ct.as<int8_t>(); a.trim = d_trim.as<uint2>();
        a.counters = d_cnt; a.rsn_n = d_rn; a.rsn_first = d_rf; a.n_written = d_nw; a.err = d_err; a.status = status;
        hipLaunchKernelGGL(k_sp_route, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, a);
        uint32_t hstat[4] = {0, 0, 0, 0};
        LSG_HIP_OR(hipMemcpyAsync(hstat, status, 16, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(h_small, d_small.p, sizeof(h_small), hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        if (hstat[0]) {
            static const char* why[] = {"", "a record shorter than its fixed fields", "a record whose fields exceed its block_size", "a record on a reference the header does not list",
                                        "a CIGAR operation above 8", "a CIGAR that does not cover the stored sequence", "an alignment that leaves its reference"};
            set_error("lsg_split_bam: %s", (hstat[0] & 8u) && hstat[2] < 7 ? why[hstat[2]] : "truncated record at the end of the file");
            return done(-1);
        }
    }
    for (int k = 0; k < 5; ++k) info->counters[k] = (int64_t)h_small[1 + k];
    for (int r = 0; r < lsr::N_REASONS; ++r) {
        info->reasons_n[r] = (int64_t)h_small[1 + 5 + r];
        info->reasons_first[r] = h_small[1 + 5 + lsr::N_REASONS + r] == ~0ull ? -1 : (int64_t)h_small[1 + 5 + lsr::N_REASONS + r];
    }
    if (h_small[0] != ~0ull) {                                      // a read on which the reference raises: the host twin's message, no table
        const uint64_t ord = h_small[0] >> 3; const int kind = (int)(h_small[0] & 7u);
        uint64_t roff = 0; uint8_t head[32 + 256];
        LSG_HIP_OR(hipMemcpyAsync(&roff, fr.d_recoff.as<uint64_t>() + ord, 8, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        const size_t n_head = (size_t)(utotal - (roff + 4)) < sizeof(head) ? (size_t)(utotal - (roff + 4)) : sizeof(head);
        LSG_HIP_OR(hipMemcpyAsync(head, u + roff + 4, n_head, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        const uint32_t l_name = head[8];
        const std::string name((const char*)head + 32, l_name ? strnlen((const char*)head + 32, l_name - 1u) : 0u);
        info->bad_ordinal = (int64_t)ord; info->bad_kind = kind;
        set_error("lsg_split_bam: read '%s' (record %llu): %s", name.c_str(), (unsigned long long)ord, sp_err_text(kind));
        return done(-1);
    }
    // ---- 3. place: every record's offset in its cell type's stream, the streams one after the other in one buffer
    uint64_t base[LSG_MAX_CELLTYPES + 1] = {0, 0, 0, 0, 0};
    hipcub::CountingInputIterator<uint32_t> iota(0);
    for (int32_t t = 0; t < n_celltypes; ++t) {
        unsigned long long bytes_t = 0;
        if (n_rec) {
            hipcub::TransformInputIterator<unsigned long long, SpLenOf, hipcub::CountingInputIterator<uint32_t>> it(iota, SpLenOf{d_len.as<uint32_t>(), d_ct.as<int8_t>(), t});
            if (exclusive_sum(fr.d_tmp, it, d_offt.as<unsigned long long>(), (int64_t)n_rec + 1, st)) return done(-1);
            hipLaunchKernelGGL(k_sp_place, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_ct.as<int8_t>(), t, d_offt.as<unsigned long long>(), (unsigned long long)(base[t] + H), n_rec,
                               d_off.as<unsigned long long>());
            LSG_HIP_OR(hipMemcpyAsync(&bytes_t, d_offt.as<unsigned long long>() + n_rec, 8, hipMemcpyDeviceToHost, st), done(-1));
            LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        }
        info->n_written[t] = (int64_t)h_small[1 + 5 + 2 * lsr::N_REASONS + t]; info->n_ubytes[t] = (int64_t)(H + bytes_t);
        base[t + 1] = (base[t] + H + bytes_t + 15u) & ~(uint64_t)15;
    }
    LSG_HIP_OR(hipEventRecord(ev[1], st), done(-1));
    // ---- 4. cut: the blocks BgzfWriter makes of each stream
    std::vector<SpBlk> blocks;
    {
        const auto t_cut = std::chrono::steady_clock::now();
        std::vector<uint32_t> h_len(n_rec); std::vector<int8_t> h_ct(n_rec);
        if (n_rec) {
            LSG_HIP_OR(hipMemcpyAsync(h_len.data(), d_len.p, n_rec * 4, hipMemcpyDeviceToHost, st), done(-1));
            LSG_HIP_OR(hipMemcpyAsync(h_ct.data(), d_ct.p, n_rec, hipMemcpyDeviceToHost, st), done(-1));
            LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        }
        std::vector<SpBlk> per[LSG_MAX_CELLTYPES];
        std::vector<SpCutter> cut;
        for (int32_t t = 0; t < n_celltypes; ++t) { cut.push_back(SpCutter{&per[t], base[t], (uint32_t)t}); cut.back().write(H); }
        for (uint64_t i = 0; i < n_rec; ++i) if (h_ct[i] >= 0) cut[(size_t)h_ct[i]].write_record(h_len[i]);
        for (int32_t t = 0; t < n_celltypes; ++t) { cut[(size_t)t].finish(); info->n_blocks[t] = (int64_t)per[t].size(); blocks.insert(blocks.end(), per[t].begin(), per[t].end()); }
        info->ms_cut = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_cut).count();
        if (blocks.size() >= 0x7fffffffull) { set_error("lsg_split_bam: more than 2^31 blocks"); return done(-2); }
    }
    // ---- 5. gather
    if (int rc = sp_reserve(d_streams, (size_t)base[n_celltypes] + 64, who, "the cell types' streams")) return done(rc);
    LSG_HIP_OR(hipEventRecord(ev[2], st), done(-1));
    for (int32_t t = 0; t < n_celltypes; ++t) LSG_HIP_OR(hipMemcpyAsync(d_streams.as<uint8_t>() + base[t], u, (size_t)H, hipMemcpyDeviceToDevice, st), done(-1));      // template=infile (:57)
    if (n_rec) {
        SpGatherArgs g{u, fr.d_recoff.as<uint64_t>(), n_rec, d_len.as<uint32_t>(), d_ct.as<int8_t>(), d_trim.as<uint2>(), d_off.as<unsigned long long>(), d_streams.as<uint8_t>()};
        hipLaunchKernelGGL(k_sp_gather, dim3((unsigned)((n_rec + 3) / 4)), dim3(256), 0, st, g);
    }
    LSG_HIP_OR(hipEventRecord(ev[3], st), done(-1));
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    (void)hipEventElapsedTime(&info->ms_route, ev[0], ev[1]); (void)hipEventElapsedTime(&info->ms_gather, ev[2], ev[3]);
    // ---- 5b. lsg_set_split_index: per cell type its records' facts (refID, pos, end, flag 0x4, offset in its stream), checked for the order
    if (with_index)
        for (int32_t t = 0; t < n_celltypes; ++t) {
            const auto t_bai = std::chrono::steady_clock::now();
            const uint64_t n_t = (uint64_t)info->n_written[t];
            bai_i[t].bad_ordinal = -1;
            if (n_t) {
                if (int rc = sp_reserve(d_sel, n_t * 4 + 16, who, "a cell type's record list")) return done(rc);
                uint32_t* rank = d_offt.as<uint32_t>();          // (n_rec + 1 words of the scan's buffer, free since the place)
                hipcub::TransformInputIterator<uint32_t, SpIsOf, hipcub::CountingInputIterator<uint32_t>> it(iota, SpIsOf{d_ct.as<int8_t>(), t, n_rec});
                if (exclusive_sum(fr.d_tmp, it, rank, (int64_t)n_rec + 1, st)) return done(-1);
                hipLaunchKernelGGL(k_sp_select, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_ct.as<int8_t>(), t, rank, n_rec, d_sel.as<uint32_t>());
            }
            const int rc = bai_facts(c, who, u, utotal, fr.d_recoff.as<uint64_t>(), d_sel.as<uint32_t>(), n_t, (int32_t)ref_len.size(), d_off.as<unsigned long long>(),
                                     (unsigned long long)base[t], status, bai_f[t], &bai_i[t]);
            bai_i[t].ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_bai).count();
            if (rc) {                                              // (a refusal names the ordinal in cell type t's file)
                c->split_bai[t] = bai_i[t]; c->split_bai_n = t + 1;
                if (bai_i[t].bad_kind) set_error("lsg_split_bam: cell type %d's file cannot be indexed: record %lld of it: %s (without lsg_set_split_index the files are written)", t,
                                                 (long long)bai_i[t].bad_ordinal, bai_err_text(bai_i[t].bad_kind));
                return done(rc);
            }
        }
    // ---- 6. deflate, CRC, pack - with the inflated input and every per-record array gone
    fr.release();
    for (DevBuf* b : {&d_len, &d_ct, &d_trim, &d_offt, &d_off, &d_sel}) b->release();
    SpTimes tm;
    std::vector<uint32_t> h_cs;
    if (const int rc = sp_compress(c, who, d_streams, blocks, n_celltypes, LSG_TABLE_SPLIT_BAM, info->n_file_bytes, &tm, with_index ? &h_cs : nullptr)) {
        drop_tables();
        return done(rc);
    }
    // ---- 7. lsg_set_split_index: every block's place in its file is known now -> the indexes
    if (with_index) {
        size_t b = 0;
        for (int32_t t = 0; t < n_celltypes; ++t) {
            const auto t_bai = std::chrono::steady_clock::now();
            std::vector<uint64_t> blk_ustart, blk_coff;
            uint64_t coff = 0;
            for (; b < blocks.size() && blocks[b].stream == (uint32_t)t; ++b) { blk_ustart.push_back(blocks[b].off - base[t]); blk_coff.push_back(coff); coff += (uint64_t)h_cs[b] + 26u; }
            int rc = coff + 28 == (uint64_t)info->n_file_bytes[t] ? 0 : -1;
            if (rc) set_error("lsg_split_bam: cell type %d's blocks end at %llu of %lld bytes", t, (unsigned long long)coff, (long long)info->n_file_bytes[t]);
            else rc = bai_build(c, who, bai_f[t], blk_ustart, blk_coff, coff << 16, LSG_TABLE_SPLIT_BAI + t, d_bai_tmp, &bai_i[t]);
            if (rc) { drop_tables(); return done(rc); }
            bai_f[t].release();
            bai_i[t].ms_total += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_bai).count();
            c->split_bai[t] = bai_i[t];
        }
        c->split_bai_n = n_celltypes;
    }
    info->ms_deflate = tm.deflate; info->ms_crc = tm.crc; info->ms_pack = tm.pack;
    info->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    return done(0);
}
