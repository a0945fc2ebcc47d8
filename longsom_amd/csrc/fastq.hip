// FASTQ for the fusion caller, printed on the device: a BAM's records as "@<CB>^<UMI>^<name>\n<seq>\n+\n<qual>\n" in table
// LSG_TABLE_FASTQ (include/longsom_hip.h lsg_bam_fastq has the semantics).
//
// Replaces bam_to_fastq (workflow/scripts/FusionCalling/BamToFastq.py:9-42: one pysam record -> read.to_dict() -> four f.write per read)
// and, in routed mode, rules BamToFastq + ConcatFastq over SplitBamCellTypes' BAMs (workflow/rules/FusionCalling.smk:3-37):
//   ingest_front   H2D, k_inflate, k_block_crc, the record chain, k_rec_list: lsg_load_bam's front half (ingest_front.h)
//   k_fq_len       one thread per record (fastq_core.h): validation, the routing decision (the load's scan_aux / cb_lookup / reason_of),
//                  the first CB / UB fields and the name's UMI field -> the record's text length, its cell type, the pieces of its
//                  header line; the smallest (ordinal << 3 | kind) of a record that cannot be printed
//   scans          per cell type an exclusive sum of the 64-bit lengths of its records (hipcub): cell type t's text follows t - 1's
//   k_fq_print     one WAVE per record, a long read strided over by its wave: the header line a byte per lane; SEQ 16 bases per lane and
//                  step (8 packed bytes -> 16 characters through a 256-entry byte -> two-characters table in LDS), QUAL 16 bytes per lane
//                  and step (+33 per byte, carry-free); a line's unaligned head and tail as byte stores, its body as 16-byte stores
// A byte-expansion job: 1.5 bytes read and 2 written per base, bound by the HBM writes and then by the file system.
#include "lsg_ctx.h"
#include "ingest_front.h"
#include "fastq_core.h"
#include "cbtable_host.h"
#include "cub_tmp.h"
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

namespace lsg {

struct FqLenArgs {
    const uint8_t* u; uint64_t total; const uint64_t* rec_off; uint64_t n_rec;
    int32_t n_ref; const int64_t* ref_len;
    int32_t routed; lsr::CbTable cbt; int32_t min_mapq, max_nm, max_nh;
    lsf::FqRec* recs; uint32_t* len; int8_t* ct;
    unsigned long long* err;              // smallest (ordinal << 3 | kind) of a record that cannot be printed (~0: none)
    unsigned long long* n_printed;        // [LSG_MAX_CELLTYPES]
    uint32_t* status;                     // ingest_front's words: bit 2 a record past the stream's end, bit 8 + word 2 lsr::validate's reason
};
__global__ __launch_bounds__(256) void k_fq_len(FqLenArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t ct = -1;
    if (i < a.n_rec) {
        const uint64_t p = a.rec_off[i];
        const uint32_t bs = lsr::rd32(a.u + p);
        const uint8_t* rec = a.u + p + 4;
        uint32_t L = 0;
        if (p + 4ull + bs > a.total) atomicOr(a.status, 2u);
        else {
            const int v = lsr::validate(rec, bs, a.n_ref, a.ref_len);
            if (v != lsr::REC_OK) { atomicOr(a.status, 8u); atomicMin(a.status + 2, (uint32_t)v); }
            else {
                int bad = lsf::FQ_OK;
                ct = a.routed ? lsf::route(rec, bs, a.cbt, a.min_mapq, a.max_nm, a.max_nh, &bad) : 0;
                lsf::FqRec r;
                if (bad == lsf::FQ_OK && ct >= 0) bad = lsf::describe(rec, bs, &r);
                if (bad != lsf::FQ_OK) { atomicMin(a.err, (unsigned long long)((i << 3) | (uint64_t)bad)); ct = -1; }
                else if (ct >= 0) { L = (uint32_t)lsf::text_len(r); a.recs[i] = r; }
            }
        }
        a.len[i] = L; a.ct[i] = (int8_t)ct;
    }
    for (int t = 0; t < LSG_MAX_CELLTYPES; ++t) {             // one atomic per wave and cell type
        const unsigned long long m = __ballot(ct == t);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(&a.n_printed[t], (unsigned long long)__popcll(m));
    }
}

struct LenOf { const uint32_t* len; const int8_t* ct; int32_t t; __host__ __device__ unsigned long long operator()(const uint32_t& i) const { return ct[i] == t ? (unsigned long long)len[i] : 0ull; } };
__global__ void k_fq_place(const int8_t* ct, int32_t t, const unsigned long long* off_t, unsigned long long base, uint64_t n_rec, unsigned long long* off) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && ct[i] == t) off[i] = base + off_t[i];
}

// A line of n characters at d: lanes write its unaligned head (< 16 bytes) and tail as bytes, its body as aligned 16-byte stores
template <class Src> __device__ __forceinline__ void put_line(char* d, uint32_t n, uint32_t lane, const Src& s) {
    const uint32_t mis = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u, head = mis < n ? mis : n;
    if (lane < head) d[lane] = (char)s.byte(lane);
    const uint32_t n_body = (n - head) >> 4;
    for (uint32_t k = lane; k < n_body; k += 64u) *reinterpret_cast<uint4*>(d + head + 16u * k) = s.chunk16(head + 16u * k);
    const uint32_t j = head + 16u * n_body + lane;
    if (j < n) d[j] = (char)s.byte(j);
    if (lane == 0) d[n] = '\n';
}
struct SeqSrc {
    const uint8_t* seq; const uint16_t* pair;         // pair[b]: the two characters of packed byte b, the high nibble's first
    __device__ __forceinline__ uint8_t byte(uint32_t j) const { return (uint8_t)(pair[seq[j >> 1]] >> ((j & 1u) ? 8 : 0)); }
    __device__ __forceinline__ uint4 chunk16(uint32_t j) const {      // bases j .. j + 15 (all inside the sequence)
        const uint8_t* p = seq + (j >> 1);
        uint64_t w;
        __builtin_memcpy(&w, p, 8);
        if (j & 1u) {                                     // the nibble stream starts at a low nibble: byte k = low(b[k]) << 4 | high(b[k + 1])
            const uint64_t M = 0x0f0f0f0f0f0f0f0full;
            w = ((w & M) << 4) | ((w >> 12) & M) | ((uint64_t)(p[8] >> 4) << 56);
        }
        uint32_t o[4];
        for (int q = 0; q < 4; ++q) o[q] = (uint32_t)pair[(w >> (16 * q)) & 0xffu] | ((uint32_t)pair[(w >> (16 * q + 8)) & 0xffu] << 16);
        return make_uint4(o[0], o[1], o[2], o[3]);
    }
};
struct QualSrc {
    const uint8_t* qual;
    __device__ __forceinline__ uint8_t byte(uint32_t j) const { return (uint8_t)(qual[j] + 33u); }
    __device__ __forceinline__ uint4 chunk16(uint32_t j) const {
        uint32_t x[4];
        __builtin_memcpy(x, qual + j, 16);
        // + 33 per byte with no carry into the next one (a quality is at most 93, but a damaged byte must wrap like the host's (uint8_t)(q + 33))
        for (int q = 0; q < 4; ++q) x[q] = ((x[q] & 0x7f7f7f7fu) + 0x21212121u) ^ (x[q] & 0x80808080u);
        return make_uint4(x[0], x[1], x[2], x[3]);
    }
};

struct FqPrintArgs { const uint8_t* u; const uint64_t* rec_off; uint64_t n_rec; const lsf::FqRec* recs; const int8_t* ct; const unsigned long long* off; char* text; };
__global__ __launch_bounds__(256) void k_fq_print(FqPrintArgs a) {
    __shared__ uint16_t pair[256];
    {
        const char* nt = "=ACMGRSVTWYHKDBN";
        const uint32_t b = threadIdx.x;
        pair[b] = (uint16_t)((uint8_t)nt[b >> 4] | ((uint32_t)(uint8_t)nt[b & 15u] << 8));
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < a.n_rec; i += n_waves) {
        if (a.ct[i] < 0) continue;
        const uint8_t* rec = a.u + a.rec_off[i] + 4;
        const lsf::FqRec r = a.recs[i];
        char* d = a.text + a.off[i];
        const uint32_t H = lsf::header_len(r);
        for (uint32_t k = lane; k < H; k += 64u) d[k] = (char)lsf::header_byte(rec, r, k);
        d += H;
        const uint8_t* seq = rec + 32 + rec[8] + 4ull * lsr::rd16(rec + 12);
        const uint8_t* qual = seq + (r.l_seq + 1) / 2;
        if (!r.l_seq) { if (lane == 0) { d[0] = '*'; d[1] = '\n'; } }
        else put_line(d, r.l_seq, lane, SeqSrc{seq, pair});
        d += lsf::seq_line_len(r);
        if (lane == 0) { d[0] = '+'; d[1] = '\n'; }
        d += 2;
        if (r.no_qual) { if (lane == 0) { d[0] = '*'; d[1] = '\n'; } }
        else put_line(d, r.l_seq, lane, QualSrc{qual});
    }
}

// the reference table of the BAM header in the first `n` bytes of the uncompressed stream (n = first_record_offset: it must end there)
static bool parse_refs(const std::vector<uint8_t>& h, std::vector<int64_t>& lens) {
    const size_t n = h.size();
    if (n < 12 || memcmp(h.data(), "BAM\1", 4) != 0) return false;
    uint64_t p = 8ull + lsr::rd32(h.data() + 4);
    if (p + 4 > n) return false;
    const uint32_t n_ref = lsr::rd32(h.data() + p); p += 4;
    for (uint32_t i = 0; i < n_ref; ++i) {
        if (p + 4 > n) return false;
        p += 4ull + lsr::rd32(h.data() + p);
        if (p + 4 > n) return false;
        lens.push_back((int64_t)lsr::rd32(h.data() + p)); p += 4;
    }
    return p == n;
}

} // namespace lsg

using namespace lsg;

extern "C" int lsg_bam_fastq(lsg_ctx* c, const uint8_t* file, int64_t n_bytes, int64_t first_record_offset, const char* barcodes, int32_t n_barcodes,
                             const int32_t* celltype_of, int32_t n_celltypes, int32_t min_mapq, lsg_fastq_info* info) {
    if (!c || !file || n_bytes < 28 || !info || first_record_offset < 12) { set_error("lsg_bam_fastq: bad arguments"); return -2; }
    const bool routed = barcodes != nullptr;
    *info = lsg_fastq_info{};
    info->bad_ordinal = -1; info->bad_kind = LSG_FASTQ_OK;
    if (routed) {
        if (n_barcodes <= 0 || !celltype_of || n_celltypes <= 0 || n_celltypes > LSG_MAX_CELLTYPES) { set_error("lsg_bam_fastq: routed mode needs a barcode list and 1..%d cell types", LSG_MAX_CELLTYPES); return -2; }
        for (int32_t i = 0; i < n_barcodes; ++i)
            if (celltype_of[i] < 0 || celltype_of[i] >= n_celltypes) { set_error("lsg_bam_fastq: barcode %d has cell type %d of %d", i, celltype_of[i], n_celltypes); return -2; }
        if (c->split_n_trim > 0) {
            set_error("lsg_bam_fastq: --n_trim %d is set on the handle: the reference would write qualities of 0 into the split BAMs; print those with BamToFastq", c->split_n_trim);
            return -2;
        }
    }
    const int32_t n_ct = routed ? n_celltypes : 1;
    LSG_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const auto t_all = std::chrono::steady_clock::now();
    c->tab_bytes[LSG_TABLE_FASTQ] = -1;                    // whatever fails below: no text is kept
    lsr::CbTableHost cbt;
    if (routed) cbt.build(barcodes, n_barcodes, celltype_of);      // the table's "id" of a barcode is its cell type
    IngestFront fr;
    DevBuf d_h, d_id, d_so, d_sl, d_str, d_reflen, d_recs, d_len, d_ct, d_offt, d_off, d_small;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto done = [&](int rc) {
        for (DevBuf* b : {&d_h, &d_id, &d_so, &d_sl, &d_str, &d_reflen, &d_recs, &d_len, &d_ct, &d_offt, &d_off, &d_small}) b->release();
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        fr.release();
        return rc;
    };
    for (auto& e : ev) LSG_HIP_OR(hipEventCreate(&e), done(-1));
    if (routed) {
        if (d_h.reserve(cbt.hash.size() * 8) || d_id.reserve(cbt.id.size() * 4) || d_so.reserve(cbt.str_off.size() * 4) || d_sl.reserve(cbt.str_len.size() * 4) || d_str.reserve(cbt.strs.size() + 16))
            return done(-1);
        LSG_HIP_OR(hipMemcpyAsync(d_h.p, cbt.hash.data(), cbt.hash.size() * 8, hipMemcpyHostToDevice, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(d_id.p, cbt.id.data(), cbt.id.size() * 4, hipMemcpyHostToDevice, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(d_so.p, cbt.str_off.data(), cbt.str_off.size() * 4, hipMemcpyHostToDevice, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(d_sl.p, cbt.str_len.data(), cbt.str_len.size() * 4, hipMemcpyHostToDevice, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(d_str.p, cbt.strs.data(), cbt.strs.size(), hipMemcpyHostToDevice, st), done(-1));
    }
    // ---- H2D, inflate, CRC, the record chain, every record's offset
    if (const int rc = ingest_front(c, "lsg_bam_fastq", file, n_bytes, first_record_offset, 0, fr)) return done(rc);
    const uint64_t n_rec = fr.n_rec, utotal = fr.utotal;
    const uint8_t* u = fr.d_u.as<uint8_t>();
    uint32_t* status = fr.d_status.as<uint32_t>();
    info->n_records = (int64_t)n_rec; info->ms_h2d = fr.ms_h2d; info->ms_inflate = fr.ms_inflate; info->ms_chain = fr.ms_chain;
    // ---- the file's own reference table (what lsr::validate checks a placed record against)
    std::vector<int64_t> ref_len;
    {
        std::vector<uint8_t> head((size_t)first_record_offset);
        LSG_HIP_OR(hipMemcpyAsync(head.data(), u, head.size(), hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        if (!parse_refs(head, ref_len)) { set_error("lsg_bam_fastq: no BAM header that ends at first_record_offset %lld", (long long)first_record_offset); return done(-1); }
    }
    if (d_reflen.reserve((ref_len.size() + 1) * 8) || d_recs.reserve((n_rec + 1) * sizeof(lsf::FqRec)) || d_len.reserve((n_rec + 2) * 4) || d_ct.reserve(n_rec + 16) ||
        d_offt.reserve((n_rec + 2) * 8) || d_off.reserve((n_rec + 2) * 8) || d_small.reserve(64)) return done(-1);
    if (!ref_len.empty()) LSG_HIP_OR(hipMemcpyAsync(d_reflen.p, ref_len.data(), ref_len.size() * 8, hipMemcpyHostToDevice, st), done(-1));
    unsigned long long* d_err = d_small.as<unsigned long long>();
    unsigned long long* d_np = d_err + 1;
    LSG_HIP_OR(hipMemsetAsync(d_err, 0xff, 8, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_np, 0, LSG_MAX_CELLTYPES * 8, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(status, 0, 4, st), done(-1));
    LSG_HIP_OR(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(status + 2), (int)0x7fffffff, 1, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_len.as<uint32_t>() + n_rec, 0, 4, st), done(-1));
    LSG_HIP_OR(hipMemsetAsync(d_ct.as<int8_t>() + n_rec, 0xff, 1, st), done(-1));
    // ---- pass 1: lengths, cell types, the first record that cannot be printed
    LSG_HIP_OR(hipEventRecord(ev[0], st), done(-1));
    unsigned long long h_small[1 + LSG_MAX_CELLTYPES] = {~0ull, 0, 0, 0, 0};
    uint32_t hstat[4] = {0, 0, 0, 0};
    if (n_rec) {
        FqLenArgs a{};
        a.u = u; a.total = utotal; a.rec_off = fr.d_recoff.as<uint64_t>(); a.n_rec = n_rec; a.n_ref = (int32_t)ref_len.size(); a.ref_len = d_reflen.as<int64_t>();
        a.routed = routed ? 1 : 0;
        a.cbt = lsr::CbTable{d_h.as<uint64_t>(), d_id.as<int32_t>(), d_so.as<uint32_t>(), d_sl.as<uint32_t>(), d_str.as<uint8_t>(), cbt.mask};
        a.min_mapq = min_mapq; a.max_nm = c->split_max_nm; a.max_nh = c->split_max_nh;
        a.recs = d_recs.as<lsf::FqRec>(); a.len = d_len.as<uint32_t>(); a.ct = d_ct.as<int8_t>(); a.err = d_err; a.n_printed = d_np; a.status = status;
        hipLaunchKernelGGL(k_fq_len, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, a);
        LSG_HIP_OR(hipMemcpyAsync(hstat, status, 16, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipMemcpyAsync(h_small, d_small.p, sizeof(h_small), hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        if (hstat[0]) {
            static const char* why[] = {"", "a record shorter than its fixed fields", "a record whose fields exceed its block_size", "a record on a reference the header does not list",
                                        "a CIGAR operation above 8", "a CIGAR that does not cover the stored sequence", "an alignment that leaves its reference"};
            set_error("lsg_bam_fastq: %s", (hstat[0] & 8u) && hstat[2] < 7 ? why[hstat[2]] : "truncated record at the end of the file");
            return done(-1);
        }
        if (h_small[0] != ~0ull) {
            const uint64_t ord = h_small[0] >> 3; const int kind = (int)(h_small[0] & 7u);
            uint64_t roff = 0; uint8_t head[32 + 256];
            LSG_HIP_OR(hipMemcpyAsync(&roff, fr.d_recoff.as<uint64_t>() + ord, 8, hipMemcpyDeviceToHost, st), done(-1));
            LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
            const size_t n_head = (size_t)(utotal - (roff + 4)) < sizeof(head) ? (size_t)(utotal - (roff + 4)) : sizeof(head);
            LSG_HIP_OR(hipMemcpyAsync(head, u + roff + 4, n_head, hipMemcpyDeviceToHost, st), done(-1));
            LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
            const uint32_t l_name = head[8];                 // validated: the name lies inside the record
            const std::string name((const char*)head + 32, l_name ? strnlen((const char*)head + 32, l_name - 1u) : 0u);
            info->bad_ordinal = (int64_t)ord; info->bad_kind = kind;
            set_error("lsg_bam_fastq: read '%s' (record %llu): %s", name.c_str(), (unsigned long long)ord, lsf::bad_text(kind));
            return done(-1);
        }
    }
    // ---- where every record's text goes: cell type after cell type, file order within one
    int64_t total = 0;
    hipcub::CountingInputIterator<uint32_t> iota(0);
    for (int32_t t = 0; t < n_ct && n_rec; ++t) {
        hipcub::TransformInputIterator<unsigned long long, LenOf, hipcub::CountingInputIterator<uint32_t>> it(iota, LenOf{d_len.as<uint32_t>(), d_ct.as<int8_t>(), t});
        if (exclusive_sum(fr.d_tmp, it, d_offt.as<unsigned long long>(), n_rec + 1, st)) return done(-1);
        hipLaunchKernelGGL(k_fq_place, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_ct.as<int8_t>(), t, d_offt.as<unsigned long long>(), (unsigned long long)total, n_rec,
                           d_off.as<unsigned long long>());
        unsigned long long bytes_t = 0;
        LSG_HIP_OR(hipMemcpyAsync(&bytes_t, d_offt.as<unsigned long long>() + n_rec, 8, hipMemcpyDeviceToHost, st), done(-1));
        LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
        info->n_printed[t] = (int64_t)h_small[1 + t]; info->n_bytes[t] = (int64_t)bytes_t;
        total += (int64_t)bytes_t;
    }
    LSG_HIP_OR(hipEventRecord(ev[1], st), done(-1));
    // ---- pass 2: the bytes
    if (total) {
        if (c->tab_text[LSG_TABLE_FASTQ].reserve((size_t)total + 16)) return done(-1);
        FqPrintArgs p{u, fr.d_recoff.as<uint64_t>(), n_rec, d_recs.as<lsf::FqRec>(), d_ct.as<int8_t>(), d_off.as<unsigned long long>(), c->tab_text[LSG_TABLE_FASTQ].as<char>()};
        unsigned g = (unsigned)((n_rec + 3) / 4); const unsigned cap = (unsigned)(c->n_cus * 32);
        if (g > cap) g = cap;
        hipLaunchKernelGGL(k_fq_print, dim3(g), dim3(256), 0, st, p);
    }
    LSG_HIP_OR(hipEventRecord(ev[2], st), done(-1));
    LSG_HIP_OR(hipGetLastError(), done(-1));
    LSG_HIP_OR(hipStreamSynchronize(st), done(-1));
    (void)hipEventElapsedTime(&info->ms_length, ev[0], ev[1]); (void)hipEventElapsedTime(&info->ms_print, ev[1], ev[2]);
    c->tab_bytes[LSG_TABLE_FASTQ] = total;
    info->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    return done(0);
}
