// The front half of the device-side BAM ingest (ingest.hip), shared by lsg_load_bam / lsg_load_bam_range and lsg_bam_fastq (fastq.hip):
// the host walks the BGZF block headers, the file goes to the device, k_inflate + k_block_crc, the record chain (k_chain / k_chain_fix
// until nothing moves) and every record's offset (k_rec_list).  What a caller gets: the uncompressed stream and the record list, on the
// device, and the phases' times.
#pragma once
#include "lsg_ctx.h"
#include "bamrec_core.h"
#include <cstring>
#include <vector>

namespace lsg {

struct IngestFront {
    DevBuf d_comp, d_u, d_blk, d_in, d_land, d_nrec, d_base, d_status, d_recoff, d_tmp;
    // d_u: the uncompressed stream (utotal bytes);  d_recoff: uint64 offset of every record's block_size word (n_rec + 1 entries reserved);
    // d_status: 16 uint32 words the caller's record kernels may go on using (words 0..3: flags, first bad block, smallest reason, changed);
    // d_tmp: scan scratch, the caller's to grow
    uint64_t utotal = 0, n_rec = 0;
    uint32_t n_blk = 0;
    // the file's NON-EMPTY BGZF blocks in file order, on the host: where each starts in the uncompressed stream and in the file, and the file
    // offset behind the last of them (what a virtual offset is made of: bamindex.hip)
    std::vector<uint64_t> blk_ustart, blk_coff;
    uint64_t data_end = 0;
    int rounds = 0;                                     // rounds of the chain beyond the first
    float ms_h2d = 0, ms_inflate = 0, ms_chain = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // start, copied, inflated, chain settled (ev[3]: where a caller's decode time starts)
    void release() {
        for (DevBuf* b : {&d_comp, &d_u, &d_blk, &d_in, &d_land, &d_nrec, &d_base, &d_status, &d_recoff, &d_tmp}) b->release();
        for (auto& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
    ~IngestFront() { release(); }
};

// who: the caller's name in the error texts.  range: the bytes are a slice of a file (lsg_load_bam_range: its last record may be cut).
// Returns 0, or the caller's return value: -1 corrupt file / device error, -2 too many records, -3 no room for the inflate tables,
// -4 the record chain did not settle in LSG_CHAIN_ROUNDS rounds (decode on the host).
int ingest_front(lsg_ctx* c, const char* who, const uint8_t* file, int64_t n_bytes, int64_t first_record_offset, int range, IngestFront& f);

// the reference lengths of the BAM header in the first bytes of the uncompressed stream (h.size() = first_record_offset: the header
// must end there)
inline bool parse_bam_refs(const std::vector<uint8_t>& h, std::vector<int64_t>& lens) {
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
