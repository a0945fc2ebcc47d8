// The two halves of the device index builder (bamindex.hip) as lsg_bam_index and lsg_split_bam (split.hip) call them: the records' facts,
// taken while the inflated stream is resident, and the index made of them once every record's virtual offset can be told.
#pragma once
#include "lsg_ctx.h"
#include <vector>

namespace lsg {

// per record of ONE file, in file order: refID, pos, the indexed interval's end (capped at 2^29 + 1), flag 0x4, and the offset of its
// block_size word in that file's uncompressed stream
struct BaiFacts {
    DevBuf tid, pos, end, unm, g, n_intv, small;      // n_intv: per reference, the last window touched + 1;  small: the smallest (ordinal << 3 | kind) refused, the placed records
    uint64_t n = 0, n_placed = 0;
    int32_t n_ref = 0;
    float ms_facts = 0;
    void release() { for (DevBuf* b : {&tid, &pos, &end, &unm, &g, &n_intv, &small}) b->release(); }
    ~BaiFacts() { release(); }
};

// u, total, rec_off: the inflated stream and its record list (ingest_front).  sel: the ordinals of the n records of this file in the
// list (null: all of the list's first n).  g_src / g_sub: a record's offset in this file's stream is g_src[ordinal] - g_sub (null: its
// offset in u).  status: ingest_front's words.  Checks every record and the order (info->bad_ordinal / bad_kind, rc -1 when refused).
int bai_facts(lsg_ctx* c, const char* who, const uint8_t* u, uint64_t total, const uint64_t* rec_off, const uint32_t* sel, uint64_t n, int32_t n_ref,
              const unsigned long long* g_src, unsigned long long g_sub, uint32_t* status, BaiFacts& f, lsg_bai_info* info);
const char* bai_err_text(int kind);      // why a record is refused (LSG_BAI_ERR_*), in lsio_build_bai_full's words

// The file's non-empty BGZF blocks in file order: where each starts in the uncompressed stream and in the file; v_eof: the virtual
// offset that ends the last record.  The .bai's bytes go into c->tab_text[table]; info's counts, n_bytes and phase times are filled.
// -3: no device memory for it, or an index of 2^31 windows or more (make that one on the host); no table is kept then.
int bai_build(lsg_ctx* c, const char* who, BaiFacts& f, const std::vector<uint64_t>& blk_ustart, const std::vector<uint64_t>& blk_coff, uint64_t v_eof, int table,
              DevBuf& tmp, lsg_bai_info* info);

} // namespace lsg
