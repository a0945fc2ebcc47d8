// What the device index builder (bamindex.hip) and its host twin (lsio_build_bai_full, hostio/bamio.cpp) share of a .bai (SAM specification section 5.2) in
// this project's canonical form: the bin of an interval, a CIGAR's reference length, the key a coordinate-sorted file
// is sorted by, the refusals, and the byte layout of the file.  No allocation; every loop bounded by its arguments.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifdef __HIPCC__
#define LSB_FN __host__ __device__ __forceinline__
#else
#define LSB_FN inline
#endif

namespace lsb {

constexpr uint32_t META_BIN = 37450;            // the pseudo-bin of a reference's metadata; every real bin is below 37449
constexpr int64_t MAX_END = (int64_t)1 << 29;   // what the five bin levels hold
constexpr int WIN_SHIFT = 14;                   // the linear index's 16 kb windows
// lsg_bai_info's bad_kind (LSG_BAI_ERR_*).  Where one record breaks several rules the smallest kind is the one named
enum { ERR_NONE = 0, ERR_UNSORTED = 1, ERR_NEG_POS = 2, ERR_TOO_FAR = 3 };

// reg2bin of the specification, for the half-open interval [beg, end), 0 <= beg < end <= 2^29
LSB_FN uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

LSB_FN uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
LSB_FN bool is_ref_op(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }      // M D N = X

// the reference bases the operations first, first + step, ... < n_cigar of a CIGAR consume (first 0, step 1: the whole CIGAR; a wave
// shares a long one with first = lane, step = 64)
LSB_FN int64_t cigar_rlen(const uint8_t* cg, uint32_t n_cigar, uint32_t first, uint32_t step) {
    int64_t r = 0;
    for (uint32_t k = first; k < n_cigar; k += step) { const uint32_t c = rd32(cg + 4ull * k); if (is_ref_op(c & 0xfu)) r += (int64_t)(c >> 4); }
    return r;
}
// the indexed interval's end: pos + rlen, one position where the CIGAR consumes none
LSB_FN int64_t interval_end(int32_t pos, int64_t rlen) { return (int64_t)pos + (rlen > 0 ? rlen : 1); }

// the key a coordinate-sorted file is non-decreasing in: placed records by (refID, pos), the unplaced ones last
LSB_FN int64_t sort_key(int32_t tid, int32_t pos) { return tid < 0 ? INT64_MAX : (int64_t)tid * ((int64_t)1 << 32) + (int64_t)pos; }
// what a record is refused for on its own (ERR_UNSORTED needs its predecessor's key and comes first)
LSB_FN int record_error(int32_t tid, int32_t pos, int64_t end) { return tid < 0 ? ERR_NONE : pos < 0 ? ERR_NEG_POS : end > MAX_END ? ERR_TOO_FAR : ERR_NONE; }
// the key of a run of records and of a bin: (refID, bin)
LSB_FN uint64_t bin_key(int32_t tid, uint32_t bin) { return ((uint64_t)(uint32_t)tid << 16) | (uint64_t)bin; }
// htslib's adjacent-block merge: chunk b starts in the block where chunk a of the same bin ends
LSB_FN bool chunks_merge(uint64_t a_end, uint64_t b_beg) { return (a_end >> 16) >= (b_beg >> 16); }

// ---- the file's bytes ----
//   "BAI\1" n_ref | per reference: n_bin, { bin, n_chunk, { beg, end } x n_chunk } x n_bin, n_intv, ioffset x n_intv | n_no_coor
// A reference with records ends its bins with META_BIN: n_chunk 2, (first record's start, last record's end), (n_mapped, n_unmapped).
constexpr uint64_t HEAD_BYTES = 8, META_BYTES = 8 + 32, TAIL_BYTES = 8;
// n_bins, n_chunks: without the pseudo-bin; has_records: whether it is there
LSB_FN uint64_t bins_bytes(uint64_t n_bins, uint64_t n_chunks, bool has_records) { return 8 * n_bins + 16 * n_chunks + (has_records ? META_BYTES : 0); }
LSB_FN uint64_t ref_bytes(uint64_t n_bins, uint64_t n_chunks, bool has_records, uint64_t n_intv) { return 4 + bins_bytes(n_bins, n_chunks, has_records) + 4 + 8 * n_intv; }
// inside a reference's bytes: bin number b_rel of the reference (its c_rel chunks of earlier bins before it), chunk c_rel of the
// reference in bin b_rel, the pseudo-bin, n_intv
LSB_FN uint64_t bin_at(uint64_t b_rel, uint64_t c_rel) { return 4 + 8 * b_rel + 16 * c_rel; }
LSB_FN uint64_t chunk_at(uint64_t b_rel, uint64_t c_rel) { return 4 + 8 * (b_rel + 1) + 16 * c_rel; }
LSB_FN uint64_t meta_at(uint64_t n_bins, uint64_t n_chunks) { return 4 + 8 * n_bins + 16 * n_chunks; }
LSB_FN uint64_t intv_at(uint64_t n_bins, uint64_t n_chunks, bool has_records) { return 4 + bins_bytes(n_bins, n_chunks, has_records); }

LSB_FN void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
LSB_FN void put64(uint8_t* p, uint64_t v) { put32(p, (uint32_t)v); put32(p + 4, (uint32_t)(v >> 32)); }
LSB_FN void put_head(uint8_t* p, uint32_t n_ref) { p[0] = 'B'; p[1] = 'A'; p[2] = 'I'; p[3] = 1; put32(p + 4, n_ref); }
LSB_FN void put_meta(uint8_t* p, uint64_t first_beg, uint64_t last_end, uint64_t n_mapped, uint64_t n_unmapped) {
    put32(p, META_BIN); put32(p + 4, 2); put64(p + 8, first_beg); put64(p + 16, last_end); put64(p + 24, n_mapped); put64(p + 32, n_unmapped);
}

} // namespace lsb
