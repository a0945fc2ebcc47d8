// One BAM record -> the pieces of its FASTQ text, shared by the device printer (csrc/fastq.hip) and its host twin (lsio_bam_fastq in hostio/bamio.cpp):
// which bytes of the record the header line "@<CB>^<UMI>^<name>" is made of, the record's text length, and whether the record can be
// printed at all.  No allocation; every loop is bounded by the record's own length fields (validated by lsr::validate / record_ok before).
//
// Replaces, per record, bam_to_fastq's name / CB / UMI logic (FusionCalling/BamToFastq.py:15-42) and the SAM rendering of SEQ / QUAL that
// pysam's read.to_dict() goes through (htslib sam_format1).
#pragma once
#include "bamrec_core.h"

namespace lsf {

enum { FQ_OK = -1, FQ_NO_CB = 0, FQ_CB_TYPE = 1, FQ_UB_TYPE = 2, FQ_NM_TYPE = 3, FQ_NH_TYPE = 4 };      // = LSG_FASTQ_* (include/longsom_hip.h)

inline const char* bad_text(int kind) {
    return kind == FQ_NO_CB ? "it has no CB tag (the reference prints the previous read's barcode, or raises NameError on the first read)" :
           kind == FQ_CB_TYPE ? "its first CB tag is not of type Z" :
           kind == FQ_UB_TYPE ? "its first UB tag is not of type Z" :
           kind == FQ_NM_TYPE ? "its nM tag is not a number (the reference's split_bam raises TypeError)" :
           kind == FQ_NH_TYPE ? "its NH tag is not a number (the reference's split_bam raises TypeError)" : "?";
}

// The header line's pieces as byte ranges of the record (rec points at refID), the flags of its SEQ / QUAL lines
struct FqRec {
    uint32_t cb_off, cb_len;              // the CB value without one trailing "-1"
    uint32_t umi_off, umi_len;            // the UMI: a range of the UB value or of the name; umi_na: the literal "NA"
    uint32_t name_len;                    // strnlen of the read name
    uint32_t l_seq;
    uint8_t umi_na, no_qual;              // no_qual: QUAL prints "*" (l_seq == 0 or the first quality byte is 0xFF)
};

// FIRST aux field named t0 t1 (htslib bam_aux_get order): *type = its type byte (0: none), for Z its value's offset and length
LSR_FN void first_tags(const uint8_t* rec, uint32_t len, uint8_t* cb_type, uint32_t* cb_off, uint32_t* cb_len, uint8_t* ub_type, uint32_t* ub_off, uint32_t* ub_len) {
    const uint32_t l_name = rec[8], n_cigar = lsr::rd16(rec + 12), l_seq = lsr::rd32(rec + 16);
    uint64_t a = 32ull + l_name + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq;
    const uint64_t end = len;
    *cb_type = 0; *ub_type = 0; *cb_off = *cb_len = *ub_off = *ub_len = 0;
    while (a + 3 <= end && !(*cb_type && *ub_type)) {
        const uint8_t t0 = rec[a], t1 = rec[a + 1], ty = rec[a + 2];
        a += 3;
        uint64_t sz = 0, zlen = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
        else if (ty == 's' || ty == 'S') sz = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') {
            uint64_t z = a;
            while (z < end && rec[z]) ++z;
            zlen = z - a; sz = zlen + 1;
        } else if (ty == 'B') {
            if (a + 5 > end) break;
            const uint8_t st = rec[a]; const uint64_t cnt = lsr::rd32(rec + a + 1);
            sz = 5 + cnt * ((st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u);
        } else break;
        if (sz > end - a) break;                      // a field that claims more bytes than the record has (an unterminated string too)
        if (t0 == 'C' && t1 == 'B' && !*cb_type) { *cb_type = ty; *cb_off = (uint32_t)a; *cb_len = (uint32_t)zlen; }
        else if (t0 == 'U' && t1 == 'B' && !*ub_type) { *ub_type = ty; *ub_off = (uint32_t)a; *ub_len = (uint32_t)zlen; }
        a += sz;
    }
}

// The record's pieces; returns FQ_OK or why it cannot be printed (BamToFastq.py:24-37)
LSR_FN int describe(const uint8_t* rec, uint32_t len, FqRec* r) {
    const uint32_t l_name = rec[8], n_cigar = lsr::rd16(rec + 12), l_seq = lsr::rd32(rec + 16);
    uint8_t cb_type, ub_type; uint32_t ub_off, ub_len;
    first_tags(rec, len, &cb_type, &r->cb_off, &r->cb_len, &ub_type, &ub_off, &ub_len);
    uint32_t nl = 0;
    while (nl + 1 < l_name && rec[32 + nl]) ++nl;
    r->name_len = nl; r->l_seq = l_seq;
    r->no_qual = (l_seq == 0 || rec[32ull + l_name + 4ull * n_cigar + (l_seq + 1) / 2] == 0xff) ? 1 : 0;
    r->umi_na = 0; r->umi_off = 0; r->umi_len = 0;
    if (!cb_type) return FQ_NO_CB;
    if (cb_type != 'Z') return FQ_CB_TYPE;
    if (ub_type && ub_type != 'Z') return FQ_UB_TYPE;
    if (r->cb_len >= 2 && rec[r->cb_off + r->cb_len - 2] == '-' && rec[r->cb_off + r->cb_len - 1] == '1') r->cb_len -= 2;      // re.sub("-1$", "", CB)
    if (ub_type) { r->umi_off = ub_off; r->umi_len = ub_len; return FQ_OK; }
    // name.split('.')[-2][:-3]: the field between the last dot and the one before it (or the name's start)
    int64_t last = -1, prev = -1;
    for (uint32_t i = 0; i < nl; ++i) if (rec[32 + i] == '.') { prev = last; last = (int64_t)i; }
    if (last < 0) { r->umi_na = 1; r->umi_len = 2; return FQ_OK; }
    const uint32_t f0 = (uint32_t)(prev + 1), fl = (uint32_t)last - f0;
    r->umi_off = 32 + f0; r->umi_len = fl > 3 ? fl - 3 : 0;
    return FQ_OK;
}

LSR_FN uint32_t header_len(const FqRec& r) { return 1 + r.cb_len + 1 + r.umi_len + 1 + r.name_len + 1; }      // '@' CB '^' UMI '^' name '\n'
LSR_FN uint32_t seq_line_len(const FqRec& r) { return (r.l_seq ? r.l_seq : 1u) + 1u; }
LSR_FN uint32_t qual_line_len(const FqRec& r) { return (r.no_qual ? 1u : r.l_seq) + 1u; }
LSR_FN uint64_t text_len(const FqRec& r) { return (uint64_t)header_len(r) + seq_line_len(r) + 2u + qual_line_len(r); }
// byte k of the header line (k < header_len)
LSR_FN uint8_t header_byte(const uint8_t* rec, const FqRec& r, uint32_t k) {
    if (k == 0) return '@';
    k -= 1;
    if (k < r.cb_len) return rec[r.cb_off + k];
    k -= r.cb_len;
    if (k == 0) return '^';
    k -= 1;
    if (k < r.umi_len) return r.umi_na ? (k == 0 ? 'N' : 'A') : rec[r.umi_off + k];
    k -= r.umi_len;
    if (k == 0) return '^';
    k -= 1;
    if (k < r.name_len) return rec[32 + k];
    return '\n';
}

// Routed mode: the cell type SplitBamCellTypes.py:65-124 writes the record to (-1: none), decided as lsg_load_bam decides it; *bad =
// FQ_NM_TYPE / FQ_NH_TYPE where its filters raise
LSR_FN int32_t route(const uint8_t* rec, uint32_t len, const lsr::CbTable& cbt, int32_t min_mapq, int32_t max_nm, int32_t max_nh, int* bad) {
    *bad = FQ_OK;
    if ((int32_t)lsr::rd32(rec) < 0) return -1;                           // infile.fetch() iterates reads placed on a reference
    uint32_t cb = 0, raw = 0, clean = 0;
    lsr::AuxNum nm, nh;
    if (!lsr::scan_aux(rec, len, &cb, &raw, &clean, &nm, &nh)) return -1;
    const int32_t ct = lsr::cb_lookup(cbt, rec + cb, clean);
    if (ct < 0) return -1;
    if (max_nm >= 0 && nm.kind == lsr::AUX_BAD) { *bad = FQ_NM_TYPE; return -1; }
    if (max_nh >= 0 && nh.kind == lsr::AUX_BAD) { *bad = FQ_NH_TYPE; return -1; }
    return lsr::reason_of(nm, nh, max_nm, max_nh, (int)rec[9] < min_mapq) == 0 ? ct : -1;
}

} // namespace lsf
