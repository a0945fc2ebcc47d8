// The arithmetic of the cell-by-gene read count that the device kernels (genecounts.hip) and a host program share: the table of
// elementary intervals, the lookup of a read's block in it, the fold of the labels it meets, a read's outcome.  Plain C++: every function
// is __host__ __device__ under hipcc and an ordinary inline function under a host compiler.
//
// Replaces the overlap test of featureCounts (rule featureCount, workflow/rules/CNACalling.smk:29-44: -t exon -g gene_id -s 0, no -O, no
// -M), restated by longsom_amd/genecounts.py, whose numpy twin is the contract.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LSGC_HD __host__ __device__ __forceinline__
#else
#define LSGC_HD inline
#endif

namespace lsgc {

// An elementary interval of the flattened annotation: [key, key + len) with key = tid << 32 | start0; start0 + len <= 2^32, so an
// interval never reaches into the next contig's keys.  label: the one gene that covers it, or AMBIG for two and more.
struct Interval { uint64_t key; uint32_t len; uint32_t label; };
static_assert(sizeof(Interval) == 16, "16 bytes an interval");
constexpr uint32_t AMBIG = 0xFFFFFFFEu;
constexpr uint32_t MAX_GENES = 0x7FFFFFFFu;

// A read's state is two words: lo = the smallest gene index its blocks met (atomicMin), hi = the largest + 1 (atomicMax).  An ambiguous
// interval counts as genes 0 and 2^32 - 2 at once.
constexpr uint32_t LO_NONE = 0xFFFFFFFFu, HI_NONE = 0u;
enum Outcome { ASSIGNED = 0, NO_FEATURES = 1, AMBIGUITY = 2, FILTERED = 3 };

LSGC_HD void fold(uint32_t label, uint32_t& lo, uint32_t& hi) {
    const uint32_t l = label == AMBIG ? 0u : label, h = label == AMBIG ? 0xFFFFFFFFu : label + 1u;
    lo = l < lo ? l : lo; hi = h > hi ? h : hi;
}
LSGC_HD int outcome(uint32_t lo, uint32_t hi) { return hi == HI_NONE ? NO_FEATURES : (uint64_t)hi == (uint64_t)lo + 1u ? ASSIGNED : AMBIGUITY; }

// is a read considered at all (the caller has checked its barcode)
LSGC_HD bool considered(uint32_t flag, uint32_t mapq, uint32_t flag_exclude, int32_t min_mapq) {
    return (flag & flag_exclude) == 0u && (int32_t)mapq >= min_mapq;
}

// the first interval that ends after `ks` (n when none does): the ends ascend with the keys, the intervals being disjoint
LSGC_HD int64_t first_ending_after(const Interval* iv, int64_t n, uint64_t ks) {
    int64_t a = 0, b = n;
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (iv[m].key + iv[m].len > ks) b = m; else a = m + 1;
    }
    return a;
}

// the labels of every interval the block [ks, ke) overlaps by at least one base, folded into (lo, hi); returns how many it met.  ke is
// on the block's own contig (ks + len, len < 2^31), so the walk stops before the next contig's first interval.
LSGC_HD int32_t fold_block(const Interval* iv, int64_t n, uint64_t ks, uint64_t ke, uint32_t& lo, uint32_t& hi) {
    int32_t met = 0;
    for (int64_t i = first_ending_after(iv, n, ks); i < n && iv[i].key < ke; ++i) { fold(iv[i].label, lo, hi); ++met; }
    return met;
}

} // namespace lsgc
