// How every table printed on the device gets its rows' places and its buffer (tables.hip, cellgeno.hip, genecounts.hip): the caller's
// first kernel measures each row into RowPlaces::len, finish_places turns the lengths into places and reads the total back, print_table
// reserves the table's text and runs the caller's second kernel.  Also the one buffer of strings such a table prints (HostBlob).
#pragma once
#include "cub_tmp.h"
#include <cstring>
#include <vector>

namespace lsg {

// The places of n rows in a scratch buffer: len[n + 1] | off[n + 1] | lo[n_contigs + 1] | shift[n_contigs + 1], each on a 256-byte
// boundary after `head` bytes of the caller's own.  lo and shift serve the tables printed contig after contig in the names' order (a
// row's place is off[i] + shift[its contig]); n_contigs = -1 leaves them out.
struct RowPlaces { uint32_t* len; uint64_t* off; int64_t* lo; int64_t* shift; int64_t n; };

// the only place that layout is computed.  grow = false: the view of places made by an earlier call with the same arguments
inline int row_places(DevBuf& scratch, int64_t n, int32_t n_contigs, RowPlaces& r, bool grow = true, size_t head = 0) {
    const size_t at_off = head + align_up((size_t)(n + 1) * 4, 256), at_lo = at_off + align_up((size_t)(n + 1) * 8, 256),
                 at_shift = at_lo + align_up((size_t)(n_contigs + 1) * 8, 256), total = at_shift + (size_t)(n_contigs + 1) * 8;
    if (grow && scratch.reserve(total)) return -1;
    char* sc = scratch.as<char>();
    r = RowPlaces{reinterpret_cast<uint32_t*>(sc + head), reinterpret_cast<uint64_t*>(sc + at_off), reinterpret_cast<int64_t*>(sc + at_lo), reinterpret_cast<int64_t*>(sc + at_shift), n};
    return 0;
}

// After the caller's length kernel: the widening scan, the caller's contig step (it queues k_contig_lo / k_contig_shift and whatever
// else has to precede the read-back; 0, or the code to return), the total through the pinned word with the one wait on the stream.
template <class C> int finish_places(lsg_ctx* c, const RowPlaces& r, int64_t* total, C contig_step) {
    hipStream_t st = c->stream;
    if (exclusive_sum(c->d_cub_tmp, hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*>(r.len, Widen()), r.off, r.n + 1, st)) return -1;
    if (int rc = contig_step()) return rc;
    LSG_HIP(hipMemcpyAsync(c->h_pin, r.off + r.n, 8, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipStreamSynchronize(st));
    *total = (int64_t)c->h_pin[0];
    return 0;
}
inline int finish_places(lsg_ctx* c, const RowPlaces& r, int64_t* total) { return finish_places(c, r, total, [] { return 0; }); }

// The table's buffer and the caller's put kernel (put(char* text) launches it); a table of no bytes launches nothing.
template <class P> int print_table(lsg_ctx* c, int32_t table, int64_t bytes, P put) {
    if (bytes > 0) {
        if (c->tab_text[table].reserve((size_t)bytes)) return -1;
        put(c->tab_text[table].as<char>());
        LSG_HIP(hipGetLastError());
        LSG_HIP(hipStreamSynchronize(c->stream));
    }
    c->tab_bytes[table] = bytes;
    return 0;
}

// Strings and index arrays uploaded as one buffer: every piece starts on an 8-byte boundary, the buffer ends in 8 bytes of padding.
struct HostBlob {
    std::vector<char> bytes;
    size_t add(const void* src, size_t n) {
        const size_t at = align_up(bytes.size(), 8);
        bytes.resize(at + n, 0);
        if (n) memcpy(bytes.data() + at, src, n);
        return at;
    }
    int upload(DevBuf& dst, hipStream_t st) {
        bytes.resize(align_up(bytes.size(), 8) + 8, 0);
        if (dst.reserve(bytes.size())) return -1;
        LSG_HIP(hipMemcpyAsync(dst.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st));
        LSG_HIP(hipStreamSynchronize(st));
        return 0;
    }
};

} // namespace lsg
