// What the filters that read a table's TEXT row by row share (hccv.hip, step3.hip; the kernels are in text_rows.hip): the staged upload
// of a table the caller holds, the newline passes that find every row's first byte, the HIP-event timer of a phase, and two things their
// lane-per-row kernels do alike - a wave's tally into a counter, and a row's place in a table that holds its chrM rows last.
#pragma once
#include "lsg_ctx.h"

namespace lsg {

// text[0 .. n_bytes) into dst (grown to n_bytes + 16) through two pinned staging buffers, as lsg_load_bam takes a file's: the CPU fills
// one while the other drains.  who: the caller's name in an error.
int upload_text(lsg_ctx* c, DevBuf& dst, const char* text, int64_t n_bytes, const char* who);

// the comment lines a table starts with: the offset of its first data row
int64_t skip_comment_lines(const char* text, int64_t n_bytes);

// The row starts of n_bytes > 0 of text on the device (256-byte aligned, its buffer padded to whole 16 bytes): a newline pass counts the
// starts of every 256-byte piece, a scan places them, a second pass writes them.  starts[0 .. *n_rows] as uint64 in `starts`, entry
// n_rows = one past the last row's newline, the one a last line may lack counted - so every row ends one byte before the next one's start.
int find_row_starts(lsg_ctx* c, DevBuf& pieces, DevBuf& starts, const char* text, int64_t n_bytes, const char* who, int64_t* n_rows);

struct PhaseTimer {                                   // HIP-event time of a phase on the stream
    hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
    explicit PhaseTimer(hipStream_t s) : st(s) { if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) a = b = nullptr; }
    ~PhaseTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    PhaseTimer(const PhaseTimer&) = delete;
    PhaseTimer& operator=(const PhaseTimer&) = delete;
    void start() { if (a) (void)hipEventRecord(a, st); }
    void stop() { if (b) (void)hipEventRecord(b, st); }
    float ms() { float v = 0; if (a && b && hipEventSynchronize(b) == hipSuccess) (void)hipEventElapsedTime(&v, a, b); return v; }
};

#if defined(__HIPCC__)
// the lanes of a wave for which `mine` holds, added to *at by one of them (every lane of the wave calls it)
__device__ __forceinline__ void wave_tally(unsigned long long* at, bool mine) {
    const unsigned long long m = __ballot(mine);
    if (m && (int)(__ffsll((long long)m) - 1) == (int)(threadIdx.x & 63)) atomicAdd(at, (unsigned long long)__popcll(m));
}
// a row's place among n rows of which the chrM rows come last: off = its place among all, offm = among the chrM rows alone
__device__ __forceinline__ int64_t chrm_last(const uint64_t* off, const uint64_t* offm, int64_t i, int64_t n, bool is_m) {
    return is_m ? (int64_t)(off[n] - offm[n]) + (int64_t)offm[i] : (int64_t)(off[i] - offm[i]);
}
#endif

} // namespace lsg
