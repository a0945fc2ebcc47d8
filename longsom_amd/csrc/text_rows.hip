// The upload and the row-start passes of the filters that read a table's text row by row (text_rows.h): hccv.hip and step3.hip run the
// same kernels over the same form of input - the text and the place of every row's first byte.
#include "text_rows.h"
#include "text_table.h"
#include <cstring>

namespace lsg {
namespace {

constexpr int PIECE = 256;                            // bytes of text a lane of the newline passes reads: sixteen 16-byte loads

// The row starts in piece t: byte 0 of the text, and every byte behind a newline that is still inside the text.  fn(place) per start, ascending.
template <class F> __device__ __forceinline__ void piece_starts(const char* text, int64_t n_bytes, int64_t t, F fn) {
    const int64_t base = t * PIECE;
    if (t == 0 && n_bytes > 0) fn((int64_t)0);
    const uint4* src = reinterpret_cast<const uint4*>(text + base);      // (the text's buffer is 256-byte aligned and padded beyond n_bytes: DevBuf)
    for (int q = 0; q < PIECE / 16; ++q) {
        const int64_t at = base + q * 16;
        if (at >= n_bytes) break;
        const uint4 v = src[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int b = 0; b < 16; ++b)
            if (((w[b >> 2] >> ((b & 3) * 8)) & 0xFFu) == (uint32_t)'\n' && at + b + 1 < n_bytes) fn(at + b + 1);
    }
}
__global__ __launch_bounds__(256) void k_text_count_starts(const char* text, int64_t n_bytes, int64_t n_pieces, uint32_t* cnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_pieces) return;
    uint32_t k = 0;
    if (t < n_pieces) piece_starts(text, n_bytes, t, [&](int64_t) { ++k; });
    cnt[t] = k;
}
// starts[n_rows] = one past the last row's newline, the one a last line may lack counted
__global__ __launch_bounds__(256) void k_text_fill_starts(const char* text, int64_t n_bytes, int64_t n_pieces, const uint64_t* off, uint64_t* starts) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_pieces) return;
    if (t == n_pieces) { starts[off[t]] = (uint64_t)n_bytes + (text[n_bytes - 1] != '\n' ? 1u : 0u); return; }
    uint64_t w = off[t];
    piece_starts(text, n_bytes, t, [&](int64_t at) { starts[w++] = (uint64_t)at; });
}

} // namespace

int find_row_starts(lsg_ctx* c, DevBuf& pieces, DevBuf& starts, const char* text, int64_t n_bytes, const char* who, int64_t* n_rows) {
    hipStream_t st = c->stream;
    const int64_t n_pieces = (n_bytes + PIECE - 1) / PIECE;
    if (n_bytes <= 0 || n_pieces >= (int64_t)1 << 31) { set_error("%s: %lld bytes of text", who, (long long)n_bytes); return -2; }
    RowPlaces pc;
    if (row_places(pieces, n_pieces, -1, pc)) return -1;
    const unsigned pblocks = (unsigned)((n_pieces + 1 + 255) / 256);
    hipLaunchKernelGGL(k_text_count_starts, dim3(pblocks), dim3(256), 0, st, text, n_bytes, n_pieces, pc.len);
    int64_t n = 0;
    if (finish_places(c, pc, &n)) return -1;
    if (n >= (int64_t)1 << 31) { set_error("%s: %lld rows", who, (long long)n); return -2; }
    if (starts.reserve((size_t)(n + 1) * 8)) return -1;
    hipLaunchKernelGGL(k_text_fill_starts, dim3(pblocks), dim3(256), 0, st, text, n_bytes, n_pieces, pc.off, starts.as<uint64_t>());
    LSG_HIP(hipGetLastError());
    *n_rows = n;
    return 0;
}

int64_t skip_comment_lines(const char* text, int64_t n_bytes) {
    int64_t at = 0;
    while (at < n_bytes && text[at] == '#') { const void* e = memchr(text + at, '\n', (size_t)(n_bytes - at)); at = e ? (const char*)e - text + 1 : n_bytes; }
    return at;
}

int upload_text(lsg_ctx* c, DevBuf& dst, const char* text, int64_t n_bytes, const char* who) {
    if (n_bytes <= 0) return 0;
    hipStream_t st = c->stream;
    if (dst.reserve((size_t)n_bytes + 16)) return -1;
    const size_t CH = 32u << 20;
    const size_t each = (size_t)n_bytes < CH ? (size_t)n_bytes : CH;
    char* pin[2] = {nullptr, nullptr}; hipEvent_t pe[2] = {nullptr, nullptr};
    bool ok = true;
    for (int i = 0; i < 2 && ok; ++i) ok = hipHostMalloc(reinterpret_cast<void**>(&pin[i]), each, hipHostMallocDefault) == hipSuccess && hipEventCreate(&pe[i]) == hipSuccess;
    size_t off = 0; int slot = 0; bool used[2] = {false, false};
    while (ok && off < (size_t)n_bytes) {
        const size_t k = (size_t)n_bytes - off < each ? (size_t)n_bytes - off : each;
        if (used[slot]) ok = hipEventSynchronize(pe[slot]) == hipSuccess;
        if (!ok) break;
        memcpy(pin[slot], text + off, k);
        ok = hipMemcpyAsync(dst.as<char>() + off, pin[slot], k, hipMemcpyHostToDevice, st) == hipSuccess && hipEventRecord(pe[slot], st) == hipSuccess;
        used[slot] = true; off += k; slot ^= 1;
    }
    if (ok) ok = hipStreamSynchronize(st) == hipSuccess;
    for (int i = 0; i < 2; ++i) { if (pe[i]) (void)hipEventDestroy(pe[i]); if (pin[i]) (void)hipHostFree(pin[i]); }
    if (!ok) { set_error("%s: copying the table to the device failed: %s", who, hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

} // namespace lsg
