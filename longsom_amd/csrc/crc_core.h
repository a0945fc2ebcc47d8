// CRC32 (IEEE 802.3, reflected: zlib's crc32) of a BGZF block's <= 64 KB by 64 lanes, the arithmetic of csrc/ingest.hip's k_block_crc as
// host + device code (as inflate_core.h is): lane i takes the 1 KB chunk i (bytewise table, 16 bytes per load), the 64 chunk CRCs are
// combined as zlib's crc32_combine does - CRC is linear over GF(2): crc0(A || B) = shift(crc0(A), |B|) ^ crc0(B) with crc0 the register
// started at 0 and shift(v, n) = v run through n zero bytes, done as a product with the precomputed 32 x 32 bit matrices of 2^k zero
// bytes (zero_ops) - and the initial and final complement are put back: crc32(M) = crc0(M) ^ shift(0xffffffff, |M|) ^ 0xffffffff.
// The kernel keeps the tables' LDS staging, the xor over the lanes, the closing complement and the comparison;
// tests/native/test_crc.cpp emulates the lanes on the host and checks every chunk edge, every alignment and the 65 536-byte block
// against zlib.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifdef __HIPCC__
#define LSC_FN __host__ __device__ __forceinline__
#else
#define LSC_FN inline
#endif

namespace lsc {

constexpr uint32_t CHUNK = 1024;              // bytes of a block per lane: 64 lanes cover a block's 65 536
struct CrcTables { uint32_t byte_tab[256]; uint32_t zero_ops[17][32]; };      // zero_ops[k][j]: where bit j of the register goes under 2^k zero bytes

#ifndef __HIP_DEVICE_COMPILE__
struct __attribute__((aligned(16), may_alias)) Quad { uint32_t x, y, z, w; };      // the host's stand-in for the device's 16-byte load (aligned, as that is)
#endif

LSC_FN uint32_t crc_shift(const uint32_t (*ops)[32], uint32_t v, uint32_t n_bytes) {
    for (int k = 0; n_bytes; ++k, n_bytes >>= 1)
        if (n_bytes & 1u) { uint32_t r = 0; for (int j = 0; j < 32; ++j) r ^= (v >> j) & 1u ? ops[k][j] : 0u; v = r; }
    return v;
}

// crc0 of the bytes [lo, hi) of the block at p, which lies at offset `uoff` of a 16-byte aligned buffer (the 16-byte loads are aligned
// in THAT buffer: the bytes in front of the first boundary and behind the last go one by one)
LSC_FN uint32_t crc_chunk(const uint32_t* tab, const uint8_t* p, uint64_t uoff, uint32_t lo, uint32_t hi) {
    uint32_t c = 0;
    uint32_t i = lo;
    for (; i < hi && ((uoff + i) & 15u); ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    for (; i + 16 <= hi; i += 16) {
#ifdef __HIP_DEVICE_COMPILE__
        const uint4 q = *reinterpret_cast<const uint4*>(p + i);
#else
        const Quad q = *reinterpret_cast<const Quad*>(p + i);
#endif
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c ^= w[k];
            c = tab[c & 0xffu] ^ (c >> 8); c = tab[c & 0xffu] ^ (c >> 8); c = tab[c & 0xffu] ^ (c >> 8); c = tab[c & 0xffu] ^ (c >> 8);
        }
    }
    for (; i < hi; ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c;
}

inline void make_crc_tables(CrcTables& t) {
    for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; t.byte_tab[i] = c; }
    for (int j = 0; j < 32; ++j) { uint32_t v = 1u << j; v = t.byte_tab[v & 0xffu] ^ (v >> 8); t.zero_ops[0][j] = v; }      // one zero byte
    for (int k = 1; k < 17; ++k)                                        // the operator of 2^k zero bytes = the one of 2^(k-1) applied twice
        for (int j = 0; j < 32; ++j) { const uint32_t v = t.zero_ops[k - 1][j]; uint32_t r = 0; for (int b = 0; b < 32; ++b) r ^= (v >> b) & 1u ? t.zero_ops[k - 1][b] : 0u; t.zero_ops[k][j] = r; }
}

} // namespace lsc
