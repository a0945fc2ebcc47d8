// Host build of longsom_amd/csrc/crc_core.h (the arithmetic of the GPU's per-block CRC32, k_block_crc) against zlib's crc32.  The wave is
// emulated: every one of the 64 lanes takes its chunk's CRC, runs it through the bytes of the block behind the chunk, the 64 words
// are xor-ed and the initial and final complement put back - what the kernel does with a shuffle reduction.  Sizes around every place
// the code changes its path: the 16-byte loads' head and tail (0..40), the edges of the first and second 1 KB chunk, the last chunk's
// edge and the 65 536-byte block, the only size that sets bit 16 of a length (zero_ops[16], the last turn of crc_shift); each at all
// 16 alignments of the block in its buffer.  Built with -fsanitize=address,undefined by the test: the 16-byte loads are typed aligned
// loads here, a misaligned one stops the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "../../longsom_amd/csrc/crc_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }

static uint32_t wave_crc(const lsc::CrcTables& t, const uint8_t* p, uint64_t uoff, uint32_t usize) {
    uint32_t x = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t lo = lane * lsc::CHUNK, hi = lo + lsc::CHUNK < usize ? lo + lsc::CHUNK : usize;
        if (lo < usize) x ^= lsc::crc_shift(t.zero_ops, lsc::crc_chunk(t.byte_tab, p, uoff, lo, hi), usize - hi);
    }
    return x ^ lsc::crc_shift(t.zero_ops, 0xffffffffu, usize) ^ 0xffffffffu;
}

int main() {
    static lsc::CrcTables t;
    lsc::make_crc_tables(t);
    std::vector<uint32_t> sizes;
    for (uint32_t n = 0; n <= 40; ++n) sizes.push_back(n);
    for (uint32_t n = 1020; n <= 1030; ++n) sizes.push_back(n);
    for (uint32_t n = 2040; n <= 2056; ++n) sizes.push_back(n);
    for (uint32_t n = 65270; n <= 65290; ++n) sizes.push_back(n);
    sizes.push_back(65535); sizes.push_back(65536);
    // the buffer: 16-byte aligned (as the device's), the block at offset `uoff` of it, exactly usize bytes (ASan guards its end)
    long n_ok = 0;
    for (int constant = 0; constant < 2; ++constant)
        for (uint32_t usize : sizes)
            for (uint32_t uoff = 0; uoff < 16; ++uoff) {
                void* mem = nullptr;
                if (posix_memalign(&mem, 16, (size_t)uoff + usize + (uoff + usize ? 0 : 1)) != 0) { fprintf(stderr, "posix_memalign failed\n"); return 2; }
                uint8_t* buf = (uint8_t*)mem; uint8_t* p = buf + uoff;
                const uint8_t fill = (uint8_t)rnd();
                for (uint32_t i = 0; i < usize; ++i) p[i] = constant ? fill : (uint8_t)rnd();
                const uint32_t want = (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, usize), got = wave_crc(t, p, uoff, usize);
                free(buf);
                if (got != want) { fprintf(stderr, "MISMATCH usize %u uoff %u %s data: %08x, zlib %08x\n", usize, uoff, constant ? "constant" : "random", got, want); return 1; }
                ++n_ok;
            }
    // the shift operators by themselves: 2^k zero bytes are 2^k steps of the byte table from the same register
    for (int k = 0; k < 17; ++k) {
        const uint32_t v0 = rnd() | 1u;
        uint32_t v = v0;
        for (uint32_t i = 0; i < (1u << k); ++i) v = t.byte_tab[v & 0xffu] ^ (v >> 8);
        if (lsc::crc_shift(t.zero_ops, v0, 1u << k) != v) { fprintf(stderr, "zero_ops[%d] is not 2^%d zero bytes\n", k, k); return 1; }
    }
    printf("crc ok: %ld blocks equal zlib\n", n_ok);
    return 0;
}
