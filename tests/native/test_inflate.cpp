// Host build of longsom_amd/csrc/inflate_core.h (the GPU's per-lane DEFLATE decoder) against zlib: every stream zlib's deflate writes
// (levels 0-9, default / fixed / huffman-only / RLE strategies, random and compressible data, BGZF-sized) must inflate to the same
// bytes; truncated and corrupted streams must fail cleanly (the binary is built with -fsanitize=address,undefined by the test).
// Members spliced from several streams of different level and strategy (full flushes between them: what a multi-threaded or a
// libdeflate writer leaves in one BGZF block) must inflate too, down to pieces of 0 and 1 bytes, and the damaged members of
// tests/test_bgzf_shapes_gpu.py - a stored block's wrong NLEN, an ISIZE one off, the reserved block type - must be refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "../../longsom_amd/csrc/inflate_core.h"

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t>& src, int level, int strategy) {
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) { fprintf(stderr, "deflateInit2 failed\n"); exit(2); }
    std::vector<uint8_t> out(src.size() + src.size() / 8 + 1024);
    zs.next_in = (Bytef*)src.data(); zs.avail_in = (uInt)src.size(); zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "deflate failed\n"); exit(2); }
    out.resize(zs.total_out); deflateEnd(&zs);
    return out;
}

// several pieces as ONE raw stream: each piece a deflate stream of its own, all but the last ended by a full flush (an empty stored
// block, not final), the last by Z_FINISH
struct Piece { std::vector<uint8_t> data; int level, strategy; };
static std::vector<uint8_t> deflate_spliced(const std::vector<Piece>& pieces) {
    std::vector<uint8_t> all;
    for (size_t i = 0; i < pieces.size(); ++i) {
        const Piece& pc = pieces[i];
        z_stream zs; memset(&zs, 0, sizeof(zs));
        if (deflateInit2(&zs, pc.level, Z_DEFLATED, -15, 8, pc.strategy) != Z_OK) { fprintf(stderr, "deflateInit2 failed\n"); exit(2); }
        std::vector<uint8_t> out(pc.data.size() + pc.data.size() / 8 + 1024);
        zs.next_in = (Bytef*)pc.data.data(); zs.avail_in = (uInt)pc.data.size(); zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
        const bool last = i + 1 == pieces.size();
        const int rc = deflate(&zs, last ? Z_FINISH : Z_FULL_FLUSH);
        if (rc != (last ? Z_STREAM_END : Z_OK) || zs.avail_in != 0 || zs.avail_out == 0) { fprintf(stderr, "deflate of a piece failed\n"); exit(2); }
        all.insert(all.end(), out.begin(), out.begin() + (long)zs.total_out);
        deflateEnd(&zs);
    }
    return all;
}

// zlib's own inflate says what a stream is: Z_STREAM_END with exactly n bytes, or an error
static bool zlib_accepts(const std::vector<uint8_t>& z, size_t n) {
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) exit(2);
    std::vector<uint8_t> out(n + 1);
    zs.next_in = (Bytef*)z.data(); zs.avail_in = (uInt)z.size(); zs.next_out = out.data(); zs.avail_out = (uInt)n;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.avail_out == 0;
    inflateEnd(&zs);
    return ok;
}

static std::vector<uint8_t> make_data(int kind, size_t n) {
    std::vector<uint8_t> d(n);
    for (size_t i = 0; i < n; ++i) {
        switch (kind) {
            case 0: d[i] = (uint8_t)rnd(); break;                                  // incompressible
            case 1: d[i] = "ACGT"[rnd() & 3]; break;                               // 2 bits of entropy per byte
            case 2: d[i] = (uint8_t)(i < 64 ? rnd() : d[i - 1 - (rnd() % 64)]); break;   // long matches at short distances
            case 3: d[i] = (uint8_t)((i / 97) & 0xff); break;                      // runs
            default: d[i] = (uint8_t)((rnd() % 100) < 90 ? 'A' + (rnd() % 4) : rnd()); break;   // BAM-like: mostly a few symbols
        }
    }
    return d;
}

int main() {
    std::vector<uint8_t> tab(lsi::T_SYM); std::vector<uint8_t> lens(lsi::T_LENS);
    lsi::Tab t{tab.data(), lens.data(), 1};
    long n_ok = 0, n_bad = 0;
    const size_t sizes[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 24, 255, 4096, 65280, 65535, 65536};
    const int strategies[] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
    for (int kind = 0; kind < 5; ++kind)
        for (size_t n : sizes)
            for (int level : {0, 1, 6, 9})
                for (int st : strategies) {
                    const std::vector<uint8_t> src = make_data(kind, n), z = deflate_raw(src, level, st);
                    std::vector<uint8_t> out(n + 1, 0xEE);
                    const int rc = lsi::inflate_raw(z.data(), z.size(), out.data(), n, t);
                    if (rc != 0 || (n && memcmp(out.data(), src.data(), n) != 0) || out[n] != 0xEE) {
                        fprintf(stderr, "MISMATCH kind %d n %zu level %d strategy %d rc %d\n", kind, n, level, st, rc); return 1;
                    }
                    ++n_ok;
                    // wrong expected size, truncation, bit flips: must return an error or (bit flips) any result, never touch memory outside
                    if (n > 0 && lsi::inflate_raw(z.data(), z.size(), out.data(), n - 1, t) == 0) { fprintf(stderr, "short output accepted\n"); return 1; }
                    std::vector<uint8_t> out2(n + 2, 0xEE);
                    if (lsi::inflate_raw(z.data(), z.size(), out2.data(), n + 1, t) == 0) { fprintf(stderr, "long output accepted\n"); return 1; }
                    if (z.size() > 2) {
                        std::vector<uint8_t> cut(z.begin(), z.begin() + (long)(z.size() / 2));
                        if (lsi::inflate_raw(cut.data(), cut.size(), out.data(), n, t) == 0 && n > 8) { fprintf(stderr, "truncated stream accepted\n"); return 1; }
                        for (int k = 0; k < 8; ++k) {
                            std::vector<uint8_t> bad = z;
                            bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() & 7));
                            std::vector<uint8_t> o(n + 1, 0xEE);
                            (void)lsi::inflate_raw(bad.data(), bad.size(), o.data(), n, t);
                            if (o[n] != 0xEE) { fprintf(stderr, "wrote past the output\n"); return 1; }
                            ++n_bad;
                        }
                    }
                }
    // spliced members: two to five pieces of different level and strategy, pieces of 0 and 1 bytes among them
    long n_spliced = 0, n_refused = 0;
    {
        const size_t piece_sizes[] = {0, 1, 0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 100, 1000, 5000, 16000};
        const int levels[] = {0, 1, 6, 9};
        for (int trial = 0; trial < 600; ++trial) {
            const int n_pieces = 2 + (int)(rnd() % 4);
            std::vector<Piece> pieces; std::vector<uint8_t> src;
            for (int i = 0; i < n_pieces; ++i) {
                // (the first 200 trials: tiny pieces only, members of 0 - 16 bytes and a little more)
                const size_t n = piece_sizes[rnd() % (trial < 200 ? 8 : 17)];
                Piece pc{make_data((int)(rnd() % 5), n), levels[(trial + i) & 3], strategies[(trial / 4 + i) % 5]};
                src.insert(src.end(), pc.data.begin(), pc.data.end());
                pieces.push_back(pc);
            }
            const size_t n = src.size();
            const std::vector<uint8_t> z = deflate_spliced(pieces);
            if (!zlib_accepts(z, n)) { fprintf(stderr, "zlib refuses spliced member %d\n", trial); return 2; }
            std::vector<uint8_t> out(n + 1, 0xEE);
            const int rc = lsi::inflate_raw(z.data(), z.size(), out.data(), n, t);
            if (rc != 0 || (n && memcmp(out.data(), src.data(), n) != 0) || out[n] != 0xEE) { fprintf(stderr, "MISMATCH spliced member %d (%d pieces, %zu bytes) rc %d\n", trial, n_pieces, n, rc); return 1; }
            ++n_spliced;
            // ISIZE one off, either way
            if (n > 0 && lsi::inflate_raw(z.data(), z.size(), out.data(), n - 1, t) == 0) { fprintf(stderr, "spliced member %d: ISIZE - 1 accepted\n", trial); return 1; }
            std::vector<uint8_t> out2(n + 2, 0xEE);
            if (lsi::inflate_raw(z.data(), z.size(), out2.data(), n + 1, t) == 0 || out2[n + 1] != 0xEE) { fprintf(stderr, "spliced member %d: ISIZE + 1 accepted\n", trial); return 1; }
            n_refused += 2;
        }
    }
    // damaged members: a good first piece (ended by a full flush, so what follows starts on a byte), then ...
    for (size_t n1 : {(size_t)0, (size_t)1, (size_t)9, (size_t)700})
        for (size_t n2 : {(size_t)0, (size_t)1, (size_t)7, (size_t)750}) {
            const std::vector<uint8_t> a = make_data(4, n1), b = make_data(1, n2);
            std::vector<uint8_t> head = deflate_spliced({Piece{a, 6, Z_DEFAULT_STRATEGY}, Piece{{}, 6, Z_DEFAULT_STRATEGY}});
            head.resize(head.size() - 2);                        // (without the empty final block of the second piece: 03 00)
            const size_t n = n1 + n2;
            std::vector<uint8_t> good = head, nlen = head, type3 = head;
            const uint8_t st[5] = {1, (uint8_t)n2, (uint8_t)(n2 >> 8), (uint8_t)~n2, (uint8_t)(~n2 >> 8)};      // a final stored block of b
            good.insert(good.end(), st, st + 5); good.insert(good.end(), b.begin(), b.end());
            nlen = good; nlen[head.size() + 4] ^= 1;             // ... the same with a wrong NLEN
            type3.push_back(7); type3.insert(type3.end(), b.begin(), b.end());      // ... a final block of the reserved type 3
            std::vector<uint8_t> out(n + 1, 0xEE);
            if (!zlib_accepts(good, n) || zlib_accepts(nlen, n) || zlib_accepts(type3, n) || zlib_accepts(type3, n1)) { fprintf(stderr, "zlib disagrees on the damaged members\n"); return 2; }
            if (lsi::inflate_raw(good.data(), good.size(), out.data(), n, t) != 0 || out[n] != 0xEE) { fprintf(stderr, "hand-made stored block refused (%zu + %zu)\n", n1, n2); return 1; }
            if (lsi::inflate_raw(nlen.data(), nlen.size(), out.data(), n, t) == 0) { fprintf(stderr, "wrong NLEN accepted (%zu + %zu)\n", n1, n2); return 1; }
            if (lsi::inflate_raw(type3.data(), type3.size(), out.data(), n, t) == 0 || lsi::inflate_raw(type3.data(), type3.size(), out.data(), n1, t) == 0) { fprintf(stderr, "block type 3 accepted (%zu + %zu)\n", n1, n2); return 1; }
            if (out[n] != 0xEE) { fprintf(stderr, "a damaged member wrote past the output\n"); return 1; }
            ++n_spliced; n_refused += 3;
        }
    // the strided table layout the device uses ([index][lane], stride 64): same result through lane 37 of a 64-lane image
    {
        std::vector<uint8_t> img((size_t)lsi::T_SYM * 64, 0xCD); std::vector<uint8_t> limg((size_t)lsi::T_LENS * 64, 0xAB);
        lsi::Tab ts{img.data() + 37, limg.data() + 37, 64};
        const std::vector<uint8_t> src = make_data(4, 60000), z = deflate_raw(src, 6, Z_DEFAULT_STRATEGY);
        std::vector<uint8_t> out(src.size());
        if (lsi::inflate_raw(z.data(), z.size(), out.data(), out.size(), ts) != 0 || out != src) { fprintf(stderr, "strided tables failed\n"); return 1; }
        for (size_t i = 0; i < img.size(); ++i) if ((i & 63) != 37 && img[i] != 0xCD) { fprintf(stderr, "strided tables wrote another lane's word\n"); return 1; }
        for (size_t i = 0; i < limg.size(); ++i) if ((i & 63) != 37 && limg[i] != 0xAB) { fprintf(stderr, "strided tables wrote another lane's byte\n"); return 1; }
    }
    printf("inflate ok: %ld streams and %ld spliced members equal zlib, %ld corrupted streams handled, %ld damaged members refused\n", n_ok, n_spliced, n_bad, n_refused);
    return 0;
}
