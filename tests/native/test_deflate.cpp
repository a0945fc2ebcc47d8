// Host build of longsom_amd/csrc/deflate_core.h (the GPU's per-lane DEFLATE encoder) against zlib: every stream it writes must inflate
// with zlib's inflate(-15) to the input with total_out == n, and with the device's own decoder (inflate_core.h), at stride 1 and with
// 64 emulated lanes whose tables are interleaved as on the device.  The buffers are exactly as large as the contract says (n + 5 bytes
// out), so the sanitizers see any byte touched outside them.  Arguments: BAM files whose inflated blocks are compressed too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "../../longsom_amd/csrc/deflate_core.h"
#include "../../longsom_amd/csrc/inflate_core.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11); }
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

enum { RANDOM, ONE_BYTE, PERIOD3, STRING64, FAR_REPEAT, FOUR_VALUES, TWO_VALUES, ALL_VALUES, TEXT, N_KINDS };
static void fill(int kind, uint8_t* d, size_t n) {
    uint8_t s64[64]; for (auto& b : s64) b = (uint8_t)rnd();
    const uint8_t one = (uint8_t)rnd();
    for (size_t i = 0; i < n; ++i) {
        switch (kind) {
            case RANDOM: d[i] = (uint8_t)rnd(); break;
            case ONE_BYTE: d[i] = one; break;                                     // distance 1, runs past 258
            case PERIOD3: d[i] = s64[i % 3]; break;
            case STRING64: d[i] = s64[i % 64]; break;
            case FAR_REPEAT: d[i] = i < 40000 ? (uint8_t)rnd() : d[i - 40000]; break;      // the only repeat lies beyond the window
            case FOUR_VALUES: d[i] = "ACGT"[rnd() & 3]; break;
            case TWO_VALUES: d[i] = (uint8_t)(rnd() & 1 ? 0x11 : 0xee); break;
            case ALL_VALUES: d[i] = (uint8_t)i; break;
            default: d[i] = (uint8_t)((rnd() % 100) < 85 ? "ACGTN:ZiCB"[rnd() % 10] : rnd()); break;
        }
    }
}
static std::vector<uint8_t> make(int kind, size_t n) { std::vector<uint8_t> d(n); fill(kind, d.data(), n); return d; }
static std::vector<uint8_t> mix(size_t n) {          // pieces of the kinds above, one after the other
    std::vector<uint8_t> d;
    while (d.size() < n) {
        const size_t left = n - d.size(), want = 1 + rnd() % 3000, take = want < left ? want : left;
        const std::vector<uint8_t> p = make((int)(rnd() % N_KINDS), take);
        if (rnd() % 4 == 0 && d.size() > 8) { const size_t from = rnd() % (d.size() - 4); for (size_t i = 0; i < take; ++i) d.push_back(d[from + i % (d.size() - from)]); }
        else d.insert(d.end(), p.begin(), p.end());
    }
    d.resize(n);
    return d;
}

// every token of the parse obeys the format's limits
struct LimitSink {
    uint32_t n, at;
    void lit(uint8_t) { ++at; }
    void match(uint32_t len, uint32_t dist, const uint8_t*) {
        CHECK(len >= 4 && len <= 258, "match length %u", len);
        CHECK(dist >= 1 && dist <= 32768 && dist <= at, "distance %u at %u", dist, at);
        CHECK(at + len <= n, "a match runs past the input's end (%u + %u > %u)", at, len, n);
        at += len;
    }
};

#ifndef LSD_TEST_HB
#define LSD_TEST_HB 7      // the device's default table: 128 entries
#endif
constexpr int HB = LSD_TEST_HB;
struct Lanes {          // the tables of `lanes` encoders, interleaved [index][lane]
    int lanes; std::vector<uint16_t> hash, work;
    explicit Lanes(int l) : lanes(l), hash((size_t)(1 << HB) * l, 0xabcd), work((size_t)lsd::W_WORDS * l, 0xabcd) {}
    lsd::Work of(int lane) { return lsd::Work{hash.data() + lane, lanes, work.data() + lane, lanes}; }
    // after a run of lane `used`: every word of every OTHER lane still holds the pattern (an access that forgot the stride stays inside
    // the buffers, where no sanitizer sees it); the used lane gets the pattern back
    void others_untouched(int used) {
        for (size_t i = 0; i < hash.size(); ++i) { if ((int)(i % (size_t)lanes) != used) CHECK(hash[i] == 0xabcd, "lane %d wrote hash word %zu of lane %d", used, i / (size_t)lanes, (int)(i % (size_t)lanes)); else hash[i] = 0xabcd; }
        for (size_t i = 0; i < work.size(); ++i) { if ((int)(i % (size_t)lanes) != used) CHECK(work[i] == 0xabcd, "lane %d wrote work word %zu of lane %d", used, i / (size_t)lanes, (int)(i % (size_t)lanes)); else work[i] = 0xabcd; }
    }
};
static long n_streams = 0, n_stored = 0;

// returns the stream's size
static uint32_t check(const std::vector<uint8_t>& src, lsd::Work w, int mode = lsd::MODE_AUTO) {
    const uint32_t n = (uint32_t)src.size();
    const uint32_t cap = mode == lsd::MODE_AUTO ? n + 5 : n * 2 + 600;
    std::vector<uint8_t> in(src);                      // a buffer of exactly n bytes: reads past the input are seen
    std::vector<uint8_t> out(cap);
    const uint32_t z = lsd::deflate_block<HB>(in.data(), n, out.data(), cap, w, mode);
    CHECK(z >= 2 && z <= cap, "n %u mode %d: %u bytes", n, mode, z);
    if (mode == lsd::MODE_AUTO) { CHECK(z <= n + 5, "n %u: %u bytes, more than stored", n, z); if ((out[0] & 6) == 0) ++n_stored; }
    z_stream zs; memset(&zs, 0, sizeof(zs));
    CHECK(inflateInit2(&zs, -15) == Z_OK, "inflateInit2");
    std::vector<uint8_t> back(n + 16);
    zs.next_in = out.data(); zs.avail_in = z; zs.next_out = back.data(); zs.avail_out = (uInt)back.size();
    const int rc = inflate(&zs, Z_FINISH);
    CHECK(rc == Z_STREAM_END, "n %u mode %d: zlib's inflate returns %d (%s)", n, mode, rc, zs.msg ? zs.msg : "");
    CHECK(zs.total_out == n && zs.avail_in == 0, "n %u mode %d: total_out %lu, %u bytes of the stream unread", n, mode, (unsigned long)zs.total_out, zs.avail_in);
    inflateEnd(&zs);
    CHECK(n == 0 || memcmp(back.data(), src.data(), n) == 0, "n %u mode %d: other bytes", n, mode);
    // the device's decoder reads it too (what lsg_load_bam will meet)
    std::vector<uint8_t> tab(lsi::T_SYM), lens(lsi::T_LENS), back2(n ? n : 1);
    const int ri = lsi::inflate_raw(out.data(), z, back2.data(), n, lsi::Tab{tab.data(), lens.data(), 1});
    CHECK(ri == 0 && (n == 0 || memcmp(back2.data(), src.data(), n) == 0), "n %u mode %d: inflate_core returns %d", n, mode, ri);
    LimitSink ls{n, 0};
    lsd::parse<HB>(in.data(), n, w, ls);
    CHECK(ls.at == n, "the parse covers %u of %u bytes", ls.at, n);
    ++n_streams;
    return z;
}

static void bam_blocks(const char* path, std::vector<std::vector<uint8_t>>& blocks) {
    FILE* f = fopen(path, "rb");
    CHECK(f, "cannot read %s", path);
    std::vector<uint8_t> file;
    uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + k);
    fclose(f);
    size_t p = 0;
    while (p + 28 <= file.size()) {
        CHECK(file[p] == 31 && file[p + 1] == 139 && file[p + 12] == 'B' && file[p + 13] == 'C', "%s: no BGZF block at %zu", path, p);
        const size_t bsize = (size_t)(file[p + 16] | (file[p + 17] << 8)) + 1;
        CHECK(p + bsize <= file.size(), "%s: cut block", path);
        const uint32_t isize = (uint32_t)file[p + bsize - 4] | ((uint32_t)file[p + bsize - 3] << 8) | ((uint32_t)file[p + bsize - 2] << 16) | ((uint32_t)file[p + bsize - 1] << 24);
        std::vector<uint8_t> u(isize + 1);
        z_stream zs; memset(&zs, 0, sizeof(zs));
        CHECK(inflateInit2(&zs, -15) == Z_OK, "inflateInit2");
        zs.next_in = file.data() + p + 18; zs.avail_in = (uInt)(bsize - 26); zs.next_out = u.data(); zs.avail_out = isize + 1;
        CHECK(inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.total_out == isize, "%s: block at %zu", path, p);
        inflateEnd(&zs);
        u.resize(isize);
        // (a foreign writer's block may hold up to 65 536 bytes: cut to what a BGZF writer of ours compresses at once)
        for (size_t a = 0; a < u.size() || a == 0; a += lsd::MAX_IN) { blocks.emplace_back(u.begin() + (long)a, u.begin() + (long)(a + lsd::MAX_IN < u.size() ? a + lsd::MAX_IN : u.size())); if (u.empty()) break; }
        p += bsize;
    }
}

int main(int argc, char** argv) {
    Lanes one(1), wave(64);
    int lane = 0;
    auto both = [&](const std::vector<uint8_t>& d, int mode = lsd::MODE_AUTO) {
        const uint32_t a = check(d, one.of(0), mode);
        const uint32_t b = check(d, wave.of(lane), mode);
        wave.others_untouched(lane);
        lane = (lane + 1) % 64;
        CHECK(a == b, "stride 1 gives %u bytes, stride 64 gives %u", a, b);
        return a;
    };
    // every small size, every content, the automatic choice and both coded forms forced (their headers: no distance code, one
    // distance code, one literal, the empty block)
    for (uint32_t n = 0; n <= 300; ++n)
        for (int kind = 0; kind < N_KINDS; ++kind) {
            const std::vector<uint8_t> d = make(kind, n);
            both(d); both(d, lsd::MODE_LZ); both(d, lsd::MODE_LITERALS);
        }
    { std::vector<uint8_t> d(5, 7); d.insert(d.end(), 5, 7); both(d, lsd::MODE_LZ); }          // one literal, one match, one distance code
    const uint32_t big[] = {32767, 32768, 32769, 0xfeff, 0xff00};
    for (uint32_t n : big)
        for (int kind = 0; kind < N_KINDS; ++kind) {
            const std::vector<uint8_t> d = make(kind, n);
            const long stored_before = n_stored;
            const uint32_t z = both(d);
            if (kind == RANDOM) CHECK(n_stored == stored_before + 2 && z == n + 5, "random bytes are not stored (%u -> %u)", n, z);
            if (kind == FAR_REPEAT) CHECK(z == n + 5, "the repeat beyond the window was coded (%u -> %u)", n, z);
            if (n == 0xff00 && kind == FOUR_VALUES) { printf("four values: %u -> %u (%.4f n)\n", n, z, (double)z / n); CHECK(z * 100ull <= 40ull * n, "four byte values: %u bytes > 0.40 n", z); }
            if (n == 0xff00 && kind == STRING64) { printf("64-byte string repeated: %u -> %u (%.4f n)\n", n, z, (double)z / n); CHECK(z * 100ull <= 10ull * n, "a repeated string: %u bytes > 0.10 n", z); }
            if (n == 0xff00 && (kind == ONE_BYTE || kind == PERIOD3)) CHECK(z * 100ull <= 2ull * n, "kind %d: %u bytes", kind, z);
        }
    for (int i = 0; i < 2000; ++i) {
        rng_state = 0x51ed270b1ull * (uint64_t)(i + 1) + 12345;                    // every mix from its own seed
        const uint32_t n = (i % 8 == 0) ? rnd() % (lsd::MAX_IN + 1) : rnd() % 2500;
        both(mix(n));
    }
    long n_bam = 0;
    for (int a = 1; a < argc; ++a) {
        std::vector<std::vector<uint8_t>> blocks;
        bam_blocks(argv[a], blocks);
        size_t in = 0, out = 0;
        for (const auto& b : blocks) { in += b.size(); out += both(b); ++n_bam; }
        printf("%s: %zu blocks, %zu -> %zu bytes\n", argv[a], blocks.size(), in, out);
    }
    printf("deflate ok: %ld streams (%ld stored), %ld BAM blocks\n", n_streams, n_stored, n_bam);
    return 0;
}
