// Raw DEFLATE (RFC 1951) ENCODER of ONE BGZF block (<= 0xff00 bytes) by ONE thread, the twin of inflate_core.h and written like it for a
// GPU lane: no recursion, no allocation, every loop bounded by the input size or a table size, tables in caller-provided storage
// addressed with a stride (device: [index][lane], stride 64 - the hash table in LDS, the rest in global memory; host tests: stride 1).
//
// This is the write half of a BAM (the reference writes its split BAMs through pysam / htslib's bgzf + zlib, SplitBamCellTypes.py:57-63,
// 172); csrc/split.hip runs it a lane per block.  One complete stream with the final bit set comes out, in the smallest of three forms:
//   LZ77 + dynamic Huffman  greedy parse, matches of 4..258 bytes found through a hash table of the last position of each 4-byte
//                           string; a candidate is verified byte by byte (a stale or colliding entry costs nothing), must lie behind
//                           the position and at most 32 768 back (a 0xff00-byte block is longer than the window)
//   dynamic Huffman only    every byte a literal (what wins on a few byte values drawn at random, where short matches cost more than
//                           the literals they replace)
//   stored                  when neither is smaller than n + 5 bytes
// No token buffer: the same deterministic parse runs twice, once into the frequency counts and once into the bit writer (a token buffer
// per lane would be 2-4 bytes per input byte of global memory written and read back; the second parse reads the input again, which
// the cache still holds, and the hash table in LDS).  The sizes are computed exactly from the counts before anything is written, so
// the choice is made first and the writer never passes n + 5 bytes.
// Code lengths: Moffat & Katajainen's in-place minimum-redundancy lengths over the symbols sorted by count, limited to 15 (7 for the
// code-length code) by moving codes down the length histogram until Kraft's sum is exact.  Every code has at least two symbols (as
// zlib's: a lone or missing distance code gets unused companions of one bit), so every code in the header is complete.
// tests/native/test_deflate.cpp compiles this for the host and checks every stream against zlib's inflate.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifdef __HIPCC__
#define LSD_FN __host__ __device__ __forceinline__
#else
#define LSD_FN inline
#endif

namespace lsd {

constexpr uint32_t MAX_IN = 0xff00, WINDOW = 32768, MIN_MATCH = 4, MAX_MATCH = 258;
constexpr int NL = 286, ND = 30, NC = 19, NSET = NL + ND;
// the work area: 16-bit words, every one at [index * stride]
//   W_LZ   counts of the LZ77 parse (286 lit/len + 30 distance)       W_LIT  the same for the literals-only form
//   W_LEN  code lengths of the form planned last                       W_CODE their codes, bit-reversed (DEFLATE sends codes MSB first)
//   W_ORD / W_A  the used symbols sorted by count / Moffat-Katajainen's array      W_CF / W_CL / W_CC  the code-length code
constexpr int W_LZ = 0, W_LIT = W_LZ + NSET, W_LEN = W_LIT + NSET, W_CODE = W_LEN + NSET, W_ORD = W_CODE + NSET, W_A = W_ORD + NL,
              W_CF = W_A + NL, W_CL = W_CF + NC, W_CC = W_CL + NC, W_WORDS = W_CC + NC;
enum { MODE_AUTO = 0, MODE_LZ = 1, MODE_LITERALS = 2 };      // the forced forms are for tests (the caller then gives room for them)

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

struct Work {
    uint16_t* hash; int hstride;          // 1 << HB entries: the last position at which a 4-byte string with this hash began
    uint16_t* w; int stride;              // W_WORDS words
    LSD_FN uint32_t h(uint32_t i) const { return hash[(size_t)i * hstride]; }
    LSD_FN void set_h(uint32_t i, uint32_t v) const { hash[(size_t)i * hstride] = (uint16_t)v; }
    LSD_FN uint32_t get(int i) const { return w[(size_t)i * stride]; }
    LSD_FN void set(int i, uint32_t v) const { w[(size_t)i * stride] = (uint16_t)v; }
    LSD_FN void inc(int i) const { uint16_t* p = w + (size_t)i * stride; *p = (uint16_t)(*p + 1u); }
};

LSD_FN uint32_t rd32(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const u32_unaligned*>(p);
#else
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
#endif
}
LSD_FN uint32_t brev(uint32_t v, int n) {       // the low n bits of v, reversed
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return n ? v >> (32 - n) : 0u;
}

// length 3..258 -> its symbol - 257, the number of extra bits and their value; distance 1..32768 likewise (RFC 1951 3.2.5)
LSD_FN void len_code(uint32_t len, uint32_t* sym, uint32_t* nx, uint32_t* x) {
    const uint32_t l = len - 3u;
    if (len == 258u) { *sym = 28; *nx = 0; *x = 0; return; }
    if (l < 8u) { *sym = l; *nx = 0; *x = 0; return; }
    const uint32_t k = 31u - (uint32_t)__builtin_clz(l);
    *sym = 4u * (k - 1u) + ((l >> (k - 2u)) & 3u); *nx = k - 2u; *x = l & ((1u << (k - 2u)) - 1u);
}
LSD_FN void dist_code(uint32_t dist, uint32_t* sym, uint32_t* nx, uint32_t* x) {
    const uint32_t d = dist - 1u;
    if (d < 2u) { *sym = d; *nx = 0; *x = 0; return; }
    const uint32_t k = 31u - (uint32_t)__builtin_clz(d);
    *sym = 2u * k + ((d >> (k - 1u)) & 1u); *nx = k - 1u; *x = d & ((1u << (k - 1u)) - 1u);
}
LSD_FN uint32_t len_extra(int s) { return s < 8 || s == 28 ? 0u : (uint32_t)(s - 4) >> 2; }       // extra bits of length symbol 257 + s
LSD_FN uint32_t dist_extra(int s) { return s < 2 ? 0u : (uint32_t)(s - 2) >> 1; }

// ---- the bit writer: LSB first, four bytes a store, never past `cap`
struct BitOut {
    uint8_t* out; uint32_t cap, pos; uint64_t acc; int cnt; int over;
    LSD_FN void put(uint32_t v, int n) {          // n <= 28, cnt < 32 on entry
        acc |= (uint64_t)v << cnt; cnt += n;
        if (cnt >= 32) {
            if (pos + 4u <= cap) {
                const uint32_t x = (uint32_t)acc;
#ifdef __HIP_DEVICE_COMPILE__
                *reinterpret_cast<u32_unaligned*>(out + pos) = x;
#else
                out[pos] = (uint8_t)x; out[pos + 1] = (uint8_t)(x >> 8); out[pos + 2] = (uint8_t)(x >> 16); out[pos + 3] = (uint8_t)(x >> 24);
#endif
            } else over = 1;
            pos += 4u; acc >>= 32; cnt -= 32;
        }
    }
    LSD_FN uint32_t finish() {                    // to the byte boundary; the bytes written (0: they did not fit)
        while (cnt > 0) { if (pos < cap) out[pos] = (uint8_t)acc; else over = 1; ++pos; acc >>= 8; cnt -= 8; }
        return over ? 0u : pos;
    }
};

// ---- the parse.  Sink: lit(byte), match(len, dist, the matched bytes).  The table is cleared first, so two runs make the same choices.
template <int HB, class Sink>
LSD_FN void parse(const uint8_t* in, uint32_t n, const Work& w, Sink& s) {
    for (uint32_t e = 0; e < (1u << HB); ++e) w.set_h(e, 0xffffu);              // no position is 0xffff (n <= 0xff00)
    uint32_t i = 0;
    while (i < n) {
        uint32_t len = 0, dist = 0;
        if (i + MIN_MATCH <= n) {
            const uint32_t hsh = (rd32(in + i) * 2654435761u) >> (32 - HB);
            const uint32_t c = w.h(hsh);
            w.set_h(hsh, i);
            if (c < i && i - c <= WINDOW) {
                const uint32_t room = n - i, mx = room < MAX_MATCH ? room : MAX_MATCH;         // a match ends where the input does
                while (len < mx && in[c + len] == in[i + len]) ++len;
                dist = i - c;
            }
        }
        if (len >= MIN_MATCH) { s.match(len, dist, in + i); i += len; }
        else { s.lit(in[i]); ++i; }
    }
}
struct CountSink {
    Work w;
    LSD_FN void lit(uint8_t b) const { w.inc(W_LZ + b); }
    LSD_FN void match(uint32_t len, uint32_t dist, const uint8_t* p) const {
        uint32_t s, nx, x;
        len_code(len, &s, &nx, &x); w.inc(W_LZ + 257 + (int)s);
        dist_code(dist, &s, &nx, &x); w.inc(W_LZ + NL + (int)s);
        for (uint32_t k = 0; k < len; ++k) w.inc(W_LIT + p[k]);                // what the literals-only form would code here
    }
};
struct EmitSink {
    Work w; BitOut* b;
    LSD_FN void sym(int at) const { b->put(w.get(W_CODE + at), (int)w.get(W_LEN + at)); }
    LSD_FN void lit(uint8_t v) const { sym(v); }
    LSD_FN void match(uint32_t len, uint32_t dist, const uint8_t*) const {
        uint32_t s, nx, x;
        len_code(len, &s, &nx, &x);
        b->put(w.get(W_CODE + 257 + (int)s) | (x << w.get(W_LEN + 257 + (int)s)), (int)(w.get(W_LEN + 257 + (int)s) + nx));
        dist_code(dist, &s, &nx, &x);
        b->put(w.get(W_CODE + NL + (int)s) | (x << w.get(W_LEN + NL + (int)s)), (int)(w.get(W_LEN + NL + (int)s) + nx));
    }
};

// ---- code lengths of the n symbols whose counts are at `freq`, into `len` (0: unused), none above maxbits.  Fewer than two used symbols
// get unused companions (count 0, one bit), so the code is always complete.
LSD_FN void build_lengths(const Work& w, int freq, int n, int maxbits, int len) {
    int m = 0;
    for (int s = 0; s < n; ++s) { w.set(len + s, 0); if (w.get(freq + s)) { w.set(W_ORD + m, (uint32_t)s); ++m; } }
    if (m < 2) {
        const int only = m ? (int)w.get(W_ORD) : -1;
        for (int s = 0; s < 2; ++s) w.set(len + s, 1);
        if (only > 1) { w.set(len + 1, 0); w.set(len + only, 1); }
        return;
    }
    // shell sort by (count, symbol), ascending
    const int gaps[6] = {132, 57, 23, 10, 4, 1};
    for (int g = 0; g < 6; ++g) {
        const int gap = gaps[g];
        for (int i = gap; i < m; ++i) {
            const uint32_t s = w.get(W_ORD + i), f = w.get(freq + (int)s);
            int j = i;
            for (; j >= gap; j -= gap) {
                const uint32_t t = w.get(W_ORD + j - gap), ft = w.get(freq + (int)t);
                if (ft < f || (ft == f && t < s)) break;
                w.set(W_ORD + j, t);
            }
            w.set(W_ORD + j, s);
        }
    }
    // Moffat & Katajainen, "In-place calculation of minimum-redundancy codes" (1995): counts -> parents -> depths -> leaf depths
    for (int i = 0; i < m; ++i) w.set(W_A + i, w.get(freq + (int)w.get(W_ORD + i)));
    w.set(W_A, w.get(W_A) + w.get(W_A + 1));
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; ++next) {
        uint32_t v;
        if (leaf >= m || w.get(W_A + root) < w.get(W_A + leaf)) { v = w.get(W_A + root); w.set(W_A + root, (uint32_t)next); ++root; }
        else { v = w.get(W_A + leaf); ++leaf; }
        if (leaf >= m || (root < next && w.get(W_A + root) < w.get(W_A + leaf))) { v += w.get(W_A + root); w.set(W_A + root, (uint32_t)next); ++root; }
        else { v += w.get(W_A + leaf); ++leaf; }
        w.set(W_A + next, v);                    // at most the input's length + 3: a 16-bit word holds it
    }
    w.set(W_A + m - 2, 0);
    for (int next = m - 3; next >= 0; --next) w.set(W_A + next, w.get(W_A + (int)w.get(W_A + next)) + 1u);
    {
        int avbl = 1, used = 0, dpth = 0, next = m - 1;
        root = m - 2;
        while (avbl > 0 && next >= 0) {
            while (root >= 0 && (int)w.get(W_A + root) == dpth) { ++used; --root; }
            while (avbl > used && next >= 0) { w.set(W_A + next, (uint32_t)dpth); --next; --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
    }
    // the limit: codes per length, the over-long ones at maxbits; one code leaves maxbits and one shorter code takes a bit more (its
    // place holds both) until Kraft's sum is 1 again - each turn lowers the sum by one unit of 2^-maxbits
    int nc[16];
    for (int l = 0; l < 16; ++l) nc[l] = 0;
    for (int i = 0; i < m; ++i) { const int l = (int)w.get(W_A + i); ++nc[l > maxbits ? maxbits : l]; }
    uint32_t total = 0;
    for (int l = 1; l <= maxbits; ++l) total += (uint32_t)nc[l] << (maxbits - l);
    for (int turn = 0; turn < m && total > (1u << maxbits); ++turn) {
        --nc[maxbits];
        for (int l = maxbits - 1; l > 0; --l) if (nc[l]) { --nc[l]; nc[l + 1] += 2; break; }
        --total;
    }
    // the sorted symbols take the lengths, the rarest the longest
    int i = 0;
    for (int l = maxbits; l >= 1; --l) for (int k = 0; k < nc[l] && i < m; ++k, ++i) w.set(len + (int)w.get(W_ORD + i), (uint32_t)l);
}
// canonical codes of the lengths at `len`, bit-reversed, into `code`
LSD_FN void assign_codes(const Work& w, int len, int n, int code) {
    int cnt[16], nxt[16];
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int s = 0; s < n; ++s) ++cnt[w.get(len + s)];
    cnt[0] = 0; nxt[0] = 0;
    int c = 0;
    for (int l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; nxt[l] = c; }
    for (int s = 0; s < n; ++s) { const int l = (int)w.get(len + s); if (l) { w.set(code + s, brev((uint32_t)nxt[l], l)); ++nxt[l]; } else w.set(code + s, 0); }
}

// the run-length form of the hlit + hdist code lengths (RFC 1951 3.2.7), as zlib's scan_tree / send_tree cut the runs.
// Sink: cl(symbol, extra bits, their value)
template <class Sink>
LSD_FN void rle_lengths(const Work& w, int hlit, int hdist, Sink& s) {
    const int n = hlit + hdist;
    auto at = [&](int i) -> int { return (int)w.get(i < hlit ? W_LEN + i : W_LEN + NL + (i - hlit)); };
    int i = 0;
    while (i < n) {
        const int v = at(i);
        int run = 1;
        while (i + run < n && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; s.cl(18, 7, (uint32_t)(r - 11)); run -= r; }
            if (run >= 3) { s.cl(17, 3, (uint32_t)(run - 3)); run = 0; }
        } else {
            s.cl(v, 0, 0); --run;
            while (run >= 3) { const int r = run < 6 ? run : 6; s.cl(16, 2, (uint32_t)(r - 3)); run -= r; }
        }
        for (; run > 0; --run) s.cl(v, 0, 0);
    }
}
struct ClCount { Work w; LSD_FN void cl(int sym, int, uint32_t) const { w.inc(W_CF + sym); } };
struct ClEmit { Work w; BitOut* b; LSD_FN void cl(int sym, int nx, uint32_t x) const { b->put(w.get(W_CC + sym) | (x << w.get(W_CL + sym)), (int)w.get(W_CL + sym) + nx); } };

struct Plan { uint32_t bits; int hlit, hdist, hclen; };
LSD_FN int cl_order(int i) { const uint8_t o[NC] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}; return o[i]; }

// lengths and codes of the counts at `set` (its end-of-block count set here), the header's three sizes, the block's exact bits
LSD_FN Plan plan(const Work& w, int set) {
    w.set(set + 256, 1);
    build_lengths(w, set, NL, 15, W_LEN);
    build_lengths(w, set + NL, ND, 15, W_LEN + NL);
    Plan p; p.bits = 3 + 5 + 5 + 4;
    for (int s = 0; s < NL; ++s) p.bits += w.get(set + s) * (w.get(W_LEN + s) + (s > 256 ? len_extra(s - 257) : 0u));
    for (int s = 0; s < ND; ++s) p.bits += w.get(set + NL + s) * (w.get(W_LEN + NL + s) + dist_extra(s));
    p.hlit = NL; while (p.hlit > 257 && !w.get(W_LEN + p.hlit - 1)) --p.hlit;
    p.hdist = ND; while (p.hdist > 1 && !w.get(W_LEN + NL + p.hdist - 1)) --p.hdist;
    for (int s = 0; s < NC; ++s) w.set(W_CF + s, 0);
    ClCount cc{w};
    rle_lengths(w, p.hlit, p.hdist, cc);
    build_lengths(w, W_CF, NC, 7, W_CL);
    p.hclen = NC; while (p.hclen > 4 && !w.get(W_CL + cl_order(p.hclen - 1))) --p.hclen;
    p.bits += 3u * (uint32_t)p.hclen;
    for (int s = 0; s < NC; ++s) p.bits += w.get(W_CF + s) * (w.get(W_CL + s) + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
    return p;
}

// in[0, n) -> one raw DEFLATE stream at out; returns its bytes (at most n + 5 in MODE_AUTO, for which cap >= n + 5), 0 when cap is too small
template <int HB>
LSD_FN uint32_t deflate_block(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, const Work& w, int mode = MODE_AUTO) {
    if (n > MAX_IN) return 0;
    for (int i = 0; i < W_LEN; ++i) w.set(i, 0);
    CountSink cs{w};
    parse<HB>(in, n, w, cs);
    for (int b = 0; b < 256; ++b) w.set(W_LIT + b, w.get(W_LIT + b) + w.get(W_LZ + b));
    const Plan plit = plan(w, W_LIT);
    Plan p = plan(w, W_LZ);                                  // (its lengths are the ones in place now)
    bool lz = true;
    if (mode == MODE_LITERALS || (mode == MODE_AUTO && plit.bits < p.bits)) { lz = false; p = plan(w, W_LIT); }
    const uint32_t coded = (p.bits + 7u) >> 3;
    if (mode == MODE_AUTO && coded >= n + 5u) {              // stored
        if (cap < n + 5u) return 0;
        out[0] = 1; out[1] = (uint8_t)n; out[2] = (uint8_t)(n >> 8); out[3] = (uint8_t)~n; out[4] = (uint8_t)(~n >> 8);
        for (uint32_t i = 0; i < n; ++i) out[5 + i] = in[i];
        return n + 5u;
    }
    assign_codes(w, W_LEN, NL, W_CODE);
    assign_codes(w, W_LEN + NL, ND, W_CODE + NL);
    assign_codes(w, W_CL, NC, W_CC);
    BitOut b{out, cap, 0, 0, 0, 0};
    b.put(1, 1); b.put(2, 2);
    b.put((uint32_t)(p.hlit - 257), 5); b.put((uint32_t)(p.hdist - 1), 5); b.put((uint32_t)(p.hclen - 4), 4);
    for (int i = 0; i < p.hclen; ++i) b.put(w.get(W_CL + cl_order(i)), 3);
    ClEmit ce{w, &b};
    rle_lengths(w, p.hlit, p.hdist, ce);
    EmitSink es{w, &b};
    if (lz) parse<HB>(in, n, w, es);
    else for (uint32_t i = 0; i < n; ++i) es.lit(in[i]);
    es.sym(256);
    return b.finish();
}

} // namespace lsd
