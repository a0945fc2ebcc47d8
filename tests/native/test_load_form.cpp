// The decision about a load's form (csrc/load_form.h) as a table: (a) from a load that settles on windows (form 6), every single reason
// against it gives the outcome build_once gave before the decision was a function - stated by hand, beside the line of store.hip /
// pileup.hip at 4e48ae5 it came from; (b) over every combination of the facts a returned rung is strictly lower than the attempt's;
// (c) following the restarts ends where the lowest rung would have ended directly.
#include "load_form.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lsg;

static int n_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++n_failed; fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const ReadFilter LOADF = {20, 0x704u, 1};
static bool same_reads(const ReadFilter& count, const ReadFilter& load) { return count_within_load_filter(count, load) && count_admits_every_stored_read(count, load); }

static LoadFacts base() {
    LoadFacts f{};
    f.rung = RUNG_WINDOWS; f.cal_enabled = true; f.skip_policy = true; f.n_ct = 2; f.n_cb = 100; f.copy_stream = true;
    f.n_events = 1 << 20; f.says_phased = true; f.events_addr = (uintptr_t)0x7f0000000000ull; f.plp_window = 50000; f.min_bq = 20; f.n_tiles = 1000;
    f.load_filter = LOADF; f.count_filter = LOADF; f.refs_loaded = true;
    f.bad = 0; f.bits = 13; f.cap_out = true; f.test_keys_only_refused = false;
    return f;
}

struct Outcome { std::vector<int> restarts; LoadForm form; bool keys_only, fused; };
static Outcome follow(LoadFacts f) {
    Outcome o{};
    for (int attempt = 0;; ++attempt) {
        const LoadWant w = load_want(f);
        const LoadSettled s = load_settle(f, w);
        const int r = s.restart ? s.restart : s.refused;
        if (!r) { o.form = s.form; o.keys_only = s.keys_only; o.fused = s.fused; return o; }
        if (attempt >= 3 || r <= f.rung || r > RUNG_TILE_VALUES) { fprintf(stderr, "rung %d returned rung %d\n", f.rung, r); exit(2); }
        o.restarts.push_back(r);
        f.rung = r;
    }
}
static bool is(const Outcome& o, std::vector<int> restarts, LoadForm form) { return o.restarts == restarts && o.form == form; }

static void single_reasons() {
    LoadFacts f = base();
    {   const LoadWant w = load_want(f);
        CHECK(w.counts && w.skip_store && w.win && w.wsh == 1 && w.n_bins == 500, "the base case wants windows");
        const Outcome o = follow(f);
        CHECK(is(o, {}, LOAD_WINDOWS) && o.keys_only && o.fused, "the base case: form %d", (int)o.form); }
    // ---- reasons against windows that the attempt knows before its early look (store.hip:821-823, `win`): it goes by tiles, keys alone; the
    // events are phased (bad = 0, aligned), so the count fetches lines (pileup.hip:2009 `al`) - unless the threshold is no byte compare
    f = base(); f.says_phased = false;                                      // store.hip:822: neither the claim nor the producer's hint
    CHECK(is(follow(f), {}, LOAD_LINES) && follow(f).keys_only, "claim not phased and no hint");
    f = base(); f.events_addr += 128;                                       // store.hip:822: ((uintptr_t)events & 255u) == 0
    CHECK(is(follow(f), {}, LOAD_LINES), "events not 256-byte aligned");
    f = base(); f.events_addr += 64;                                        // store.hip:911: not 128-byte aligned either: src_shift 0
    CHECK(is(follow(f), {}, LOAD_DIRECT), "events not 128-byte aligned");
    f = base(); f.plp_window = 127;                                         // store.hip:822: plp_window >= 128
    CHECK(is(follow(f), {}, LOAD_LINES), "plp_window 127");
    f = base(); f.min_bq = 0;                                               // store.hip:823, pileup.hip:2009: min_bq >= 1
    CHECK(is(follow(f), {}, LOAD_DIRECT), "min_bq 0");
    f = base(); f.min_bq = 256;                                             // store.hip:823, pileup.hip:2009: min_bq <= 255
    CHECK(is(follow(f), {}, LOAD_DIRECT), "min_bq 256");
    f = base(); f.n_tiles = 1001;                                           // store.hip:823: (n_tiles & 1) == 0
    CHECK(is(follow(f), {}, LOAD_LINES) && load_want(f).n_bins == 1001, "n_tiles odd");
    // ---- reasons the windows attempt meets after its early look: it starts again by tiles (store.hip:956 `win && !keys_only`)
    f = base(); f.count_filter.min_mq = 30;                                 // store.hip:952: filters differ -> no keys alone; :1099: the count is within -> still made
    { const Outcome o = follow(f); CHECK(is(o, {RUNG_TILE_KEYS}, LOAD_LINES) && !o.keys_only && o.fused, "count within the load filter, not equal"); }
    f = base(); f.count_filter.flag_exclude |= 0x800u;
    CHECK(is(follow(f), {RUNG_TILE_KEYS}, LOAD_LINES) && !follow(f).keys_only, "count excludes more flags than the load");
    f = base(); f.count_filter.min_mq = 10;                                 // store.hip:1099: the count would be refused -> store, count on request
    { const Outcome o = follow(f); CHECK(is(o, {RUNG_TILE_KEYS}, LOAD_STORE) && !o.fused, "count outside the load filter"); }
    f = base(); f.count_filter.ignore_orphans = 0;                          // store.hip:1099: st_ignore_orphans && !q.ignore_orphans
    CHECK(is(follow(f), {RUNG_TILE_KEYS}, LOAD_STORE), "count keeps the orphans the load dropped");
    f = base(); f.cap_out = false;                                          // store.hip:953, 1100: the depth cap might fire
    CHECK(is(follow(f), {RUNG_TILE_KEYS}, LOAD_STORE), "cap_out false");
    f = base(); f.refs_loaded = false;                                      // store.hip:954, 1101: a reference is missing
    CHECK(is(follow(f), {RUNG_TILE_KEYS}, LOAD_STORE), "a reference missing");
    f = base(); f.bad = LOOK_UNPHASED;                                      // store.hip:910: the claim was wrong -> by tiles; :911 src_shift 0 -> descriptors
    { const Outcome o = follow(f); CHECK(is(o, {RUNG_TILE_KEYS}, LOAD_DIRECT) && o.keys_only, "not phased after a phased claim"); }
    f = base(); f.bad = LOOK_UNPHASED | LOOK_BAD_EVENTS;                    // store.hip:910: unsound arrays are an error (build_once), never a restart
    CHECK(!look_refutes_windows(load_want(f), f.bad), "unsound arrays do not restart");
    // ---- the load does not count at all: no windows, no keys alone, the store
    f = base(); f.skip_policy = false;                                      // store.hip:815, 1146: the store written by the pass that counts
    { const Outcome o = follow(f); CHECK(is(o, {}, LOAD_FUSED) && !o.keys_only && o.fused, "policy keep"); }
    f = base(); f.n_ct = 3;                                                 // store.hip:791 count_in_load: at most two cell types
    CHECK(is(follow(f), {}, LOAD_STORE) && !follow(f).fused, "n_ct 3");
    f = base(); f.n_events = 63;                                            // store.hip:814: the pass that counts takes 64 events and more
    CHECK(is(follow(f), {}, LOAD_STORE), "n_events 63");
    f = base(); f.n_events = 127;                                           // store.hip:821: windows take 128 and more; tiles count
    CHECK(is(follow(f), {}, LOAD_LINES), "n_events 127");
    f = base(); f.cal_enabled = false;
    CHECK(is(follow(f), {}, LOAD_STORE), "no count at load");
    // ---- the test hook (store.hip:1117): windows -> tiles, keys alone -> tiles, values -> counted from lines with values
    f = base(); f.test_keys_only_refused = true;
    { const Outcome o = follow(f); CHECK(is(o, {RUNG_TILE_KEYS, RUNG_TILE_VALUES}, LOAD_LINES) && !o.keys_only && o.fused, "the hook");
      const LoadSettled s = load_settle(f, load_want(f)); CHECK(!s.restart && s.refused == RUNG_TILE_KEYS && s.keys_only, "the hook refuses after the sort, not before"); }
    // ---- rows that outgrew their buffer (store.hip:1136-1140)
    f = base();
    { LoadWant w = load_want(f); CHECK(load_rows_outgrew(w, load_settle(f, w)).restart == RUNG_TILE_KEYS, "rows outgrew: from windows by tiles");
      f.rung = RUNG_TILE_KEYS; w = load_want(f); CHECK(load_rows_outgrew(w, load_settle(f, w)).restart == RUNG_TILE_VALUES, "rows outgrew: from keys alone with values");
      f.rung = RUNG_TILE_VALUES; w = load_want(f); const LoadSettled s = load_rows_outgrew(w, load_settle(f, w));
      CHECK(!s.restart && s.form == LOAD_STORE && !s.fused, "rows outgrew: the store, counted on request"); }
    // ---- the source field of keys alone (store.hip:933): n_events >> src_shift < 2^(50 - bits - 2 wsh)
    f = base(); f.bits = 24;
    {   f.n_events = (1ll << 24) << 7;                                      // windows: src_shift 7, 2^(50 - 24 - 2) lines of 256 bytes
        LoadWant w = load_want(f); LoadSettled s = load_settle(f, w);
        CHECK(w.win && s.restart == RUNG_TILE_KEYS, "windows, source field exactly full: by tiles");
        f.n_events -= 1; w = load_want(f); s = load_settle(f, w);
        CHECK(w.win && !s.restart && s.keys_only && s.form == LOAD_WINDOWS && s.src_shift == 7, "windows, one below: keys alone");
        f.rung = RUNG_TILE_KEYS; f.n_events = (1ll << 26) << 6;             // tiles: src_shift 6, 2^(50 - 24) lines
        w = load_want(f); s = load_settle(f, w);
        CHECK(!s.restart && !s.keys_only && s.fused && s.form == LOAD_LINES && source_fits_key(f, w, s.src_shift, false), "tiles, exactly full: with values");
        f.n_events -= 1; w = load_want(f); s = load_settle(f, w);
        CHECK(!s.restart && s.keys_only && s.form == LOAD_LINES && s.src_shift == 6, "tiles, one below: keys alone");
        f.n_events = (1ll << 28) << 6; CHECK(!source_fits_key(f, load_want(f), 6, false), "52 - bits: the key itself"); }
    // ---- the predicates
    const ReadFilter a = {20, 0x704u, 1}, stricter = {30, 0xF04u, 1}, laxer = {0, 0x4u, 0};
    CHECK(same_reads(a, a) && count_within_load_filter(stricter, a) && !count_admits_every_stored_read(stricter, a), "a stricter count is within, admits not all");
    CHECK(!count_within_load_filter(laxer, a) && count_admits_every_stored_read(laxer, a) && !same_reads(laxer, a) && !same_reads(stricter, a), "a laxer count is refused");
    const ReadFilter orph2 = {20, 0x704u, 2};
    CHECK(same_reads(orph2, a) && same_reads(a, orph2), "ignore_orphans is a truth value");
    const uint8_t x = 0; const uint8_t* refs[3] = {&x, nullptr, &x};
    CHECK(first_missing_reference(refs, 3) == 1 && !references_loaded(refs, 3) && references_loaded(refs, 1) && references_loaded(refs, 0), "references");
    CHECK(keeps_store(LOAD_STORE) && keeps_store(LOAD_FUSED) && !keeps_store(LOAD_DIRECT) && !keeps_store(LOAD_LINES) && !keeps_store(LOAD_WINDOWS), "keeps_store");
    CHECK(bin_shift(LOAD_WINDOWS) == 1 && bin_shift(LOAD_LINES) == 0 && bin_shift(LOAD_STORE) == 0, "bin_shift");
}

// (b), (c): every combination of the facts
static void exhaustive() {
    const ReadFilter counts[3] = {LOADF, {30, 0x704u, 1}, {10, 0x704u, 1}};      // the load's own, within it, outside it
    const uintptr_t addr[3] = {0x7f0000000000ull, 0x7f0000000080ull, 0x7f0000000040ull};
    const int64_t nev[5] = {63, 64, 127, 128, 1 << 20};
    const int32_t bq[3] = {0, 20, 256};
    long long n = 0, n_restarted = 0;
    for (int m = 0; m < (1 << 11); ++m)
    for (int ct = 0; ct <= 3; ++ct) for (int fi = 0; fi < 3; ++fi) for (int ai = 0; ai < 3; ++ai) for (int ei = 0; ei < 5; ++ei) for (int qi = 0; qi < 3; ++qi) {
        LoadFacts f = base();
        f.cal_enabled = m & 1; f.skip_policy = m & 2; f.copy_stream = m & 4; f.says_phased = m & 8; f.plp_window = (m & 16) ? 128 : 127; f.n_tiles = (m & 32) ? 1000 : 1001;
        f.refs_loaded = m & 64; f.bad = (m & 128) ? LOOK_UNPHASED : 0u; f.cap_out = m & 256; f.test_keys_only_refused = m & 512; f.n_cb = (m & 1024) ? 100 : 0;
        f.n_ct = ct; f.count_filter = counts[fi]; f.events_addr = addr[ai]; f.n_events = nev[ei]; f.min_bq = bq[qi];
        LoadForm tile_form[4] = {};
        for (int rung = RUNG_TILE_VALUES; rung >= RUNG_WINDOWS; --rung) {
            f.rung = rung;
            const LoadWant w = load_want(f);
            const LoadSettled s = load_settle(f, w);
            ++n;
            // (b) a returned rung is a lower one: at most three attempts
            CHECK(s.restart == 0 || (s.restart > rung && s.restart <= RUNG_TILE_VALUES), "rung %d restarts on %d", rung, s.restart);
            CHECK(s.refused == 0 || (s.refused > rung && s.refused <= RUNG_TILE_VALUES), "rung %d is refused to %d", rung, s.refused);
            CHECK(!(s.restart && s.refused), "one way out");
            const int out = load_rows_outgrew(w, s).restart;
            CHECK(s.restart || out == 0 || (out > rung && out <= RUNG_TILE_VALUES), "rung %d, rows outgrew: %d", rung, out);
            CHECK(w.win == (w.wsh == 1) && (!w.win || rung == RUNG_WINDOWS), "windows on the top rung only");
            if (s.restart) continue;
            CHECK(s.keys_only ? (s.fused && !keeps_store(s.form) && rung <= RUNG_TILE_KEYS) : !w.win, "keys alone: counted without a store; windows: keys alone");
            CHECK(s.fused == (s.form != LOAD_STORE) && (s.form == LOAD_WINDOWS) == w.win, "form %d", (int)s.form);
            tile_form[rung] = s.form;
        }
        // (c) the restarts from the top end in the form the lowest rung gives directly, whenever the higher rungs refuse
        f.rung = RUNG_WINDOWS;
        const Outcome o = follow(f);
        if (!o.restarts.empty()) { ++n_restarted; CHECK(o.form == tile_form[RUNG_TILE_VALUES], "restarts end in form %d, the lowest rung in %d", (int)o.form, (int)tile_form[RUNG_TILE_VALUES]); }
        else if (o.form != LOAD_WINDOWS) CHECK(o.form == tile_form[RUNG_TILE_VALUES], "the form of a load by tiles does not depend on the rung");
    }
    printf("%lld evaluations, %lld loads restarted\n", n, n_restarted);
}

int main() {
    single_reasons();
    exhaustive();
    if (n_failed) { fprintf(stderr, "%d checks failed\n", n_failed); return 1; }
    printf("load form ok\n");
    return 0;
}
