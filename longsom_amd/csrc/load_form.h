// The form of a load (store.hip build_store), decided in one place: what an attempt wants before its early look at the device, what it
// settles on after it - or the lower rung to start again on - and the predicates about read filters and references that the load and the
// counts share.  Plain host C++ (no HIP): tests/native/test_load_form.cpp walks the whole table.
#pragma once
#include <cstdint>

namespace lsg {

// lsg_get_layout_info's `path` of a load.  The context keeps the last load's; a handle that has loaded nothing reads LOAD_STORE.
enum LoadForm {
    LOAD_STORE = 2,        // the store is written, counted on request
    LOAD_FUSED = 3,        // the store is written by the pass that makes the first count (lsg_set_count_at_load)
    LOAD_DIRECT = 4,       // no store (lsg_set_store_policy): the count from the caller's events, an entry through a descriptor of its own bytes
    LOAD_LINES = 5,        // ... tile-phased events: one 128-byte line per entry
    LOAD_WINDOWS = 6,      // ... entries binned by 128-position windows, one 256-byte block per entry
};
inline bool keeps_store(LoadForm f) { return f == LOAD_STORE || f == LOAD_FUSED; }
inline bool bins_windows(LoadForm f) { return f == LOAD_WINDOWS; }
inline int bin_shift(LoadForm f) { return bins_windows(f) ? 1 : 0; }      // tiles per bin = 1 << bin_shift (the kernels' wsh)

// The forms of a load, leanest first.  A load that cannot keep the form it was started in returns the rung to start again on
// (build_store), always a lower one: windows and keys alone, tiles and keys alone, tiles and values.
enum LoadRung { RUNG_WINDOWS = 1, RUNG_TILE_KEYS, RUNG_TILE_VALUES };

// ---- read filters: a store holds the reads that passed the load's; a count has its own
struct ReadFilter { int32_t min_mq; uint32_t flag_exclude; int32_t ignore_orphans; };
// the count admits no read the load dropped (else it is refused: lsg_api.hip check_load_filter)
inline bool count_within_load_filter(const ReadFilter& count, const ReadFilter& load) {
    return !(count.min_mq < load.min_mq || (load.flag_exclude & ~count.flag_exclude) != 0 || (load.ignore_orphans && !count.ignore_orphans));
}
// the count admits every read the load kept (no admission bit per read is needed: pileup.hip fill_args); with the above: the same reads
inline bool count_admits_every_stored_read(const ReadFilter& count, const ReadFilter& load) {
    return count.min_mq <= load.min_mq && (count.flag_exclude & ~load.flag_exclude) == 0 && (!count.ignore_orphans || load.ignore_orphans);
}
// every contig's reference is loaded; else the first one that is not
inline int first_missing_reference(const uint8_t* const* ref_ptr, int n_contigs) { for (int t = 0; t < n_contigs; ++t) if (!ref_ptr[t]) return t; return -1; }
inline bool references_loaded(const uint8_t* const* ref_ptr, int n_contigs) { return first_missing_reference(ref_ptr, n_contigs) < 0; }

// ---- the facts the decision reads
constexpr uint32_t LOOK_BAD_EVENTS = 1u, LOOK_BAD_READ = 2u, LOOK_UNPHASED = 4u;      // k_seg_static's `bad` bits
struct LoadFacts {
    int rung;                                   // the attempt's (LoadRung)
    // known before the early look
    bool cal_enabled, skip_policy;              // lsg_set_count_at_load; lsg_set_store_policy is LSG_STORE_SKIP_WHEN_COUNTED
    int32_t n_ct, n_cb; bool copy_stream;
    int64_t n_events;
    bool says_phased;                           // lsg_set_events_layout says LSG_LAYOUT_PHASED, or this library's producer laid out this very array
    uintptr_t events_addr;
    int32_t plp_window, min_bq;                 // (min_bq: the count's)
    uint32_t n_tiles;
    ReadFilter load_filter, count_filter;
    bool refs_loaded;
    // from the early look
    uint32_t bad; int bits;                     // LOOK_*; the barcode bits of the sort key
    bool cap_out;                               // the depth cap of the load's count cannot fire
    bool test_keys_only_refused;                // LSG_TEST_KEYS_ONLY_REFUSED
};

// Can the load make the count itself (lsg_set_count_at_load: at most two cell types, barcodes set, the copy stream for the plan)?  The gate
// of every form of the load that counts; each form adds conditions of its own.
inline bool count_in_load(const LoadFacts& f) { return f.cal_enabled && f.n_ct >= 1 && f.n_ct <= 2 && f.n_cb > 0 && f.copy_stream; }

// ---- what an attempt wants, before the early look
struct LoadWant { bool counts, skip_store, win; int wsh; uint32_t n_bins; };
inline LoadWant load_want(const LoadFacts& f) {
    LoadWant w{};
    // (the pass that counts takes 64 .. 2^39 events; the plan's tile-level half and the depth cap's bounds need the gate alone)
    w.counts = count_in_load(f) && f.n_events >= 64 && f.n_events < (1ll << 39);
    w.skip_store = f.cal_enabled && f.skip_policy;
    // WINDOWS.  A load that will keep no store and sort keys alone (below), over events its producer says are phased modulo 128
    // (lsg_set_events_layout; this library's own producers say so themselves), bins its entries by 128-position windows - tiles (2 w, 2 w + 1) -
    // instead of tiles: 0.58 x as many entries through the scatter and the sort, and every entry one aligned 256-byte block for the count
    // (k_tm_count_win).  Everything that is "per tile" is then per window (n_bins); the count's units stay the tiles'.  Should the early
    // look say otherwise (events not phased after all, a depth cap that could fire, ...), the load starts again by tiles (RUNG_TILE_KEYS).
    w.win = f.rung == RUNG_WINDOWS && w.skip_store && w.counts && f.n_events >= 128 && f.says_phased && (f.events_addr & 255u) == 0 && f.plp_window >= 128 &&
            f.min_bq >= 1 && f.min_bq <= 255 && (f.n_tiles & 1u) == 0;
    w.wsh = w.win ? 1 : 0;
    w.n_bins = f.n_tiles >> w.wsh;
    return w;
}

// ---- what it settles on, after the early look
// the look refutes the windows: events not phased modulo 128 after all (and otherwise sound: unsound ones are an error, not a restart)
inline bool look_refutes_windows(const LoadWant& w, uint32_t bad) { return w.win && (bad & LOOK_UNPHASED) && !(bad & (LOOK_BAD_EVENTS | LOOK_BAD_READ)); }
// tile-phased events (LSG_LAYOUT_PHASED): every entry lies inside one aligned 128-byte line of the caller's array (256 bytes for windows);
// the key carries the line, not the event (k_seg_static looked at the phase modulo the bins' width: 64, or 128 for windows)
inline int load_src_shift(const LoadFacts& f, const LoadWant& w) { return !(f.bad & LOOK_UNPHASED) && (f.events_addr & (w.wsh ? 255u : 127u)) == 0 ? 6 + w.wsh : 0; }
// the packed sort key holds a barcode, 12 (windows: 14) bits of geometry and the source: 52 bits for both ends, 50 when two flags ride along
inline bool source_fits_key(const LoadFacts& f, const LoadWant& w, int src_shift, bool with_flags) {
    return (f.n_events >> src_shift) < (1ll << ((with_flags ? 50 : 52) - f.bits - 2 * w.wsh));
}

struct LoadSettled {
    int restart;             // a LoadRung to start again on at once (then nothing else holds), or 0
    int refused;             // ... or once the scatter and the sort are done, where the count would have been refused (the test hook), or 0
    bool keys_only, fused;   // keys alone through the scatter and the sort; the load makes the count
    int src_shift;
    LoadForm form;
};
inline LoadSettled load_settle(const LoadFacts& f, const LoadWant& w) {
    LoadSettled s{};
    s.form = LOAD_STORE;
    if (look_refutes_windows(w, f.bad)) { s.restart = RUNG_TILE_KEYS; return s; }
    s.src_shift = load_src_shift(f, w);
    // what any count made by the load needs: the count would not be refused, its depth cap cannot fire, the references are there
    const bool countable = w.counts && count_within_load_filter(f.count_filter, f.load_filter) && f.cap_out && f.refs_loaded;
    // A load that is counted once, without a store, by a count that admits every stored read (the filters of the load) and whose depth cap
    // cannot fire needs nothing of an entry's value but two flags: they ride in the key (bits 62, 63, above a source field two bits
    // narrower) and the scatter, the sort and the count move 8 bytes an entry instead of 12.  Should the count not be made that way after
    // all (its rows outgrow their buffer), the load starts again with values (RUNG_TILE_VALUES).
    s.keys_only = f.rung <= RUNG_TILE_KEYS && w.skip_store && countable && source_fits_key(f, w, s.src_shift, true) &&
                  count_admits_every_stored_read(f.count_filter, f.load_filter);
    if (w.win && !s.keys_only) { s.restart = RUNG_TILE_KEYS; return s; }
    if (s.keys_only && f.test_keys_only_refused) s.refused = w.win ? RUNG_TILE_KEYS : RUNG_TILE_VALUES;      // (test hook: the way a refused count of keys alone takes)
    // The first count in the same pass (lsg_set_count_at_load): when its parameters and the barcode table are known now, the depth cap
    // cannot fire and one pass covers the cell types, the load counts: without a store from the sort's output, or in the pass that
    // writes the store (pileup.hip's k_tm_gather_count, which counts while each block is in registers).
    s.fused = countable;
    if (s.fused && w.skip_store) {
        // (an entry is fetched as its one 128-byte line when the events are tile-phased and the quality compare can read the event's low byte)
        const bool lines = s.src_shift == 6 && f.min_bq >= 1 && f.min_bq <= 255;
        s.form = w.win ? LOAD_WINDOWS : lines ? LOAD_LINES : LOAD_DIRECT;
    } else if (s.fused) s.form = LOAD_FUSED;
    return s;
}
// a count without a store whose rows outgrew their buffer: from windows start again by tiles, from keys alone with values, otherwise the
// store is written after all and counted on request
inline LoadSettled load_rows_outgrew(const LoadWant& w, LoadSettled s) {
    s.restart = w.win ? RUNG_TILE_KEYS : s.keys_only ? RUNG_TILE_VALUES : 0;
    s.fused = false; s.form = LOAD_STORE;
    return s;
}

} // namespace lsg
