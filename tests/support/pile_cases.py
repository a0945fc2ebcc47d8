"""Directed piles for the count kernels' packed counters: records built by hand so that a tile, a window or a job holds EXACTLY the
number of entries at which a field of the counters is full (pileup.hip tm_add / tw_add, lsg_ctx.h TM_JOB_LIMIT, ROW_NARROW_MAX).

A pile is a stack of identical reads: every read is ONE segment of eight positions whose event at position P + k has symbol class k
(A, C, T, G, I, D, N, O) and quality 255, so position P + 7 carries symbol class 7.  Around it lie a handful of ordinary reads in the
other 128-position windows (entries that straddle tile edges exist; none touches the pile's windows, so its tiles and windows hold what
the case says and nothing else).  tests/test_count_edges_cpu.py proves every case from the records and the CPU oracle alone;
tests/test_count_edges_gpu.py counts them on the device in every form.

The barcodes: 0 and 2 belong to cell type 0 and own the long runs, 1 belongs to cell type 1 and owns the second run of a limit case
(reverse strand); 2..257 are the 256 (257) barcodes of the many-barcode tiles; 258.. carry the ordinary reads (all cell types), the
last one is in no cell type."""
import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np

from longsom_amd.engine import ReadRecords
from tests.support.synth_simple import random_records

PILE_SYMBOLS = tuple(range(8))
QMAX = 255
N_CB = 300
JOB_LIMIT = 4095            # lsg_ctx.h TM_JOB_LIMIT: entries of a job counted in the packed planes
NARROW_MAX = 256            # lsg_ctx.h ROW_NARROW_MAX: entries of a one-job tile whose rows are written as 16-bit planes
# A tile of more entries than the plan's job target is cut into J = ceil(n / 768) jobs (store.hip k_tm_tiles; 768 is the target of every
# load this small) at the first run start at or after n j / J (tm_make_job).  A long run that comes LAST in its tile therefore starts a
# job of its own only when the run before it reaches past n / J: 5 entries do not (the job would be the whole tile: 4100 entries, the
# wide walk), 768 do (n = 4863, J = 7, n / J = 694).
SECOND_RUN, SECOND_RUN_BEFORE = 5, 768


def build_records(groups, tid=0) -> ReadRecords:
    """groups: (barcode, n_reads, start, symbols, quality, reverse) - n_reads identical reads of one segment each, its events
    LSG_EVENT(symbols[i], quality) at start + i (quality: one value, or one per position).  The reads come out sorted by start."""
    groups = sorted(groups, key=lambda g: g[2])
    cb, pos, flag, ln, ev = [], [], [], [], []
    for barcode, n, start, symbols, quality, reverse in groups:
        sym = np.asarray(symbols, np.uint16)
        q = np.broadcast_to(np.asarray(quality, np.uint16), sym.shape)
        assert (sym < 8).all() and (q <= 255).all() and n >= 0 and start >= 0
        cb.append(np.full(n, barcode, np.int32)); pos.append(np.full(n, start, np.int32))
        flag.append(np.full(n, 0x10 if reverse else 0, np.uint16)); ln.append(np.full(n, len(sym), np.int32))
        ev.append(np.tile((0x0800 | (sym << 8) | q).astype(np.uint16), n))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    cb, pos, flag, ln, ev = cat(cb, np.int32), cat(pos, np.int32), cat(flag, np.uint16), cat(ln, np.int32), cat(ev, np.uint16)
    R = len(cb)
    off = (np.cumsum(ln) - ln).astype(np.int64)
    return ReadRecords(np.full(R, tid, np.int32), pos, flag, np.full(R, 60, np.uint8), cb, np.arange(R, dtype=np.uint32), pos.copy(), ln, off, ev)


def concat_records(a: ReadRecords, b: ReadRecords) -> ReadRecords:
    return ReadRecords(np.r_[a.read_tid, b.read_tid], np.r_[a.read_pos, b.read_pos], np.r_[a.read_flag, b.read_flag], np.r_[a.read_mapq, b.read_mapq],
                       np.r_[a.read_cb, b.read_cb], np.r_[a.seg_read, b.seg_read + np.uint32(a.n_reads)], np.r_[a.seg_start, b.seg_start],
                       np.r_[a.seg_len, b.seg_len], np.r_[a.seg_ev_off, b.seg_ev_off + a.n_events], np.r_[a.events, b.events])


def entries_per_bin(rec: ReadRecords, width: int) -> Dict[Tuple[int, int], int]:
    """the store's entries - (segment x bin) of every read that carries a barcode - per (contig, bin) of `width` positions: 64 = tiles,
    128 = the windows of a load that kept no store"""
    out: Dict[Tuple[int, int], int] = {}
    for s in range(rec.n_segs):
        r = int(rec.seg_read[s])
        if rec.read_cb[r] < 0:
            continue
        st, ln = int(rec.seg_start[s]), int(rec.seg_len[s])
        for b in range(st // width, (st + ln - 1) // width + 1):
            out[(int(rec.read_tid[r]), b)] = out.get((int(rec.read_tid[r]), b), 0) + 1
    return out


def neighbours(seed, lens, keep_out, n_draw=160) -> ReadRecords:
    """ordinary reads (qualities 2..60, all flags) none of whose segments touches a 128-position window of contig 0 listed in keep_out"""
    rec = random_records(seed, n_draw, lens, N_CB - 258, max_exons=3, exon_len=(20, 90), intron_len=(5, 40))
    bad = np.zeros(rec.n_reads, bool)
    for s in range(rec.n_segs):
        r = int(rec.seg_read[s])
        if rec.read_tid[r] == 0:
            st, ln = int(rec.seg_start[s]), int(rec.seg_len[s])
            if any(w in keep_out for w in range(st // 128, (st + ln - 1) // 128 + 1)):
                bad[r] = True
    rec = rec.subset(~bad)
    rec.read_cb[rec.read_cb >= 0] += 258
    return rec


def celltypes(n_ct: int) -> np.ndarray:
    ct_of = (np.arange(N_CB) % n_ct).astype(np.uint8)
    ct_of[:258] = 0
    ct_of[1] = 1
    ct_of[N_CB - 1] = 255
    return ct_of


@dataclasses.dataclass
class PileCase:
    name: str
    lens: List[int]
    rec: ReadRecords
    refs: List[np.ndarray]
    piles: List[Tuple[int, int, int, int]]      # (start P, reads, distinct barcodes, cell type) of the runs of cell type 0 / 1, all forward / all reverse
    tiles: Dict[int, int]                       # entries the case claims per tile of contig 0 (the pile's tiles)
    windows: Dict[int, int]                     # ... and per 128-position window
    kind: str                                   # "narrow", "wide", "limit", "past"
    plan: Optional[Tuple[Tuple[int, ...], int]] = None      # limit / past: (numbers of wide jobs a plan may report, longest packed job: exact for "limit", at most for "past")

    def celltype_of(self, n_ct=2):
        return celltypes(n_ct)


LENS = [637, 130]           # contig 0: ten tiles, the last one cut short; five windows


def _refs(P_list):
    """references without N (every pile position makes a row); at P + k: C C A G T T T T against the pile's A C T G I D N O, so P and
    P + 2 are alternative alleles for the call stage and P + 1, P + 3 are the reference"""
    rng = np.random.default_rng(4242)
    refs = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L) for L in LENS]
    for P in P_list:
        refs[0][P:P + 8] = np.frombuffer(b"CCAGTTTT", np.uint8)
    return refs


def _case(name, kind, groups, piles, tiles, windows, plan=None, seed=1):
    keep_out = set(windows)
    rec = concat_records(neighbours(seed, LENS, keep_out), build_records(groups))
    return PileCase(name, list(LENS), rec, _refs(sorted({p[0] for p in piles})), piles, tiles, windows, kind, plan)


def _pile(barcode, n, P, reverse=False):
    return (barcode, n, P, PILE_SYMBOLS, QMAX, reverse)


def row_cases() -> List[PileCase]:
    """narrow / wide rows: a one-job tile of 256 entries writes 16-bit rows (256 x 255 = 65 280 < 2^16), one of 257 does not"""
    P = 140                                                   # tile 2, the lower tile of window 1
    many = lambda n: [_pile(2 + i, 1, P) for i in range(n)]
    out = [
        _case("256 reads, 256 barcodes", "narrow", many(256), [(P, 256, 256, 0)], {2: 256}, {1: 256}),
        _case("256 reads, one barcode", "narrow", [_pile(0, 256, P)], [(P, 256, 1, 0)], {2: 256}, {1: 256}),
        _case("257 reads, 257 barcodes", "wide", many(257), [(P, 257, 257, 0)], {2: 257}, {1: 257}),
        _case("257 reads, one barcode", "wide", [_pile(0, 257, P)], [(P, 257, 1, 0)], {2: 257}, {1: 257}),
        # narrow by tiles (200 and 57), wide by windows (257)
        _case("200 + 57 in one window", "narrow", [_pile(0, 200, P), _pile(0, 57, 201)], [(P, 200, 1, 0), (201, 57, 1, 0)], {2: 200, 3: 57}, {1: 257}),
    ]
    return out


def limit_cases(n: int) -> List[PileCase]:
    """one barcode's run of n entries (n = JOB_LIMIT: the longest job the packed planes hold; n = JOB_LIMIT + 1: the wide walk's) beside a
    short run of a barcode of the other cell type, reverse strand, in the same tile"""
    kind = "limit" if n <= JOB_LIMIT else "past"
    wide1 = ((0,), n) if kind == "limit" else ((1,), JOB_LIMIT)
    wide12 = ((0,), n) if kind == "limit" else ((1, 2), JOB_LIMIT)      # a pile in two tiles: two wide jobs by tiles, one by windows
    S, B = SECOND_RUN, SECOND_RUN_BEFORE

    def two(P, long_cb=0, second=S):
        return [_pile(long_cb, n, P), _pile(1, second, P, reverse=True)], [(P, n, 1, 0), (P, second, 1, 1)]

    def mk(name, P, tiles, windows, plan, **kw):
        groups, piles = two(P, **kw)
        return _case("%d entries, %s" % (n, name), kind, groups, piles, tiles, windows, plan)

    L = LENS[0]
    return [
        mk("long run first, lower tile, even start", 140, {2: n + S}, {1: n + S}, wide1),
        mk("long run first, lower tile, odd start", 141, {2: n + S}, {1: n + S}, wide1),
        mk("long run last (its job starts inside the tile)", 140, {2: n + B}, {1: n + B}, wide1, long_cb=2, second=B),
        mk("long run first, upper tile", 201, {3: n + S}, {1: n + S}, wide1),
        mk("long run first, across a tile edge", 188, {2: n + S, 3: n + S}, {1: n + S}, wide12),
        mk("long run first, from position 0", 0, {0: n + S}, {0: n + S}, wide1),
        mk("long run first, up to the contig's last position", L - 8, {(L - 1) // 64: n + S}, {(L - 1) // 128: n + S}, wide1),
    ]


def sweep_case(seed=5):
    """a few thousand ordinary reads whose qualities are uniform in the whole byte, some of them piled on one region"""
    lens = [3000, 700]
    rng = np.random.default_rng(seed + 1000)
    refs = [rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=L, p=[0.245, 0.245, 0.245, 0.245, 0.02]) for L in lens]
    n_cb = 40
    ct_of = rng.integers(0, 2, n_cb).astype(np.uint8)
    ct_of[7] = 255
    rec = random_records(seed, 2000, lens, n_cb, hot_regions=[(0, 1000, 1090)], hot_frac=0.5, cb_skew=0.2, max_exons=3, exon_len=(30, 150),
                         intron_len=(20, 300), qual_range=(0, 255))
    return rec, lens, refs, ct_of
