"""Cases of the per-cell genotyping tests (numpy only, no engine): read records whose tiles are deep enough for every trip of
k_geno_sites' block loop and for the store's multi-job tiles, the same reads in coordinate order, and a hand-made contig for the edges
of the depth cap's replay (GenoHostReads::replay).  Every builder returns (rec, lens, celltype_of, keys, alt); tests/test_genotype_cases_cpu.py
counts the preconditions from the records and pins the oracle at the hand-made case, tests/test_genotype_store_gpu.py runs them."""
import dataclasses
import functools

import numpy as np

from longsom_amd.engine import ReadRecords
from tests.support.synth_simple import random_records

DEEP_LENS = np.array([3000, 700, 64, 50], np.int64)
N_CB = 70                                            # not a multiple of 8 or of 64
EMPTY_TILE = (0, 0)                                  # (contig, tile) that deep_case leaves without an entry
FIXED_POS = (1023, 1024, 1055, 1087, 1088)           # lane 0 and lane 63 of the deep tile 16 and of its neighbours, and its middle
WINDOWS = (150, 5000)
DEEP_DEPTHS = (1, 2, 50, 3000)
# the oracle's Dp sums over deep_case's sites with min_mq = 0 (tests/test_genotype_cases_cpu.py computes them; the GPU file compares the
# device's sums with the same numbers): free, and per (window, max_depth)
DEEP_FREE_SUM = 32453
DEEP_CAP_SUMS = {(150, 1): 648, (150, 2): 650, (150, 50): 883, (150, 3000): 23204, (5000, 1): 609, (5000, 2): 611, (5000, 50): 827, (5000, 3000): 23190}


def key(tid, pos):
    return (int(tid) << 32) | int(pos)


def entries_per_tile(rec, lens, n_cb=None, min_mq=0, flag_exclude=0, ignore_orphans=0):
    """admitted entries per 64-position tile, one array per contig: an entry is a segment of a read that has a barcode (inside the table of
    n_cb barcodes, where given), passes the load filter, lies on its contig and overlaps the tile"""
    out = [np.zeros((int(L) + 63) // 64, np.int64) for L in lens]
    for s in range(rec.n_segs):
        r = int(rec.seg_read[s])
        f, cb, tid = int(rec.read_flag[r]), int(rec.read_cb[r]), int(rec.read_tid[r])
        if cb < 0 or (n_cb is not None and cb >= n_cb) or int(rec.read_mapq[r]) < min_mq or (f & flag_exclude) or (ignore_orphans and (f & 1) and not (f & 2)):
            continue
        st, ln = int(rec.seg_start[s]), int(rec.seg_len[s])
        if tid < 0 or tid >= len(lens) or st < 0 or ln <= 0 or st + ln > int(lens[tid]):
            continue
        out[tid][st >> 6:((st + ln - 1) >> 6) + 1] += 1
    return out


@functools.lru_cache(maxsize=None)
def _deep():
    rec = random_records(7, 6000, [3000, 700, 64, 50], 70, hot_regions=[(0, 1024, 1088)], hot_frac=0.9, cb_skew=0.4, max_exons=2, exon_len=(30, 120))
    # every tile of these contigs is under some read: the one read over EMPTY_TILE loses its barcode, so the store holds no entry there
    over = [int(rec.seg_read[s]) for s in range(rec.n_segs) if rec.read_tid[rec.seg_read[s]] == EMPTY_TILE[0] and
            (rec.seg_start[s] >> 6) <= EMPTY_TILE[1] <= ((rec.seg_start[s] + rec.seg_len[s] - 1) >> 6)]
    rec = spoil_reads(rec, over, "cb")
    rng = np.random.default_rng(7007)
    celltype_of = rng.integers(0, 2, N_CB).astype(np.uint8)
    celltype_of[[5, 33, 69]] = 255                   # not in barcodes.tsv; barcode 0 (cb_skew: the deep cell) stays typed
    celltype_of[0] = 0
    sites = {(0, p) for p in FIXED_POS} | {(0, int(p)) for p in rng.integers(1000, 1200, 20)}
    sites |= {(0, 0), (0, 2999), (1, 0), (1, 699), (2, 63), (3, 49)}
    sites.add((3, 50))                               # at its contig's length: counts nothing
    sites.add((EMPTY_TILE[0], EMPTY_TILE[1] * 64 + 17))
    sites = sorted(sites)
    keys = np.array([key(t, p) for t, p in sites], np.int64)
    alt = rng.integers(0, 7, len(keys)).astype(np.uint8)
    return rec, DEEP_LENS, celltype_of, keys, alt


def deep_case():
    """6 000 reads, nine in ten starting inside tile 16 of contig 0 (positions 1024..1087): tile 16 holds more entries than one job of the
    store takes (TM_JOB_LIMIT 4 095), tile 17 more than TM_JOB_TGT (3 072), both more than one trip of the site kernel's block loop (2 048);
    four reads in ten carry barcode 0, whose Dp passes 1 000 at the deep sites (atomics piling up on one word)"""
    rec, lens, ct_of, keys, alt = _deep()
    return rec, lens.copy(), ct_of.copy(), keys.copy(), alt.copy()


def reorder_reads(rec, order):
    """the same reads in the order `order` (old indices): segments follow their reads, seg_read renumbered, events packed again"""
    order = np.asarray(order, np.int64)
    new_of = np.empty(rec.n_reads, np.int64); new_of[order] = np.arange(rec.n_reads)
    seg_order = np.argsort(new_of[rec.seg_read], kind="stable")
    ln = rec.seg_len[seg_order].astype(np.int64)
    off_old = rec.seg_ev_off[seg_order]
    off_new = (np.cumsum(ln) - ln).astype(np.int64)
    idx = np.repeat(off_old - off_new, ln) + np.arange(int(ln.sum()), dtype=np.int64)
    return ReadRecords(rec.read_tid[order], rec.read_pos[order], rec.read_flag[order], rec.read_mapq[order], rec.read_cb[order],
                       new_of[rec.seg_read[seg_order]].astype(np.uint32), rec.seg_start[seg_order], rec.seg_len[seg_order], off_new, rec.events[idx])


def sorted_deep_case():
    """deep_case's reads in coordinate order (stable: reads of one start position keep their file order, so the depth cap drops the same
    reads): GenoHostReads::fetch finds them sorted and skips its sort"""
    rec, lens, ct_of, keys, alt = deep_case()
    order = np.argsort((rec.read_tid.astype(np.int64) << 32) | rec.read_pos.astype(np.int64), kind="stable")
    return reorder_reads(rec, order), lens, ct_of, keys, alt


def with_cb_suffix(rec, seed=5, frac=0.1):
    """a tenth of the reads get LSG_FLAG_CB_SUFFIX (their raw CB carried a "-suffix": strict_cb leaves them out)"""
    flag = rec.read_flag.copy()
    flag[np.random.default_rng(seed).random(rec.n_reads) < frac] |= 0x8000
    return dataclasses.replace(rec, read_flag=flag)


def spoil_reads(rec, reads, what):
    """single reads made uncountable: what = "cb" (no barcode), "mapq" (3), "flag" (duplicate) or "orphan" (paired, mate unmapped)"""
    cb, mq, fl = rec.read_cb.copy(), rec.read_mapq.copy(), rec.read_flag.copy()
    for r in reads:
        if what == "cb":
            cb[r] = -1
        elif what == "mapq":
            mq[r] = 3
        elif what == "flag":
            fl[r] |= 0x400
        elif what == "orphan":
            fl[r] = (fl[r] | 0x1) & ~0x2
        else:
            raise ValueError(what)
    return dataclasses.replace(rec, read_cb=cb, read_mapq=mq, read_flag=fl)


def window_groups(keys, window):
    """group_off of the reference's windows of target sites (HCCVSingleCellGenotype.py:243-265: contig and floor((pos0 + 1) / window))"""
    keys = np.asarray(keys, np.int64)
    code = (keys >> 32) * (1 << 40) + ((keys & 0xFFFFFFFF) + 1) // window
    return np.concatenate([[0], np.nonzero(np.diff(code))[0] + 1, [len(keys)]]).astype(np.int64)


# ---- the hand-made contig of the depth cap's edges --------------------------------------------------------------------------------------
CAP_LEN = 600
# (position, segment length or 0 for a read without segments, flag, mapq) in file order = coordinate order; the index is the read's number
_CAP_READS = (
    # 0..2: position 0 (a group whose region starts at -1); read 0 has no segment: it ends at pos + 1, fills the buffer, is counted nowhere
    [(0, 0, 0, 60), (0, 5, 0, 60), (0, 5, 0, 60)] +
    # 3..16: runs of 1, 2, 3 and 8 reads of one start position, each run gone from the buffer when the next begins (first_here)
    [(10, 1, 0, 60)] + [(12, 1, 0, 60)] * 2 + [(14, 1, 0, 60)] * 3 + [(16, 20, 0, 60)] * 8 +
    # 17..23: read 17 ends where the region [100, 111) starts (never fetched, although first of its position); 18 long, 19 short;
    # 20, 21 start at end_ - 1 = 110; 22, 23 start at end_ = 111
    [(95, 5, 0, 60), (95, 30, 0, 60), (95, 10, 0, 60), (110, 5, 0, 60), (110, 5, 0, 60), (111, 5, 0, 60), (111, 5, 0, 60)] +
    # 24..29: a third supplementary (they fill the buffer, :168 counts none of them)
    [(140, 10, f, 60) for f in (0, 0x800, 0, 0, 0x800, 0)] +
    # 30..36: MAPQ 10 (first of its position), good, orphan, good, duplicate, good, proper pair
    [(170, 10, 0, 10), (170, 10, 0, 60), (170, 10, 0x1, 60), (170, 10, 0, 60), (170, 10, 0x400, 60), (170, 10, 0, 60), (170, 10, 0x3, 60)] +
    # 37: the long read, 300 positions before the group at 500 and across it; 38..77: 40 short reads that end before that group (pmax)
    [(200, 320, 0, 60)] + [(210 + 5 * i, 10, 0, 60) for i in range(40)] +
    # 78..80: three reads at 500; 81..83: read 81 ends at 545, a group's first site (its region starts one position earlier: fetched)
    [(500, 10, 0, 60)] * 3 + [(540, 5, 0, 60), (540, 10, 0, 60), (540, 10, 0, 60)] +
    # 84..87: the contig's end - two reads ending at its last base, two that are its last base only
    [(580, 20, 0, 60)] * 2 + [(599, 1, 0, 60)] * 2)
# the groups of sites (one pileup call each) and, between them, two empty groups
_CAP_GROUPS = ([0, 2], [], [10, 12, 14, 16, 20], [101, 110], [141, 145], [171, 175], [], [300, 302], [500, 505], [545, 550], [590, 599])


# the oracle's Dp sums over cap_edge_case's sites and groups, per parameter set: {0: free, max_depth: capped}
CAP_EDGE_SUMS = {(): {0: 69, 1: 25, 2: 37, 3: 50},
                 (("min_mq", 0), ("ignore_orphans", 0)): {0: 73, 1: 25, 2: 37, 3: 50}}


def cap_edge_case():
    n = len(_CAP_READS)
    pos = np.array([r[0] for r in _CAP_READS], np.int32)
    seg_read = np.array([i for i, r in enumerate(_CAP_READS) if r[1] > 0], np.uint32)
    seg_len = np.array([r[1] for r in _CAP_READS if r[1] > 0], np.int32)
    seg_start = pos[seg_read]
    off = (np.cumsum(seg_len, dtype=np.int64) - seg_len).astype(np.int64)
    within = np.arange(int(seg_len.sum())) - np.repeat(off, seg_len)
    sym = ((np.repeat(seg_read, seg_len) + np.repeat(seg_start, seg_len) + within) % 4).astype(np.uint16)      # bases only, quality 40
    events = (0x0800 | (sym << 8) | 40).astype(np.uint16)
    rec = ReadRecords(np.zeros(n, np.int32), pos, np.array([r[2] for r in _CAP_READS], np.uint16), np.array([r[3] for r in _CAP_READS], np.uint8),
                      (np.arange(n) % 4).astype(np.int32), seg_read, seg_start, seg_len, off, events)
    sites = [p for g in _CAP_GROUPS for p in g]
    keys = np.array([key(0, p) for p in sites], np.int64)
    alt = (np.arange(len(keys)) % 4).astype(np.uint8)
    return rec, np.array([CAP_LEN], np.int64), np.array([0, 1, 0, 1, 255], np.uint8), keys, alt


def cap_edge_groups():
    """group_off over cap_edge_case's sites: the first group starts at position 0, the last ends at the contig's last base, two are empty"""
    return np.concatenate([[0], np.cumsum([len(g) for g in _CAP_GROUPS])]).astype(np.int64)
