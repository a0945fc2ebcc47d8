"""CPU: the cases of tests/test_genotype_store_gpu.py (tests/support/geno_cases.py) are what they claim to be - counted from the records -
and the oracle the GPU tests lean on (oracle/genotype_oracle.py depth_cap_drops) gives the hand-derived answers at every edge of the depth
cap's replay that the hand-made contig holds.  No GPU, no engine."""
import numpy as np
import pytest

from oracle import genotype_oracle as go
from tests.support import geno_cases as gc
from tests.util import assert_same_records, phased_records


def events_at_sites(rec, keys):
    """the events of every segment at every site it covers"""
    out = []
    keys = np.asarray(keys, np.int64)
    for s in range(rec.n_segs):
        k_lo = (int(rec.read_tid[int(rec.seg_read[s])]) << 32) | int(rec.seg_start[s])
        for k in keys[np.searchsorted(keys, k_lo):np.searchsorted(keys, k_lo + int(rec.seg_len[s]))]:
            out.append(int(rec.events[int(rec.seg_ev_off[s]) + int(k) - k_lo]))
    return np.array(out)


def test_deep_case_is_deep_where_the_kernels_change_path():
    rec, lens, ct_of, keys, alt = gc.deep_case()
    assert rec.n_reads == 6000 and len(ct_of) == 70 and 0 < (ct_of == 255).sum() < 8 and ct_of[0] != 255
    assert (np.diff(keys) > 0).all() and set(alt.tolist()) == set(range(7))
    e = gc.entries_per_tile(rec, lens)
    assert e[0][16] > 4095                                        # more than one job of the store takes (TM_JOB_LIMIT)
    assert e[0][17] > 3072                                        # past TM_JOB_TGT
    assert 0 < e[0][15] < 2048 and 0 < e[0][18] < 2048            # one trip of the site kernel's block loop (256 threads x 8 entries)
    assert (e[0][16], e[0][17], e[0][15]) == (5259, 4229, 1240)
    site_tiles = {(int(k >> 32), int(k & 0xFFFFFFFF) >> 6) for k in keys if (k & 0xFFFFFFFF) < lens[k >> 32]}
    assert {(0, 15), (0, 16), (0, 17), (0, 18), gc.EMPTY_TILE, (0, 46), (1, 0), (1, 10), (2, 0), (3, 0)} <= site_tiles
    assert e[gc.EMPTY_TILE[0]][gc.EMPTY_TILE[1]] == 0             # a site in a tile without an entry
    for p in gc.FIXED_POS:
        assert gc.key(0, p) in keys
    ev = events_at_sites(rec, keys)
    valid = ev[(ev & 0x0800) != 0]
    assert set(((valid >> 8) & 7).tolist()) == set(range(8)) and (ev == 0).any()      # the seven alt classes, 'O' and 'NA'
    dp, al = go.genotype(rec, lens, ct_of, keys, alt, min_mq=0)
    assert dp.max() == dp[:, 0].max() == 1066 and dp.sum() == gc.DEEP_FREE_SUM       # one cell's Dp past 1 000: atomics on one word
    at = {int(k): i for i, k in enumerate(keys)}
    assert dp[at[gc.key(3, 50)]].sum() == 0 and dp[at[gc.key(3, 49)]].sum() > 0      # at the contig's length: nothing
    assert dp[at[gc.key(gc.EMPTY_TILE[0], gc.EMPTY_TILE[1] * 64 + 17)]].sum() == 0
    assert (dp[:, ct_of == 255] == 0).all() and 0 < al.sum() < dp.sum()
    for p in gc.FIXED_POS:
        assert dp[at[gc.key(0, p)]].sum() > 100


def test_sorted_deep_case_is_the_same_reads_in_coordinate_order():
    rec, lens, ct_of, keys, alt = gc.deep_case()
    srt = gc.sorted_deep_case()[0]
    k = (srt.read_tid.astype(np.int64) << 32) | srt.read_pos
    assert (np.diff(k) >= 0).all() and not (np.diff((rec.read_tid.astype(np.int64) << 32) | rec.read_pos) >= 0).all()
    assert (np.diff(srt.seg_read.astype(np.int64)) >= 0).all() and srt.n_segs == rec.n_segs and srt.n_events == rec.n_events
    order = np.argsort((rec.read_tid.astype(np.int64) << 32) | rec.read_pos.astype(np.int64), kind="stable")
    assert_same_records(srt, gc.reorder_reads(rec, order))
    np.testing.assert_array_equal(srt.read_cb, rec.read_cb[order])
    for a, b in zip(go.genotype(srt, lens, ct_of, keys, alt, min_mq=0), go.genotype(rec, lens, ct_of, keys, alt, min_mq=0)):
        np.testing.assert_array_equal(a, b)
    g = gc.window_groups(keys, 150)
    assert go.genotype(srt, lens, ct_of, keys, alt, min_mq=0, group_off=g, max_depth=50)[0].sum() == gc.DEEP_CAP_SUMS[150, 50]


def test_phased_deep_case_holds_the_same_records():
    rec = gc.deep_case()[0]
    ph = phased_records(rec)
    assert_same_records(ph, rec, phased_a=True)
    assert len(ph.events) > len(rec.events)


@pytest.mark.parametrize("window", gc.WINDOWS)
def test_every_capped_configuration_of_the_deep_case_drops_reads_and_leaves_some(window):
    """no GPU case is vacuous: under each cap the oracle's Dp sum lies strictly between zero and the free one"""
    rec, lens, ct_of, keys, alt = gc.deep_case()
    g = gc.window_groups(keys, window)
    for d in gc.DEEP_DEPTHS:
        dp, al = go.genotype(rec, lens, ct_of, keys, alt, min_mq=0, group_off=g, max_depth=d)
        assert dp.sum() == gc.DEEP_CAP_SUMS[window, d] and 0 < dp.sum() < gc.DEEP_FREE_SUM, (window, d)


def test_every_capped_configuration_of_the_hand_made_contig_drops_reads_and_leaves_some():
    rec, lens, ct_of, keys, alt = gc.cap_edge_case()
    g = gc.cap_edge_groups()
    assert g[0] == 0 and g[-1] == len(keys) and (np.diff(g) == 0).sum() == 2
    assert int(keys[0]) == 0 and int(keys[-1]) == gc.CAP_LEN - 1                   # a region from -1, a region to the contig's end
    for kw, sums in gc.CAP_EDGE_SUMS.items():
        free = go.genotype(rec, lens, ct_of, keys, alt, **dict(kw))[0].sum()
        assert free == sums[0]
        for d in (1, 2, 3):
            dp = go.genotype(rec, lens, ct_of, keys, alt, group_off=g, max_depth=d, **dict(kw))[0]
            assert dp.sum() == sums[d] and 0 < dp.sum() < free, (kw, d)


# the hand-derived drops: region [first site - 1, last site + 1) -> {max_depth: dropped reads}.  A read enters when it is the first fetched
# read of its start position, or when (reads that entered and end at or after that position) + 1 <= max_depth.
HAND = [
    # reads 0..2 at position 0, read 0 without a segment (it ends at 1 > -1: fetched, enters first and fills the buffer)
    ((-1, 3), {1: {1, 2}, 2: {2}, 3: set()}),
    # 3 | 4 5 | 6 7 8 | 9..16: every run has left the buffer when the next starts, so max_depth reads of a run enter
    ((9, 21), {1: {5, 7, 8} | set(range(10, 17)), 2: {8} | set(range(11, 17)), 3: set(range(12, 17))}),
    # 17 ends at 100 = the region's start: not fetched, so 18 is the first of 95 (ends 125), 19 the second (ends 105, gone at 110);
    # 20 and 21 start at end_ - 1 beside 18; 22 and 23 start at end_: outside
    ((100, 111), {1: {19, 21}, 2: {21}, 3: set()}),
    # 24..29 at 140, 25 and 28 supplementary: they take places in the buffer like any read
    ((140, 146), {1: {25, 26, 27, 28, 29}, 2: {26, 27, 28, 29}, 3: {27, 28, 29}}),
    # 30 (MAPQ 10), 32 (orphan), 34 (duplicate) never reach the buffer: 31 is the first of 170, then 33, 35, 36
    ((170, 176), {1: {33, 35, 36}, 2: {35, 36}, 3: {36}}),
    # the long read 37 and three short ones of 290, 295, 300, each the first of its position: nothing drops at any depth
    ((299, 303), {1: set(), 2: set(), 3: set()}),
    # 37 (200..520) is found behind 40 reads that ended long before; 78 is the first of 500, 79 and 80 meet a buffer of two
    ((499, 506), {1: {79, 80}, 2: {79, 80}, 3: {80}}),
    # 81 ends at 545, the group's first site: the region starts at 544, so it is fetched and is the first of 540 although it covers no site
    ((544, 551), {1: {82, 83}, 2: {83}, 3: set()}),
    # 84, 85 end at the contig's end, 86, 87 are its last base
    ((589, 600), {1: {85, 87}, 2: {87}, 3: {87}}),
]


def test_depth_cap_drops_hand_derived_answers():
    rec, lens, ct_of, keys, alt = gc.cap_edge_case()
    g = gc.cap_edge_groups()
    regions = [(int(keys[a]) - 1, int(keys[b - 1]) + 1) for a, b in zip(g[:-1], g[1:]) if b > a]
    assert regions == [r for r, _ in HAND]                        # the GPU test's groups are these regions
    for (start, end), want in HAND:
        for d, drops in want.items():
            assert go.depth_cap_drops(rec, 0, start, end, 60, 0xF04, 1, d) == drops, (start, end, d)
    # without min_mq and with orphans, 30 is the first of 170 and 32 takes a place too (34, a duplicate, still does not)
    for d, drops in {1: {31, 32, 33, 35, 36}, 2: {32, 33, 35, 36}, 3: {33, 35, 36}}.items():
        assert go.depth_cap_drops(rec, 0, 170, 176, 0, 0xF04, 0, d) == drops
    # a flag filter without the supplementary bit changes nothing for 25 and 28: the pileup never filtered them
    assert go.depth_cap_drops(rec, 0, 140, 146, 60, 0x704, 1, 2) == {26, 27, 28, 29}
    # the region one position later no longer fetches read 0 (it ends at 1): read 1 is first
    assert go.depth_cap_drops(rec, 0, 1, 3, 60, 0xF04, 1, 1) == {2}
    # a dropped supplementary read is in the set and counted nowhere; a dropped good read loses its counts
    free = go.genotype(rec, lens, ct_of, keys, alt)[0]
    cap = go.genotype(rec, lens, ct_of, keys, alt, group_off=g, max_depth=1)[0]
    i = int(np.searchsorted(keys, 141))
    assert free[i].sum() == 4 and cap[i].sum() == 1               # 24, 26, 27, 29 free; 24 alone under the cap


def test_oracle_docstring_names_the_tests_that_pin_it():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for word in go.__doc__.split():
        if word.strip("().,:;").startswith("tests/"):
            assert os.path.exists(os.path.join(root, word.strip("().,:;").split("::")[0])), word
