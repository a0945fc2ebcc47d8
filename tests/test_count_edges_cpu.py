"""CPU: the directed piles of tests/support/pile_cases.py are what they claim to be - proved from the records and the events-level oracle
(oracle/count_oracle.c, 32-bit sums) alone, so that a failure of tests/test_count_edges_gpu.py means the kernel and not the fixture -
and the arithmetic by which every packed field of the count kernels fits its worst case, stated as expressions."""
import numpy as np
import pytest

from longsom_amd.engine import ReadRecords
from tests.support import pile_cases as pc
from tests.support.synth_simple import random_records
from tests.util import phased_records

DP, NC, CC, BC, BQ, BCF, BCR = 0, 1, 2, 10, 18, 26, 34          # columns of an oracle row (count_oracle.c: 42 words)


def test_the_fields_fit_their_worst_case_exactly():
    """TM_JOB_LIMIT = 4095 entries of 8-bit qualities against pileup.hip's fields (tm_add: quality sum 20 | forward 12, count 16 |
    duplicates 16; tw_add: quality sum 20 | forward 12 || count 13 | duplicates x 2^symbol 19) and the narrow rows' 16 bits"""
    assert pc.JOB_LIMIT == 4095 and pc.NARROW_MAX == 256 and pc.QMAX == 255
    assert (1 << 20) - 1 - 4095 * 255 == 4350                    # the quality sum's headroom: 17 more entries of quality 255 would carry into the forward count
    assert (1 << 20) - 1 - 4095 * 255 >= 0 and (1 << 20) - 1 - 4096 * 255 >= 0 and (1 << 20) - 1 - 4113 * 255 < 0
    assert 4095 == (1 << 12) - 1                                 # the forward count fills its field to the last value
    assert 4095 < (1 << 13)                                      # the windows' count
    assert 4094 <= 4095                                          # the windows' duplicates of symbol class 7 (every entry of a run but its first) in the 32 - 13 - 7 = 12 bits left
    assert 32 - 13 - 7 == 12
    assert 256 * 255 < 1 << 16                                   # a narrow row's largest quality sum: 65 280
    assert 257 * 255 == 0xFFFF                                   # ... and the first tile that is not narrow would still fit, by one
    assert 258 * 255 > 0xFFFF


def oracle(case, ct, min_bq=255):
    from oracle import loader
    k, rf, c, ncols = loader.count(case.rec, case.lens, case.refs, case.celltype_of(2), ct, min_bq=min_bq, min_mq=0, min_dp=1, min_cc=1)
    return {int(key): row for key, row in zip(k, c)}


ALL_CASES = pc.row_cases() + pc.limit_cases(pc.JOB_LIMIT) + pc.limit_cases(pc.JOB_LIMIT + 1)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    by_tile, by_win = pc.entries_per_bin(case.rec, 64), pc.entries_per_bin(case.rec, 128)
    for t, n in case.tiles.items():
        assert by_tile.get((0, t), 0) == n, "tile %d" % t
    for w, n in case.windows.items():
        assert by_win.get((0, w), 0) == n, "window %d" % w
        for t in (2 * w, 2 * w + 1):                             # nothing but the pile in its windows
            assert by_tile.get((0, t), 0) == case.tiles.get(t, 0)
    assert len(by_tile) > len(case.tiles) + 3                    # the ordinary reads are there ...
    segs_in_two = sum(1 for s in range(case.rec.n_segs) if case.rec.seg_len[s] < 64 and case.rec.seg_start[s] // 64 != (case.rec.seg_start[s] + case.rec.seg_len[s] - 1) // 64)
    assert segs_in_two > 0                                       # ... and some of their segments straddle a tile edge
    # the phased layout holds the same events (what the device sees in paths 5 and 6), the largest case 525 k of them
    ph = phased_records(case.rec)
    assert len(ph.events) % 128 == 0 and len(ph.events) <= 128 * (case.rec.n_segs + case.rec.n_reads)
    # the oracle's rows at the pile's positions
    rows = [oracle(case, ct) for ct in (0, 1)]
    L = case.lens[0]
    for P, n, n_cb, ct in case.piles:
        for k in range(8):
            pos = P + k
            assert pos < L
            if pos == 0:
                assert pos not in rows[ct]                       # (0-based position 0 is never visited: count_oracle.c)
                continue
            r = rows[ct][pos]
            fwd = ct == 0
            assert r[DP] == n and r[NC] == n_cb
            for sym in range(8):
                want = n if sym == k else 0
                assert r[BC + sym] == want and r[BQ + sym] == want * 255
                assert r[BCF + sym] == (want if fwd else 0) and r[BCR + sym] == (0 if fwd else want)
                assert r[CC + sym] == (n_cb if sym == k else 0)
                assert r[BC + sym] - r[CC + sym] == (n - n_cb if sym == k else 0)          # the duplicates the kernels count
    # the same rows under the product's min_bq = 20 at the pile's positions (the ordinary reads' qualities end at 60)
    rows20 = [oracle(case, ct, min_bq=20) for ct in (0, 1)]
    for P, n, n_cb, ct in case.piles:
        for k in range(8):
            if P + k:
                np.testing.assert_array_equal(rows20[ct][P + k], rows[ct][P + k])


def _at(case, P, ct=0):
    return oracle(case, ct)[P + 7]


def test_the_named_cases_table():
    """symbol class 7's position of the named cases: DP, NC, BC[7], BQ[7], BCf[7]"""
    rows, lim, past = pc.row_cases(), pc.limit_cases(4095), pc.limit_cases(4096)
    name = {c.name: c for c in rows + lim + past}
    for nm, want in (("256 reads, 256 barcodes", (256, 256, 256, 65280, 256)), ("256 reads, one barcode", (256, 1, 256, 65280, 256)),
                     ("257 reads, one barcode", (257, 1, 257, 65535, 257)), ("4095 entries, long run first, lower tile, even start", (4095, 1, 4095, 1044225, 4095)),
                     ("4096 entries, long run first, lower tile, even start", (4096, 1, 4096, 1044480, 4096))):
        r = _at(name[nm], 140)
        assert (r[DP], r[NC], r[BC + 7], r[BQ + 7], r[BCF + 7]) == want, nm
    r = _at(name["4095 entries, long run first, lower tile, even start"], 140, ct=1)
    assert (r[DP], r[NC], r[BC + 7], r[BQ + 7], r[BCF + 7], r[BCR + 7]) == (5, 1, 5, 1275, 0, 5)
    # every symbol class falls on both parities of the windows' half-words: even and odd pile starts
    assert {c.piles[0][0] % 2 for c in lim} == {0, 1}
    # position 0 and the contig's last position each appear
    assert any(c.piles[0][0] == 0 for c in lim) and any(c.piles[0][0] + 8 == c.lens[0] for c in lim)
    # the long run first and last in its tile; the lower and the upper tile of a window; across a tile edge
    assert any(c.piles[0][1] == 4095 and c.piles[1][1] == pc.SECOND_RUN_BEFORE for c in lim)
    assert {(c.piles[0][0] // 64) % 2 for c in lim} == {0, 1} and any(len(c.tiles) == 2 for c in lim)


def test_where_the_plan_cuts_a_limit_tile():
    """store.hip tm_make_job restated: which jobs a tile of the limit cases is cut into (J = ceil(n / 768) jobs, each from the first run
    start at or after n j / J) - the long run is ONE job of exactly its own entries in every case, first or last in its tile"""
    def jobs(runs, tgt=768):
        n = sum(runs)
        starts = np.cumsum([0] + runs[:-1]).tolist()
        J = 1 if n <= tgt else -(-n // tgt)
        cut = lambda x: min([s for s in starts if s >= x] + [n])
        out = []
        for j in range(J):
            e0 = 0 if j == 0 else cut(n * j // J)
            e1 = n if j + 1 == J else cut(n * (j + 1) // J)
            out.append(max(e1, e0) - e0)
        return [x for x in out if x]
    for n in (4095, 4096):
        assert jobs([n, pc.SECOND_RUN]) == [n, pc.SECOND_RUN]                      # barcode 0's run, then barcode 1's
        assert jobs([pc.SECOND_RUN_BEFORE, n]) == [pc.SECOND_RUN_BEFORE, n]        # barcode 1's run, then barcode 2's
        assert jobs([pc.SECOND_RUN, n]) == [n + pc.SECOND_RUN]                      # (why the run before a last long run is not 5 entries: one job of the whole tile)


def test_quality_sweep_case_spans_the_byte():
    rec, lens, refs, ct_of = pc.sweep_case()
    q = rec.events[rec.events != 0] & 0xff
    assert q.min() == 0 and q.max() == 255 and {127, 128, 93, 200}.issubset(set(np.unique(q).tolist()))
    assert rec.n_reads == 2000
    assert abs(float((q >= 128).mean()) - 0.5) < 0.02
    from oracle import loader
    cols = [loader.count(rec, lens, refs, ct_of, 0, min_bq=b, min_mq=0, min_dp=1, min_cc=1)[3] for b in (0, 1, 93, 128, 200, 255, 256)]
    assert all(a >= b for a, b in zip(cols, cols[1:])) and cols[-2] > 0 and cols[-1] == 0
    deep = max(pc.entries_per_bin(rec, 64).values())
    assert deep > 768                                            # a tile of several jobs is among them


# ---- random_records draws the records it always drew --------------------------------------------
def random_records_before(seed, n_reads, contig_lens, n_cb, hot_regions=(), hot_frac=0.0, cb_skew=0.0,
                          max_exons=4, exon_len=(30, 400), intron_len=(20, 3000)):
    """tests/support/synth_simple.py random_records as it was before it took a quality range, word for word"""
    rng = np.random.default_rng(seed)
    contig_lens = np.asarray(contig_lens, dtype=np.int64)
    read_tid = np.zeros(n_reads, np.int32); read_pos = np.zeros(n_reads, np.int32)
    read_flag = np.zeros(n_reads, np.uint16); read_mapq = np.zeros(n_reads, np.uint8)
    read_cb = np.zeros(n_reads, np.int32)
    seg_read, seg_start, seg_len = [], [], []
    for r in range(n_reads):
        if hot_regions and rng.random() < hot_frac:
            tid, hs, he = hot_regions[int(rng.integers(0, len(hot_regions)))]
            start = int(rng.integers(max(0, hs - 20), he))
        else:
            tid = int(rng.integers(0, len(contig_lens)))
            start = int(rng.integers(0, max(1, contig_lens[tid] - 50)))
        clen = int(contig_lens[tid])
        pos = start
        n_ex = int(rng.integers(1, max_exons + 1))
        first = True
        for _ in range(n_ex):
            ln = int(rng.integers(exon_len[0], exon_len[1]))
            if pos >= clen:
                break
            ln = min(ln, clen - pos)
            if ln <= 0:
                break
            seg_read.append(r); seg_start.append(pos); seg_len.append(ln)
            if first:
                read_pos[r] = pos; first = False
            pos += ln + int(rng.integers(intron_len[0], intron_len[1]))
        read_tid[r] = tid
        f = 0
        u = rng.random()
        if u < 0.5: f |= 0x10
        u = rng.random()
        if u < 0.01: f |= 0x800
        elif u < 0.015: f |= 0x100
        elif u < 0.017: f |= 0x400
        elif u < 0.018: f |= 0x200
        elif u < 0.019: f |= 0x4
        elif u < 0.022: f |= 0x1          # paired, not proper pair -> orphan
        elif u < 0.025: f |= 0x3          # proper pair -> kept
        read_flag[r] = f
        read_mapq[r] = 60 if rng.random() < 0.92 else int(rng.integers(0, 60))
        u = rng.random()
        if u < 0.02: read_cb[r] = -1
        elif rng.random() < cb_skew: read_cb[r] = 0
        else: read_cb[r] = int(rng.integers(0, n_cb))
    seg_read = np.asarray(seg_read, np.uint32); seg_start = np.asarray(seg_start, np.int32); seg_len = np.asarray(seg_len, np.int32)
    n_ev = int(seg_len.sum())
    seg_ev_off = np.concatenate([[0], np.cumsum(seg_len)[:-1]]).astype(np.int64) if len(seg_len) else np.zeros(0, np.int64)
    # symbols: mostly A/C/T/G, some indel anchors / deletions / N / NA
    sym = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 15], dtype=np.uint16), size=n_ev,
                     p=[0.235, 0.235, 0.235, 0.235, 0.01, 0.01, 0.005, 0.025, 0.01])
    qual = np.where(rng.random(n_ev) < 0.9, rng.integers(20, 61, n_ev), rng.integers(2, 20, n_ev)).astype(np.uint16)
    events = np.where(sym < 8, 0x0800 | (sym << 8) | qual, 0).astype(np.uint16)      # LSG_EVENT(sym, qual)
    return ReadRecords(read_tid, read_pos, read_flag, read_mapq, read_cb, seg_read, seg_start, seg_len, seg_ev_off, events)


@pytest.mark.parametrize("seed,args,kw", [(1, (600, [5000, 1200, 70], 50), {}),
                                          (14, (900, [2500], 30), dict(hot_regions=[(0, 700, 760)], hot_frac=0.97, cb_skew=0.9))])
def test_existing_seeds_draw_the_same_records(seed, args, kw):
    a, b = random_records(seed, *args, **kw), random_records_before(seed, *args, **kw)
    for name, _ in ReadRecords._SPEC:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    # ... and a quality range changes the qualities alone
    c = random_records(seed, *args, qual_range=(0, 255), **kw)
    for name, _ in ReadRecords._SPEC[:-1]:
        assert getattr(c, name).tobytes() == getattr(b, name).tobytes(), name
    np.testing.assert_array_equal(c.events & 0xff00, b.events & 0xff00)
    assert (c.events & 0xff).max() > 200
