"""GPU: the load's first half (store.hip: the admission pass k_seg_static; the scatter k_bin, whose loads are taken an item ahead -
bin_fetch / bin_make - and whose eight entries' hash operations go side by side) at the shapes where a pipeline goes wrong: the edges
of a batch (256 segments; 1 024 in the admission pass) and of a dequeue (16 batches), chunks that stop in the middle of a batch and
resume there, segments cut by pileup-window edges, clamped and prefetched loads of segments nobody may count, a few contigs and many
(a contig table in LDS was tried for the admission pass, docs/TRIED.md: its bound would lie between them), and a read whose span marks
come from two batches.  Every case goes through tests.test_fused_gpu.fused_vs_oracle (compact, phased and hinted-phased input: bins of
64 and of 128 positions) and equals the CPU oracle bit for bit."""
import dataclasses

import numpy as np
import pytest

from longsom_amd._lib import CountParams
from longsom_amd.engine import ReadRecords
from tests.support.synth_simple import random_reference
from tests.test_depth_bound_gpu import tile_bound
from tests.test_fused_gpu import fused_vs_oracle

pytestmark = pytest.mark.gpu

BATCH, SUPER = 256, 16           # store.hip: BIN_THREADS, BIN_SUPER
N_CB = 40


def records(rng, read_tid, read_cb, read_flag, read_mapq, seg_read, seg_start, seg_len):
    """ReadRecords from hand-made read and segment columns: compact events, random symbols and qualities"""
    seg_read = np.asarray(seg_read, np.uint32); seg_start = np.asarray(seg_start, np.int32); seg_len = np.asarray(seg_len, np.int32)
    R = len(read_tid)
    read_pos = np.zeros(R, np.int32)
    first = np.r_[True, seg_read[1:] != seg_read[:-1]] if len(seg_read) else np.zeros(0, bool)
    read_pos[seg_read[first]] = seg_start[first]
    n_ev = int(seg_len.sum())
    off = (np.cumsum(seg_len, dtype=np.int64) - seg_len).astype(np.int64)
    sym = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 15], dtype=np.uint16), size=n_ev, p=[0.235, 0.235, 0.235, 0.235, 0.01, 0.01, 0.005, 0.025, 0.01])
    qual = np.where(rng.random(n_ev) < 0.9, rng.integers(20, 61, n_ev), rng.integers(2, 20, n_ev)).astype(np.uint16)
    events = np.where(sym < 8, 0x0800 | (sym << 8) | qual, 0).astype(np.uint16)
    return ReadRecords(np.asarray(read_tid, np.int32), read_pos, np.asarray(read_flag, np.uint16), np.asarray(read_mapq, np.uint8),
                       np.asarray(read_cb, np.int32), seg_read, seg_start, seg_len, off, events)


def sorted_case(seed, n_segs, lens, seg_len=(20, 300), segs_per_read=(1, 3)):
    """n_segs segments of reads with one to three exons each, the reads in coordinate order as in a sorted BAM (consecutive batches
    hit the same tiles); returns the columns so that a test can spoil single reads and segments before it builds the records"""
    rng = np.random.default_rng(seed)
    n_reads = n_segs                                   # at most: cut below
    tid = np.sort(rng.integers(0, len(lens), n_reads)).astype(np.int32)
    start = np.zeros(n_reads, np.int64)
    for t, L in enumerate(lens):
        m = tid == t
        start[m] = np.sort(rng.integers(0, max(1, int(L) - 3 * (seg_len[1] + 200)), int(m.sum())))
    sr, ss, sl = [], [], []
    for r in range(n_reads):
        pos = int(start[r])
        for _ in range(int(rng.integers(segs_per_read[0], segs_per_read[1] + 1))):
            ln = int(rng.integers(seg_len[0], seg_len[1]))
            if len(sr) == n_segs or pos + ln > int(lens[tid[r]]):
                break
            sr.append(r); ss.append(pos); sl.append(ln)
            pos += ln + int(rng.integers(20, 200))
        if len(sr) == n_segs:
            break
    R = sr[-1] + 1
    used = np.zeros(R, bool); used[sr] = True
    assert used.all() and len(sr) == n_segs
    cols = dict(read_tid=tid[:R].copy(), read_cb=rng.integers(0, N_CB, R).astype(np.int32), read_flag=np.where(rng.random(R) < 0.5, 0x10, 0).astype(np.uint16),
                read_mapq=np.full(R, 60, np.uint8), seg_read=np.array(sr, np.uint32), seg_start=np.array(ss, np.int32), seg_len=np.array(sl, np.int32))
    return rng, cols


def table(seed, lens):
    rng = np.random.default_rng(seed + 5000)
    refs = [random_reference(rng, int(L)) for L in lens]
    ct_of = rng.integers(0, 2, N_CB).astype(np.uint8)
    ct_of[rng.random(N_CB) < 0.05] = 255
    return refs, ct_of


def spoil(cols, lens, at):
    """the segments `at` become inadmissible, one kind after the other: no barcode, MAPQ under the load filter (60), tid -1, off the
    contig's end - a clamped or prefetched load of one of them must never be counted"""
    for n, s in enumerate(at):
        r = int(cols["seg_read"][s])
        kind = n % 4
        if kind == 0:
            cols["read_cb"][r] = -1
        elif kind == 1:
            cols["read_mapq"][r] = 3
        elif kind == 2:
            cols["read_tid"][r] = -1
        else:
            L = int(lens[cols["read_tid"][r]]) if cols["read_tid"][r] >= 0 else int(lens[0])
            cols["seg_start"][s] = L - 10; cols["seg_len"][s] = 40


@pytest.mark.parametrize("n_segs", [1, BATCH - 1, BATCH, BATCH + 1, BATCH * SUPER - 1, BATCH * SUPER, BATCH * SUPER + 1, 2 * BATCH * SUPER + 3])
def test_batch_and_super_edges_with_inadmissible_neighbours(engine, n_segs):
    lens = [30000, 2500]
    rng, cols = sorted_case(100 + n_segs, n_segs, lens)
    edges = [e for e in (BATCH, 4 * BATCH, BATCH * SUPER, 2 * BATCH * SUPER) if e < n_segs]       # (4 x 256: a batch of the admission pass)
    at = sorted({s for e in edges for s in (e - 1, e)} | {n_segs - 1}) if n_segs > 1 else []
    spoil(cols, lens, at)
    rec = records(rng, **cols)
    refs, ct_of = table(n_segs, lens)
    engine.set_load_filter(60, 0, 0)                             # (the count's own min_mq: what is dropped here no count could admit)
    try:
        fused_vs_oracle(engine, rec, lens, refs, ct_of, 2, CountParams.longsom_defaults())
    finally:
        engine.set_load_filter()


def test_a_read_index_outside_the_reads_is_still_refused(engine):
    lens = [30000, 2500]
    rng, cols = sorted_case(7, 2 * BATCH * 4 + 5, lens)
    rec = records(rng, **cols)
    refs, ct_of = table(7, lens)
    engine.set_contigs(lens)
    for t, r in enumerate(refs):
        engine.load_reference(t, r)
    engine.set_barcodes(ct_of, 2)
    for s in (4 * BATCH, BATCH, len(rec.seg_read) - 1):          # first of a batch (both kernels'), the load's last segment
        sr = rec.seg_read.copy(); sr[s] = rec.n_reads
        with pytest.raises(RuntimeError, match="read index"):
            engine.load_reads(dataclasses.replace(rec, seg_read=sr))
        assert engine.reads_shape() == (0, 0, 0)
    fused_vs_oracle(engine, rec, lens, refs, ct_of, 2, CountParams.longsom_defaults())


def test_rounds_and_a_chunk_that_stops_inside_a_batch(engine):
    """eight consecutive batches that each hold one 5 000-position segment (40 windows: 5 rounds of eight; 79 tiles: 10 rounds) between
    short ones of the same region: the 32 items of a chunk run out in the middle of a batch and the next chunk resumes at that round"""
    lens = [6000]
    n = 8 * BATCH + 40
    rng, cols = sorted_case(21, n, lens, seg_len=(20, 120), segs_per_read=(1, 2))
    for b in range(8):
        s = b * BATCH + 57 + b
        r = int(cols["seg_read"][s])
        own = np.flatnonzero(cols["seg_read"] == r)
        if len(own) > 1:                                          # the long one stands alone in its read: take the read's other segments short and early
            cols["seg_start"][own] = 10 + 150 * np.arange(len(own)); cols["seg_len"][own] = 30
        cols["seg_start"][s] = 400 + b; cols["seg_len"][s] = 5000
        if len(own) > 1 and own[-1] != s:                        # keep a read's segments in position order
            cols["seg_start"][own[own > s]] = 5500 + 40 * np.arange(int((own > s).sum())); cols["seg_len"][own[own > s]] = 30
    rec = records(rng, **cols)
    refs, ct_of = table(21, lens)
    fused_vs_oracle(engine, rec, lens, refs, ct_of, 2, CountParams.longsom_defaults())


def test_batches_that_fill_the_hash(engine):
    """256 segments of 1 500 positions, each somewhere else: a batch touches 3 000 windows (6 000 tiles), more than the hash takes
    (2 560), so the chunk stops on its fill after one round and the batch's other rounds follow in chunks of their own"""
    n = 2 * BATCH + 9
    L = 2000 * n + 4000
    rng = np.random.default_rng(33)
    R = n
    cols = dict(read_tid=np.zeros(R, np.int32), read_cb=rng.integers(0, N_CB, R).astype(np.int32), read_flag=np.zeros(R, np.uint16), read_mapq=np.full(R, 60, np.uint8),
                seg_read=np.arange(n, dtype=np.uint32), seg_start=(2000 * np.arange(n) + rng.integers(0, 400, n)).astype(np.int32), seg_len=np.full(n, 1500, np.int32))
    rec = records(rng, **cols)
    refs, ct_of = table(33, [L])
    fused_vs_oracle(engine, rec, [L], refs, ct_of, 2, CountParams.longsom_defaults(min_dp=0, min_cc=0))      # (depth 1: the gates would leave no row)


def test_pileup_window_edges_inside_a_bin(engine):
    """contigs longer than a pileup window: segments crossing position 50 001 (inside a bin of 64 and of 128) in several batches, one
    segment longer than a whole window (two edges inside it), inadmissible ones among them"""
    lens = [160000, 60000]
    n = 3 * BATCH + 11
    rng, cols = sorted_case(41, n, lens)
    R = len(cols["read_tid"])
    lone = np.flatnonzero(np.bincount(cols["seg_read"], minlength=R)[cols["seg_read"]] == 1)      # segments that are their read's only one
    pick = lone[np.linspace(0, len(lone) - 1, 60).astype(int)]
    for j, s in enumerate(pick):
        cols["seg_start"][s] = 49990 - 7 * j + (j % 5) * 3; cols["seg_len"][s] = 30 + 9 * j            # (start .. end straddle 50 000 and 50 001)
    s = int(pick[30])
    cols["seg_start"][s] = 49000; cols["seg_len"][s] = 52000     # crosses 50 001 and 100 001
    spoil(cols, lens, [int(pick[3]), int(pick[4]), int(pick[5]), int(pick[6])])
    rec = records(rng, **cols)
    refs, ct_of = table(41, lens)
    engine.set_load_filter(60, 0, 0)
    try:
        fused_vs_oracle(engine, rec, lens, refs, ct_of, 2, CountParams.longsom_defaults())
    finally:
        engine.set_load_filter()


@pytest.mark.parametrize("n_contigs", [1, 25, 600])
def test_one_contig_a_few_dozen_and_hundreds(engine, n_contigs):
    lens = [9000] if n_contigs == 1 else [int(x) for x in np.random.default_rng(n_contigs).integers(700, 1500, n_contigs)]
    n = 4 * BATCH + 300                                           # a second batch of the admission pass
    rng, cols = sorted_case(50 + n_contigs, n, lens, seg_len=(20, 150))
    spoil(cols, lens, [4 * BATCH - 1, 4 * BATCH, n - 1])
    rec = records(rng, **cols)
    refs, ct_of = table(n_contigs, lens)
    engine.set_load_filter(60, 0, 0)
    try:
        fused_vs_oracle(engine, rec, lens, refs, ct_of, 2, CountParams.longsom_defaults(min_dp=0, min_cc=0))      # (600 contigs are shallow: no gates)
    finally:
        engine.set_load_filter()


def test_span_marks_of_a_read_whose_segments_lie_in_two_batches(engine):
    """the depth cap's bound: the +1 of a read's first segment and the -1 of its last come from neighbouring batches of the admission
    pass (segments 1023 and 1024) - the bound equals the numpy restatement, and it decides which loads may count in their own pass"""
    lens = [4000]
    rng = np.random.default_rng(61)
    R = 800
    nseg = np.full(R, 2); nseg[0] = 3                             # reads own (0,1,2), (3,4), ... (1023,1024), ...
    seg_read = np.repeat(np.arange(R), nseg).astype(np.uint32)
    assert seg_read[4 * BATCH - 1] == seg_read[4 * BATCH]
    start = np.sort(rng.integers(0, 2500, R))
    seg_start = np.concatenate([start[r] + 300 * np.arange(nseg[r]) for r in range(R)]).astype(np.int32)
    seg_len = rng.integers(30, 250, len(seg_read)).astype(np.int32)
    cb = rng.integers(0, N_CB, R).astype(np.int32); cb[rng.random(R) < 0.03] = -1
    rec = records(rng, np.zeros(R, np.int32), cb, np.zeros(R, np.uint16), np.full(R, 60, np.uint8), seg_read, seg_start, seg_len)
    refs, ct_of = table(61, lens)
    engine.set_contigs(lens); engine.load_reference(0, refs[0]); engine.set_barcodes(ct_of, 2)
    engine.load_reads(rec)
    has_cb = rec.read_cb >= 0
    ct_read = np.where(has_cb, ct_of[np.maximum(rec.read_cb, 0)], 255)
    bound_all = tile_bound(rec, lens, has_cb)[0]
    bound_ct = max(tile_bound(rec, lens, ct_read == ct)[0] for ct in range(2))
    assert engine.max_live_reads_all() == bound_all and engine.max_live_reads() == bound_ct > 8
    for max_depth, path in ((bound_ct // 3, 2), (2 * bound_all, 3)):        # under the bound the cap could fire: the count decides, not the load
        p = CountParams.longsom_defaults(); p.max_depth = max_depth
        engine.set_count_at_load(p)
        try:
            engine.load_reads(rec)
        finally:
            engine.set_count_at_load(None)
        assert engine.layout_info()[0] == path, max_depth
    fused_vs_oracle(engine, rec, lens, refs, ct_of, 2, CountParams.longsom_defaults())


def test_a_capped_count_of_a_sample_of_several_batches_equals_the_bam_level_oracle(engine, tmp_path):
    """the route of tests/test_depth_bound_gpu.py at a smaller size: BAM -> load -> count under a cap that bites, against oracle/plp_oracle.c"""
    from longsom_amd import hostio, pipeline, synth, tsvio
    from oracle import loader
    m = synth.named("C1", n_reads=3000, n_genes=5, n_cb=40, snp_mod=120)
    bam, fa, bct = str(tmp_path / "S1.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "barcodes.tsv")
    hostio.synth_bam(m, bam, fa)
    hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
    res = pipeline.load_sample(bam, bct, fa, engine, 60)
    assert engine.reads_shape()[1] > 4 * BATCH                    # more than one batch of the admission pass
    names, seqs = tsvio.read_fasta(fa)
    max_depth = 37
    assert engine.max_live_reads() > max_depth
    engine.pileup_count(CountParams.longsom_defaults(max_depth=max_depth))
    for ct in range(2):
        k, r, c = engine.fetch_counts(ct)
        ok, orf, oc = loader.plp_count(bam, res.table.barcodes, res.table.celltype_of, ct, [len(s) for s in seqs], seqs, max_depth=max_depth)
        assert np.array_equal(k, ok) and np.array_equal(r, orf) and np.array_equal(c, oc), "cell type %d" % ct
