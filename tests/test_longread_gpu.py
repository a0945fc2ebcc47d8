"""GPU: the device ingest, every form of the load, the count, the depth cap, the slices, the genotyping and the gene count on
long-read-shaped records (tests/support/longread_cases.py: 65 535 CIGAR operations in a record over seven or eight BGZF members, a 120 000-base
match, 400 exons with a 600 000-base intron, a 10 000-base deletion and a 5 000-base insertion on a contig filled to its last base).
Every comparison is exact.  References: the host decoder's arrays, the events-level oracle over them, and the BAM-level column oracle
(oracle/plp_oracle.c), which tests/test_longread_cpu.py shows to agree with each other on this file."""
import numpy as np
import pytest

from longsom_amd import genecounts, hostio
from longsom_amd._lib import CountParams, GenotypeParams
from oracle import loader
from tests.support import longread_cases as lc
from tests.test_count_gpu import run_both
from tests.test_fused_gpu import fused_vs_oracle
from tests.test_ingest_gpu import both_ways, slices_add_up

pytestmark = pytest.mark.gpu

DEFAULTS = (20, 60, 5, 5)                                     # CountParams.longsom_defaults(): min_bq, min_mq, min_dp, min_cc
LOOSE = (10, 30, 1, 1)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    c = lc.written(tmp_path_factory)
    c.first = hostio.bam_header(c.bam)[2]
    c.tables = {}                                             # the BAM-level oracle's tables, each made once
    c.records = {}
    return c


def plp(case, ct, p=DEFAULTS, legacy=False, max_depth=200000, window=lc.WINDOW):
    key = (ct, p, legacy, max_depth, window)
    if key not in case.tables:
        loader.plp_set_legacy_del_merge(legacy)
        try:
            case.tables[key] = loader.plp_count(case.bam, case.barcodes, case.celltype_of, ct, case.lens, case.refs, *p, max_depth=max_depth, window=window)
        finally:
            loader.plp_set_legacy_del_merge(False)
    return case.tables[key]


def host_records(case, min_mapq=60):
    if min_mapq not in case.records:
        case.records[min_mapq] = case.decoded(min_mapq).records
    return case.records[min_mapq]


def bind(engine, case, celltype_of=None, n_ct=2):
    engine.set_contigs(case.lens)
    for t, r in enumerate(case.refs):
        engine.load_reference(t, r)
    engine.set_barcodes(case.celltype_of if celltype_of is None else celltype_of, n_ct)
    engine.set_region()


def assert_rows(engine, case, p, what, **kw):
    """the resident load counted under p == the BAM-level oracle's table, per cell type; the first row that differs is named"""
    rows, _ = engine.pileup_count(CountParams.longsom_defaults(min_bq=p[0], min_mq=p[1], min_dp=p[2], min_cc=p[3], **({"max_depth": kw["max_depth"]} if "max_depth" in kw else {})))
    for ct in range(2):
        k, r, c = engine.fetch_counts(ct)
        ok, orf, oc = plp(case, ct, p, **kw)
        n = min(len(k), len(ok))
        bad = np.flatnonzero((k[:n] != ok[:n]) | (r[:n] != orf[:n]) | (c[:n] != oc[:n]).any(axis=1))
        at = int(bad[0]) if len(bad) else n
        assert len(bad) == 0 and len(k) == len(ok), "%s, cell type %d, %s: %d rows against the oracle's %d, first difference at row %d (device key %s, oracle key %s)" % (
            what, ct, p, len(k), len(ok), at, tuple(divmod(int(k[at]), 1 << 32)) if at < len(k) else None, tuple(divmod(int(ok[at]), 1 << 32)) if at < len(ok) else None)
    return rows


@pytest.mark.parametrize("form", ["phased", "compact", "legacy_del_merge"])
def test_ingest_three_ways(engine, case, form, monkeypatch):
    """device decoder == host decoder read for read and event for event (both_ways, with SplitBam's counters and tallies), and the device's
    count tables == the BAM-level oracle's under the defaults and under (10, 30, 1, 1)"""
    legacy = form == "legacy_del_merge"
    if form == "compact":
        monkeypatch.setenv("LSG_INGEST_COMPACT", "1")
    old = hostio.set_legacy_del_merge(legacy)
    try:
        info, dec = both_ways(engine, case.bam, case.barcodes, case.celltype_of, case.refs, min_mapq=60, compact=form == "compact")
        assert info["n_records"] == 80 and info["chain_rounds"] >= 2
        assert dec.records.n_segs > 7000 and np.bincount(dec.records.seg_read).max() >= 400
        # both_ways leaves the host decoder's arrays resident: the device decoder's own store against the column oracle
        info, _, _ = engine.load_bam(case.bam, case.barcodes, min_mapq=30, first_record_offset=case.first)
        assert info["n_records"] == 80
        rows = assert_rows(engine, case, DEFAULTS, "device ingest (%s)" % form, legacy=legacy)
        assert min(rows) >= 100_000
        assert_rows(engine, case, LOOSE, "device ingest (%s)" % form, legacy=legacy)
    finally:
        hostio.set_legacy_del_merge(old)


@pytest.mark.parametrize("n_ct", [2, 3])
def test_plain_load_of_the_decoded_arrays(engine, case, n_ct):
    """lsg_load_reads + the count over the store (k_tm_resolve, k_tm_walk) against the events-level oracle, two and three cell types"""
    rec = host_records(case)
    ct_of = case.celltype_of if n_ct == 2 else (np.arange(len(case.barcodes)) % 3).astype(np.uint8)
    rows, _ = run_both(engine, rec, case.lens, case.refs, ct_of, n_ct)
    assert min(rows) >= 50_000
    run_both(engine, rec, case.lens, case.refs, ct_of, n_ct, CountParams.longsom_defaults(min_bq=10, min_mq=30, min_dp=1, min_cc=1))


def test_fused_loads_of_the_decoded_arrays(engine, case):
    """the fused gather-count and a re-count of its store, the loads that keep no store (paths 4, 5 and 6) and the wrong-claim restart"""
    rec = host_records(case)
    fused_vs_oracle(engine, rec, case.lens, case.refs, case.celltype_of, 2, CountParams.longsom_defaults())


@pytest.mark.parametrize("depth", ["8", "below_the_bound"])
@pytest.mark.parametrize("window", [50_000, 1_000])
def test_the_depth_cap_replayed_per_window(engine, case, window, depth):
    """a read of 120 000 columns overlaps 3 or 4 windows of 50 000 ([1 + k W, 1 + (k + 1) W): one starts on a window's first column, one
    ends on a window's last, one has a single column in the window before) and 120 or 121 of 1 000, and is dropped in some and counted in
    others"""
    engine.set_pileup_window(window)
    try:
        bind(engine, case)
        engine.load_bam(case.bam, case.barcodes, min_mapq=60, first_record_offset=case.first)
        B = engine.max_live_reads_exact()
        assert B > 9
        free = assert_rows(engine, case, DEFAULTS, "no cap, window %d" % window, max_depth=0, window=window)
        if depth == "8":
            capped = assert_rows(engine, case, DEFAULTS, "max_depth 8, window %d" % window, max_depth=8, window=window)
            assert sum(capped) < sum(free)
        else:
            print("window %d: lsg_max_live_reads_exact = %d" % (window, B))
            assert_rows(engine, case, DEFAULTS, "max_depth B - 1 = %d, window %d" % (B - 1, window), max_depth=B - 1, window=window)
            assert assert_rows(engine, case, DEFAULTS, "max_depth B = %d, window %d" % (B, window), max_depth=B, window=window) == free
    finally:
        engine.set_pileup_window(50_000)


@pytest.mark.parametrize("world", [2, 3, 5])
def test_slices_add_up_and_one_needs_a_second_attempt(engine, case, monkeypatch, world):
    """regions.BaiPlan cuts chr1 inside many_exons' long intron: the slice before the cut ends on reads that start before it, its first
    guessed end (four index windows on) holds no record at or past the cut, and ingest_slice comes back with a longer one.  The attempts
    counted here are its host-side checks of the guess (_last_key_of_block) followed by one device ingest; the repeat of the device ingest
    itself (last_key short of the region's end after a load) is reached by no file of the suite"""
    from longsom_amd import regions
    attempts = []
    real = regions.ingest_slice

    def noting(engine, bam, plan, lo, hi, barcodes, min_mapq):
        got = real(engine, bam, plan, lo, hi, barcodes, min_mapq)
        if got is not None:
            attempts.append((lo, hi, got[0]["attempts"]))
        return got
    monkeypatch.setattr(regions, "ingest_slice", noting)
    slices_add_up(engine, case.bam, case.barcodes, case.celltype_of, case.refs, world)
    for lo, hi, n in attempts:
        print("world %d: region %s..%s took %d attempt(s)" % (world, lo, hi, n))
    assert len(attempts) >= 2 and max(n for _, _, n in attempts) >= 2


def genotype_sites(case):
    """about 100 target sites, ascending keys (tid << 32 | pos0), with the symbol class expected at each"""
    rng = np.random.default_rng(77)
    lm = case.by_family["long_match"]
    ex = case.cigars["many_exons_n_then_i"]
    p0 = case.by_family["many_exons"][2]["pos"]                  # a copy that carries N followed by I
    x, intron, before_ni = p0, None, None
    for i, (op, l) in enumerate(ex):
        if op == "N" and intron is None and l < lc.LONG_INTRON:
            intron = x + l // 2
        if op == "N" and i + 1 < len(ex) and ex[i + 1][0] == "I" and before_ni is None:
            before_ni = [x - 1, x + l - 1, x + l]                 # the exon's last column, the intron's last column (it carries the I), the next exon's first
        if op in "MN":
            x += l
    chr1 = [r["pos"] for r in lm] + [r["pos"] + 120_000 - 1 for r in lm] + [r["pos"] - 1 for r in lm[:2]] + [r["pos"] + 120_000 for r in lm[:2]]
    chr1 += [intron] + before_ni + [p0 + case.by_family["many_exons"][0]["ref_len"] - 1, lc.WINDOW - 1, 2 * lc.WINDOW - 1, 2 * lc.WINDOW]
    chr1 += [int(v) for v in rng.integers(case.spans["max_cigar"][1], case.spans["max_cigar"][2], 30)]
    chr1 += [int(v) for v in rng.integers(case.spans["many_exons"][1] + 700_000, case.spans["many_exons"][2], 20)]
    chrm = [0, 49, 50, 5_000, 10_049, 10_050, 10_088, 10_089, 10_090, 10_091, 15_998, 15_999]    # D = [50, 10 050), the I behind column 10 089
    keys = np.array(sorted(set((0 << 32) | p for p in chr1) | set((1 << 32) | p for p in chrm)), np.int64)
    return keys, rng.integers(0, 7, len(keys)).astype(np.uint8)


@pytest.mark.parametrize("kw", [dict(), dict(min_bq=0, min_mq=0, strict_cb=0)])
def test_genotype_at_sites_inside_the_long_reads(engine, case, kw):
    from oracle import genotype_oracle as go
    keys, alt = genotype_sites(case)
    assert 90 <= len(keys) <= 130
    bind(engine, case)
    engine.load_bam(case.bam, case.barcodes, min_mapq=0, first_record_offset=case.first)
    rec = host_records(case, 0)
    p = GenotypeParams.longsom_defaults(**kw)
    dp, al = engine.genotype_cells(keys, alt, p)
    odp, oal = go.genotype(rec, case.lens, case.celltype_of, keys, alt, p.min_bq, p.min_mq, p.flag_exclude, p.ignore_orphans, p.alt_only, p.strict_cb)
    np.testing.assert_array_equal(dp, odp); np.testing.assert_array_equal(al, oal)
    assert dp.sum() > 500 and 0 < al.sum() < dp.sum()
    assert dp[keys == ((1 << 32) | 15_999)].sum() > 0 and dp[keys == ((1 << 32) | 0)].sum() > 0 and dp[keys == lc.WINDOW].sum() > 0
    assert dp[keys == ((1 << 32) | 5_000)].sum() == 0                                            # inside the deletion: 'O' is no base
    window = 5_000
    code = (keys >> 32) * (1 << 40) + ((keys & 0xFFFFFFFF) + 1) // window
    group_off = np.concatenate([[0], np.nonzero(np.diff(code))[0] + 1, [len(keys)]]).astype(np.int64)
    gdp, gal = engine.genotype_cells_grouped(keys, alt, group_off, p, 8)
    odp8, oal8 = go.genotype(rec, case.lens, case.celltype_of, keys, alt, p.min_bq, p.min_mq, p.flag_exclude, p.ignore_orphans, p.alt_only, p.strict_cb,
                             group_off=group_off, max_depth=8)
    np.testing.assert_array_equal(gdp, odp8); np.testing.assert_array_equal(gal, oal8)
    assert gdp.sum() < dp.sum()                                                                  # the cap really dropped reads


def annotation(case, n_under):
    """2 500 disjoint exons of n_under genes under the long match (every 60 columns, 30 long), a gene per 10 blocks of many_exons with every
    fourth one reaching into its neighbour's first block (ambiguous intervals), one gene over chrM"""
    gene, contig, s0, e0 = [], [], [], []
    for i in range(2500):
        gene.append(i % n_under); contig.append("chr1"); s0.append(50_000 + 60 * i); e0.append(50_000 + 60 * i + 30)
    x, blocks = case.by_family["many_exons"][0]["pos"], []
    for op, l in case.cigars["many_exons"]:
        if op == "M":
            blocks.append((x, x + l))
        x += l
    far = [b for b in blocks if b[0] > 700_000]                                                   # behind the long intron: clear of the exons above
    for g in range(len(far) // 10):
        own = far[10 * g:10 * g + 10] + (far[10 * g + 10:10 * g + 11] if g % 4 == 0 else [])
        for a, b in own:
            gene.append(n_under + g); contig.append("chr1"); s0.append(a); e0.append(b)
    n_genes = n_under + len(far) // 10 + 1
    gene.append(n_genes - 1); contig.append("chrM"); s0.append(10_060); e0.append(10_080)       # between the deletion and the insertion
    ex = genecounts.Exons(["LRG%03d" % g for g in range(n_genes)], np.asarray(gene, np.int64), contig, np.asarray(s0, np.int64), np.asarray(e0, np.int64))
    return genecounts.flatten(ex, [n for n, _ in case.contigs])


@pytest.mark.parametrize("n_under,min_mapq,flag_exclude", [(1, 0, 0x4), (50, 30, 0x904)])
def test_gene_counts_under_segments_that_cover_thousands_of_intervals(engine, case, n_under, min_mapq, flag_exclude):
    """one gene under the long match: its reads are assigned through a segment over 2 000 intervals; fifty genes: they are ambiguous"""
    ann = annotation(case, n_under)
    assert ann.n_intervals >= 2500 and (ann.labels == genecounts.AMBIG).any()
    rows, row_of_gene = genecounts.rows_of(ann.gene_ids, None)
    order = genecounts.column_order(case.barcodes)
    rec = host_records(case, 0)
    matrix, tallies = genecounts.count(rec, ann, row_of_gene, len(rows), len(case.barcodes), min_mapq, flag_exclude)
    text = genecounts.matrix_text(matrix, rows, case.barcodes, order)
    t = tallies.sum(axis=0)
    assert t[0] > 10 and t[2] > 10 and (min_mapq == 0 or t[3] > 0)                               # assigned, ambiguous, and filtered where a filter is set
    bind(engine, case)
    engine.gene_counts_reset()
    try:
        for how in ("device ingest", "host arrays"):
            if how == "device ingest":
                engine.load_bam(case.bam, case.barcodes, min_mapq=0, first_record_offset=case.first)
            else:
                engine.load_reads(rec)
            engine.gene_counts_reset()
            engine.load_annotation(ann, row_of_gene, len(rows))
            info = engine.gene_counts(min_mapq, flag_exclude)
            engine.gene_counts_set_text(rows, order, case.barcodes, ",")
            n = engine.format_table(engine.TABLE_GENE_COUNTS)
            got_m, got_t = engine.gene_counts_fetch()
            np.testing.assert_array_equal(got_m.astype(np.int64), matrix, err_msg=how)
            np.testing.assert_array_equal(got_t.astype(np.int64), tallies, err_msg=how)
            assert engine.table_bytes(engine.TABLE_GENE_COUNTS, n) == text, how
            assert [info[k] for k in ("n_assigned", "n_no_features", "n_ambiguity", "n_filtered")] == t.tolist()
    finally:
        engine.gene_counts_reset()
