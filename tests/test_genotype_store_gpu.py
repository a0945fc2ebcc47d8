"""GPU: the genotyping site kernel (genotype.hip k_geno_sites) over every store a load can leave it, against the events-level oracle
(oracle/genotype_oracle.py), bit for bit: tiles deep enough for several trips of the block loop and for multi-job tiles, stores written
by the plain gather (store.hip) and by the fused one (pileup.hip), from compact and from tile-phased events, under a load filter, a
region, other numbers of cell types, a re-annotated table and a capped count; the depth cap's replay at its edges; lsg_cellgeno_count's
counts; and the refusals, after which the handle still works.  The cases are tests/support/geno_cases.py, pinned on the CPU by
tests/test_genotype_cases_cpu.py."""
import hashlib

import numpy as np
import pytest

from longsom_amd import hostio, synth
from longsom_amd._lib import CountParams, GenotypeParams
from tests.support import geno_cases as gc
from tests.support.synth_simple import random_reference
from tests.util import phased_records

pytestmark = pytest.mark.gpu

PARAMS = (dict(), dict(alt_only=1), dict(strict_cb=0, min_bq=0), dict(min_mq=0, ignore_orphans=0, min_bq=45))
STRICT = (60, 0xF04, 1)                                # the load filter of the rules' own read filters
_oracle_cache = {}


def oracle(rec, lens, ct_of, keys, alt, p, group_off=None, max_depth=0):
    """go.genotype, computed once per (records, table, sites, parameters, groups, cap)"""
    from oracle import genotype_oracle as go
    h = hashlib.sha1()
    for a in (rec.read_tid, rec.read_pos, rec.read_flag, rec.read_mapq, rec.read_cb, rec.seg_start, rec.seg_ev_off, np.asarray(lens, np.int64),
              np.asarray(ct_of, np.uint8), np.asarray(keys, np.int64), np.asarray(alt, np.uint8), np.asarray([] if group_off is None else group_off, np.int64)):
        h.update(a.tobytes()); h.update(b"|")
    k = (h.hexdigest(), p.min_bq, p.min_mq, p.flag_exclude, p.ignore_orphans, p.alt_only, p.strict_cb, int(max_depth))
    if k not in _oracle_cache:
        _oracle_cache[k] = go.genotype(rec, lens, ct_of, keys, alt, p.min_bq, p.min_mq, p.flag_exclude, p.ignore_orphans, p.alt_only, p.strict_cb,
                                       group_off=group_off, max_depth=max_depth)
    return _oracle_cache[k]


def geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, params_list=PARAMS):
    out = []
    for kw in params_list:
        p = GenotypeParams.longsom_defaults(**kw)
        dp, al = engine.genotype_cells(keys, alt, p)
        odp, oal = oracle(rec, lens, ct_of, keys, alt, p)
        assert dp.shape == (len(keys), len(ct_of))
        np.testing.assert_array_equal(dp, odp, err_msg=str(kw)); np.testing.assert_array_equal(al, oal, err_msg=str(kw))
        out.append((dp, al))
    assert out[0][0].sum() > 0
    return out


def refs_of(lens):
    rng = np.random.default_rng(99)
    return [random_reference(rng, int(L)) for L in lens]


def load(engine, rec, lens, ct_of, n_ct=2, count=None, load_filter=(0, 0, 0), region=None, hint=False):
    """one load that keeps a store, under exactly the settings given (the session's engine gets its defaults back); count: a CountParams -
    the load also makes that count (lsg_set_count_at_load).  Returns the path the load took."""
    engine.set_contigs(lens)
    for t, r in enumerate(refs_of(lens)):
        engine.load_reference(t, r)
    engine.set_barcodes(ct_of, n_ct)
    engine.set_region(*(region or ()))
    engine.set_pileup_window(50000)
    saved = engine.load_settings()
    engine.set_load_filter(*load_filter)
    engine.set_store_policy(engine.STORE_KEEP)
    engine.set_count_at_load(count)
    engine.set_events_layout(engine.LAYOUT_PHASED if hint else engine.LAYOUT_COMPACT)
    try:
        engine.load_reads(rec)
    finally:
        engine.set_events_layout(engine.LAYOUT_COMPACT)
        engine.restore_load_settings(saved)
    return engine.layout_info()[0]


@pytest.fixture
def whole_region(engine):
    yield
    engine.set_region()


# ---- a. deep tiles --------------------------------------------------------------------------------------------------------------------
def test_deep_tiles_before_and_after_the_first_count(engine):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    assert load(engine, rec, lens, ct_of) == 2
    first = geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)          # no count was made of this load: the plan's second half does not exist
    engine.pileup_count(CountParams.longsom_defaults())
    assert engine.count_stats().n_deep_units > 0
    again = geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)
    for (a, b), (c, d) in zip(first, again):
        np.testing.assert_array_equal(a, c); np.testing.assert_array_equal(b, d)
    deep = geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, (dict(min_mq=0),))[0][0]
    assert deep.sum() == gc.DEEP_FREE_SUM and deep[:, 0].max() > 1000         # one cell deep enough to pile atomics on one word
    assert (first[1][0] == first[1][1]).all()                                 # alt_only: Dp is Alt
    p = GenotypeParams.longsom_defaults()
    total = np.zeros_like(first[0][0])
    for sym in range(7):                                                      # every site asked for every alt class in turn
        one = np.full(len(keys), sym, np.uint8)
        dp, al = engine.genotype_cells(keys, one, p)
        odp, oal = oracle(rec, lens, ct_of, keys, one, p)
        np.testing.assert_array_equal(dp, odp); np.testing.assert_array_equal(al, oal)
        np.testing.assert_array_equal(dp, first[0][0])
        assert al.sum() > 0
        total += al
    np.testing.assert_array_equal(total, first[0][0])                         # the seven Alt arrays sum to Dp
    dp, al = engine.genotype_cells(keys, np.full(len(keys), 7, np.uint8), p)
    np.testing.assert_array_equal(dp, first[0][0])
    assert not al.any()                                                       # 'O' is no alt


# ---- b. every form of a load that keeps a store ---------------------------------------------------------------------------------------
def test_plain_load_of_compact_events(engine):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    rec = gc.with_cb_suffix(rec)                                              # (strict_cb has reads to leave out)
    assert load(engine, rec, lens, ct_of) == 2
    out = geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)
    assert out[2][0].sum() > out[0][0].sum()


@pytest.mark.parametrize("form", ["phased", "phased, claimed", "compact, claimed phased"])
def test_plain_load_of_phased_events(engine, form):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    if form != "compact, claimed phased":
        rec = phased_records(rec)
    assert load(engine, rec, lens, ct_of, hint="claimed" in form) == 2       # (a wrong claim is found out: the load falls back)
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)


@pytest.mark.parametrize("form", ["compact", "phased"])
def test_fused_load(engine, form):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    if form == "phased":
        rec = phased_records(rec)
    p = CountParams.longsom_defaults()
    assert load(engine, rec, lens, ct_of, count=p) == 3
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)
    engine.pileup_count(p)                                                    # the count the load made is handed out
    assert engine.count_stats().n_deep_units > 0
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, PARAMS[:1])


def test_fused_load_under_a_region_leaves_a_whole_store(engine, whole_region):
    """the region ends between the two deep tiles (position 1088 = tile 17; regions are made of whole tiles): tile 17 and everything behind
    it is gathered and not counted, and the genotyping pass reads sites on both sides"""
    rec, lens, ct_of, keys, alt = gc.deep_case()
    assert gc.key(0, 1087) in keys and gc.key(0, 1088) in keys and (keys >> 32).max() == 3
    assert load(engine, rec, lens, ct_of, count=CountParams.longsom_defaults(), region=(0, 0, 0, 1088)) == 3
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)


@pytest.mark.parametrize("fused", [False, True])
def test_store_built_under_the_strict_load_filter(engine, fused):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    count = CountParams.longsom_defaults(min_mq=STRICT[0], flag_exclude=STRICT[1], ignore_orphans=STRICT[2]) if fused else None
    assert load(engine, rec, lens, ct_of, count=count, load_filter=STRICT) == (3 if fused else 2)
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, PARAMS[:3] + (dict(min_bq=45), dict(min_mq=61, flag_exclude=0xF05)))


def test_store_built_under_a_loose_load_filter(engine):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    assert load(engine, rec, lens, ct_of, load_filter=(30, 0, 0)) == 2
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, PARAMS[:3] + (dict(min_mq=30, ignore_orphans=0, min_bq=45),))


@pytest.mark.parametrize("n_ct", [1, 3, 4])
def test_other_numbers_of_cell_types(engine, n_ct):
    rec, lens, _, keys, alt = gc.deep_case()
    ct_of = (np.arange(gc.N_CB) % n_ct).astype(np.uint8)
    assert load(engine, rec, lens, ct_of, n_ct=n_ct) == 2
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)
    assert load(engine, rec, lens, ct_of, n_ct=n_ct, count=CountParams.longsom_defaults()) == (3 if n_ct == 1 else 2)
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)


def test_reannotation_without_a_reload(engine):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    load(engine, rec, lens, ct_of)
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, PARAMS[:1])
    perm = ct_of[np.random.default_rng(3).permutation(len(ct_of))]
    assert (perm != ct_of).any() and perm[0] != 255
    engine.set_barcodes(perm, 2)
    geno_equals_oracle(engine, rec, lens, perm, keys, alt)
    short = ct_of[:63].copy()                                                 # the store's reads of barcodes 63..69 count nowhere
    assert (rec.read_cb >= 63).sum() > 100
    engine.set_barcodes(short, 2)
    out = geno_equals_oracle(engine, rec, lens, short, keys, alt)
    assert out[0][0].shape == (len(keys), 63)


def test_device_arrays(engine):
    m = synth.named("C1", n_reads=3000, n_genes=20, n_cb=30, snp_mod=300)
    rec = hostio.synth_records(m)
    tid = int(rec.read_tid[0])
    cover = np.zeros(int(m.contig_len[tid]) + 1, np.int64)
    np.add.at(cover, rec.seg_start[rec.read_tid[rec.seg_read] == tid], 1)
    np.add.at(cover, (rec.seg_start + rec.seg_len)[rec.read_tid[rec.seg_read] == tid], -1)
    pos = np.sort(np.argsort(np.cumsum(cover)[:-1])[-12:])                     # the best covered positions of the first contig with reads
    keys = (np.int64(tid) << 32) | pos.astype(np.int64)
    alt = (np.arange(len(keys)) % 7).astype(np.uint8)
    engine.set_contigs(m.contig_len); engine.set_barcodes(m.celltype_of, 2); engine.set_region()
    g = engine.synth_generate(m)
    assert g.on_device == 1 and g.n_reads == rec.n_reads
    engine.load_reads_struct(g)
    geno_equals_oracle(engine, rec, m.contig_len, m.celltype_of, keys, alt)


def test_a_capped_count_does_not_leak_its_drops(engine):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    load(engine, rec, lens, ct_of)
    assert engine.max_live_reads() > 37
    free_cols = engine.pileup_count(CountParams.longsom_defaults())[1]
    assert engine.pileup_count(CountParams.longsom_defaults(max_depth=37))[1] <= free_cols      # the count has marked its drops
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt)
    p = GenotypeParams.longsom_defaults(min_mq=0)
    g = gc.window_groups(keys, 150)
    dp, al = engine.genotype_cells_grouped(keys, alt, g, p, 50)
    odp, oal = oracle(rec, lens, ct_of, keys, alt, p, g, 50)
    np.testing.assert_array_equal(dp, odp); np.testing.assert_array_equal(al, oal)
    assert dp.sum() == gc.DEEP_CAP_SUMS[150, 50]


# ---- c. the depth cap -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", gc.WINDOWS)
@pytest.mark.parametrize("case", ["deep_case", "sorted_deep_case"])
def test_depth_cap_on_deep_windows(engine, case, window):
    rec, lens, ct_of, keys, alt = getattr(gc, case)()
    load(engine, rec, lens, ct_of)
    p = GenotypeParams.longsom_defaults(min_mq=0)
    g = gc.window_groups(keys, window)
    free_dp, free_al = engine.genotype_cells(keys, alt, p)
    assert free_dp.sum() == gc.DEEP_FREE_SUM
    B = engine.max_live_reads_all() + 1                                       # run_genotype replays the cap when max_live_all + 1 > max_depth
    assert B - 1 > 3000
    for max_depth in gc.DEEP_DEPTHS + (B - 1, B):
        dp, al = engine.genotype_cells_grouped(keys, alt, g, p, max_depth)
        odp, oal = oracle(rec, lens, ct_of, keys, alt, p, g, max_depth)
        np.testing.assert_array_equal(dp, odp, err_msg=str(max_depth)); np.testing.assert_array_equal(al, oal, err_msg=str(max_depth))
        if max_depth in gc.DEEP_DEPTHS:
            assert dp.sum() == gc.DEEP_CAP_SUMS[window, max_depth] < free_dp.sum()       # the cap really dropped reads, on the device too
    np.testing.assert_array_equal(dp, free_dp); np.testing.assert_array_equal(al, free_al)      # at B nothing is replayed


@pytest.mark.parametrize("kw", list(gc.CAP_EDGE_SUMS), ids=["defaults", "min_mq 0, orphans kept"])
def test_depth_cap_at_the_edges_of_the_replay(engine, kw):
    rec, lens, ct_of, keys, alt = gc.cap_edge_case()
    load(engine, rec, lens, ct_of)
    p = GenotypeParams.longsom_defaults(**dict(kw))
    g = gc.cap_edge_groups()
    sums = gc.CAP_EDGE_SUMS[kw]
    dp, al = engine.genotype_cells(keys, alt, p)
    odp, oal = oracle(rec, lens, ct_of, keys, alt, p)
    np.testing.assert_array_equal(dp, odp); np.testing.assert_array_equal(al, oal)
    assert dp.sum() == sums[0]
    assert engine.max_live_reads_all() + 1 > 3                                # every cap below is replayed
    for max_depth in (1, 2, 3):
        dp, al = engine.genotype_cells_grouped(keys, alt, g, p, max_depth)
        odp, oal = oracle(rec, lens, ct_of, keys, alt, p, g, max_depth)
        np.testing.assert_array_equal(dp, odp, err_msg=str(max_depth)); np.testing.assert_array_equal(al, oal, err_msg=str(max_depth))
        assert dp.sum() == sums[max_depth] < sums[0]


# ---- d. lsg_cellgeno_count ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_cellgeno_count_counts_what_the_oracle_counts(engine, fused):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    assert load(engine, rec, lens, ct_of, count=CountParams.longsom_defaults() if fused else None) == (3 if fused else 2)
    p = GenotypeParams.longsom_defaults(strict_cb=0, min_mq=0)
    g = gc.window_groups(keys, 150)
    for max_depth in (50, 200000):
        engine.cellgeno_count(keys, alt, np.zeros(len(keys), np.uint8), g, p, max_depth)
        got = engine.cellgeno_fetch()
        odp, oal = oracle(rec, lens, ct_of, keys, alt, p, g, max_depth)
        np.testing.assert_array_equal(got["dp"], odp); np.testing.assert_array_equal(got["alt"], oal)
        np.testing.assert_array_equal(got["n_covered"], (odp > 0).sum(axis=0))
        assert got["dp"].sum() == (gc.DEEP_CAP_SUMS[150, 50] if max_depth == 50 else gc.DEEP_FREE_SUM)


# ---- e. refusals leave the handle usable ----------------------------------------------------------------------------------------------
def test_read_filters_looser_than_the_load_filter_are_refused(engine):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    load(engine, rec, lens, ct_of, load_filter=STRICT)
    g = gc.window_groups(keys, 150)
    chrm = np.zeros(len(keys), np.uint8)
    good = GenotypeParams.longsom_defaults()
    for kw in (dict(min_mq=30), dict(flag_exclude=0x704)):
        bad = GenotypeParams.longsom_defaults(**kw)
        for call in (lambda q: engine.genotype_cells(keys, alt, q), lambda q: engine.genotype_cells_grouped(keys, alt, g, q, 50),
                     lambda q: engine.cellgeno_count(keys, alt, chrm, g, q, 50)):
            with pytest.raises(RuntimeError, match="load filter"):
                call(bad)
            geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, PARAMS[:1])
    dp, al = engine.genotype_cells_grouped(keys, alt, g, good, 50)
    odp, oal = oracle(rec, lens, ct_of, keys, alt, good, g, 50)
    np.testing.assert_array_equal(dp, odp); np.testing.assert_array_equal(al, oal)


def test_bad_groups_and_an_unloaded_handle_are_refused(engine):
    rec, lens, ct_of, keys, alt = gc.deep_case()
    load(engine, rec, lens, ct_of)
    p = GenotypeParams.longsom_defaults()
    n = len(keys)
    n0 = int((keys >> 32 == 0).sum())
    assert engine.max_live_reads_all() + 1 > 50                               # run_genotype looks at the groups only when it replays the cap
    for group_off, message in (([0, n0 + 1, n], "spans two contigs"), ([0, 5, 3, n], "ascending"), ([0, 5, n + 2], "cover the sites"), ([1, 5, n], "cover the sites")):
        with pytest.raises(RuntimeError, match=message):
            engine.genotype_cells_grouped(keys, alt, np.array(group_off, np.int64), p, 50)
        geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, PARAMS[:1])
    with pytest.raises(RuntimeError, match="spans two contigs"):
        engine.cellgeno_count(keys, alt, np.zeros(n, np.uint8), np.array([0, n0 + 1, n], np.int64), p, 50)
    g = gc.window_groups(keys, 150)
    dp, al = engine.genotype_cells_grouped(keys, alt, g, p, 50)
    odp, oal = oracle(rec, lens, ct_of, keys, alt, p, g, 50)
    np.testing.assert_array_equal(dp, odp); np.testing.assert_array_equal(al, oal)
    engine.unload_reads()
    for call in (lambda: engine.genotype_cells(keys, alt, p), lambda: engine.genotype_cells_grouped(keys, alt, g, p, 50),
                 lambda: engine.cellgeno_count(keys, alt, np.zeros(n, np.uint8), g, p, 50)):
        with pytest.raises(RuntimeError, match="no reads loaded"):
            call()
    load(engine, rec, lens, ct_of)
    geno_equals_oracle(engine, rec, lens, ct_of, keys, alt, PARAMS[:1])
