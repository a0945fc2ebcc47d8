"""GPU: the peripheral kernels whose grid is capped at a multiple of the CU count, on inputs past twice the cap, so that every worker makes
two trips through its loop and some make three (tests/support/grid_caps.py has the table of the caps and of who tests what).  Every size
comes from the device's CU count; every comparison is exact, against the same twins and references the kernels' own modules use
(hostio.bam_fastq, bnpc._Host and scipy's linkage, scipy's betabinom through reference_cell, the golden tail table, bbfit.histograms),
except the branch-2 means of the BnpC estimate, which keep their module's bound.  What a later trip decides is asserted to be there:
printed records, used samples, kept rows behind the first trip, and expected values that differ from those one stride earlier (a trip
that read the first trip's items again would not pass)."""
import json
import os
import time

import numpy as np
import pytest

from longsom_amd import bbfit, bnpc, hostio
from tests.support import bamwrite, fastq_cases as fc
from tests.support import grid_caps as gc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INFO_KEYS = ("n_records", "n_printed", "n_bytes", "bad_ordinal", "bad_kind")


def cap_of(kernel, cu):
    caps = {e.cap(cu) for e in gc.LAUNCHES if e.kernel == kernel and e.test}
    assert len(caps) == 1, kernel
    return caps.pop()


def sized(kernel, n, cap):
    """the common preconditions, and the line every test prints"""
    assert n > 2 * cap and n % cap != 0, (kernel, n, cap)
    print("%s: %d items, cap %d at %d CUs, %d trips for the busiest worker" % (kernel, n, cap, gc.cu_count(), gc.trips(n, cap)))


def where(i, cap):
    return "index %d (trip %d of its worker)" % (i, i // cap + 1)


def same_everywhere(name, got, want, cap):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, name
    bad = np.flatnonzero(got != want)
    assert not len(bad), "%s differs at %d of %d items, first at %s: got %s, want %s" % (name, len(bad), len(want), where(int(bad[0]), cap), got[bad[0]], want[bad[0]])


def differs_from_a_stride_earlier(name, want, cap):
    """the expected values are not those of the items one trip earlier"""
    want = np.asarray(want).ravel()
    assert np.count_nonzero(want[cap:] != want[:-cap]) > len(want) // 100, name


def repeated(period, n, cap):
    """n indices into a pattern of `period` items: the pattern over and over, rotated by one item per repeat if its period divides the stride"""
    i = np.arange(n, dtype=np.int64)
    if cap % period == 0:
        i = i + i // period
    idx = i % period
    assert cap % period != 0 or np.any(idx[cap:] != idx[:-cap])
    return idx


# ---- k_fq_print: a wave per record ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    """past(32 CUs x 4 waves, 5) fuzzed records of 0 .. 40 bases, written once: (records, the BAM, the barcode table, the cap)"""
    cap = cap_of("k_fq_print", gc.cu_count())
    n = gc.past(cap, 5)
    t0 = time.time()
    recs = fc.fuzz_records(n, max_len=40)
    assert {0 if r["seq"] == "*" else len(r["seq"]) for r in recs} == set(range(41))
    assert any(r["qual"] for r in recs) and any(not r["qual"] and r["seq"] != "*" for r in recs) and any(r["tid"] < 0 for r in recs)
    bam = str(tmp_path_factory.mktemp("caps") / "fuzz.bam")
    bamwrite.write_bam(bam, [("chr1", 10 * n + 100), ("chr2", 90000)], recs)       # fuzz_records puts record k at 10 k: a contig that holds them all
    print("fuzz: %d records written in %.1f s, %d bytes" % (n, time.time() - t0, os.path.getsize(bam)))
    table = hostio.BarcodeTable(list(fc.FUZZ_BARCODES), np.asarray(fc.FUZZ_CELLTYPE_OF, np.uint8), ["Cancer", "Non-Cancer"])
    return recs, bam, table, cap


def blocks_of(text):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [lines[k:k + 4] for k in range(0, len(lines) - 1, 4)]


def compare_fastq(dev, text, host, want, cap):
    assert {k: dev[k] for k in INFO_KEYS} == {k: host[k] for k in INFO_KEYS}
    if text != want:                                              # name the first printed record that differs
        assert len(text) == len(want)
        diff = np.flatnonzero(np.frombuffer(text, np.uint8) != np.frombuffer(want, np.uint8))
        k = int(diff[0])
        pytest.fail("device FASTQ differs from the host twin's in %d bytes, first at byte %d: printed record %d of %d (a wave's first trip ends at %d): %r / %r" % (
            len(diff), k, want[:k].count(b"\n") // 4, want.count(b"\n") // 4, cap, text[max(k - 20, 0):k + 20], want[max(k - 20, 0):k + 20]))


def lowest_indices(blocks, recs):
    """a lower bound on the file index of every printed record: within one text the records come in file order, so each block is
    matched to the first later record with its name and bases"""
    out, at = [], 0
    for header, seq, _, _ in blocks:
        name = header.rsplit(b"^", 1)[1].decode()
        while recs[at]["name"] != name or recs[at]["seq"].encode() != seq:
            at += 1
        out.append(at)
        at += 1
    return out


def test_fastq_print_past_the_cap(engine, fuzz, tmp_path):
    """Plain mode, then routed mode twice over the same BAM.  Under min_mapq 10 and --max_nM 1 the fuzz's barcodes, MAPQs and nM tags
    route a seventh of the records (4 733 + 4 793 of 65 541 at 256 CUs): fewer than one trip's worth, so what is asserted there is that
    each cell type prints records behind every wave's first trip.  With min_mapq 0 and no limit the barcode list alone routes 45 442,
    and the two cell types print more than the cap's worth between them."""
    recs, bam, table, cap = fuzz
    n = len(recs)
    sized("k_fq_print", n, cap)
    h = str(tmp_path / "h.fastq")

    def device(tab, min_mapq):
        info = engine.bam_fastq(bam, None if tab is None else tab.barcodes, None if tab is None else tab.celltype_of, 0 if tab is None else len(tab.celltype_names), min_mapq)
        return info, engine.table_bytes(engine.TABLE_FASTQ, sum(info["n_bytes"]))

    # plain mode: every record, the last one (a third trip's) included
    host = hostio.bam_fastq(bam, h)
    with open(h, "rb") as f:
        want = f.read()
    dev, text = device(None, 60)
    compare_fastq(dev, text, host, want, cap)
    last = blocks_of(want)[-1]
    assert dev["n_printed"][0] == n and last[0].endswith(b"^" + recs[-1]["name"].encode()) and last[1] == recs[-1]["seq"].encode()
    assert blocks_of(text)[-1] == last
    # routed mode: the issue's filters, which let a seventh of the records through, then none but the barcode list, which lets more than
    # the cap's worth through
    for min_mapq, filters in ((10, hostio.SplitFilters(max_nM=1)), (0, None)):
        host = hostio.bam_fastq(bam, h, table, min_mapq, filters)
        with open(h, "rb") as f:
            want = f.read()
        engine.set_split_filters(filters)
        try:
            dev, text = device(table, min_mapq)
        finally:
            engine.set_split_filters(None)
        compare_fastq(dev, text, host, want, cap)
        n0, n1 = dev["n_printed"][:2]
        print("routed (min_mapq %d, %s): %d + %d records printed" % (min_mapq, filters, n0, n1))
        blocks = blocks_of(want)
        assert len(blocks) == n0 + n1 and n0 > 0 and n1 > 0
        for part in (blocks[:n0], blocks[n0:]):              # both cell types print records no wave reaches in its first trip
            assert lowest_indices(part, recs)[-1] >= cap
        if filters is None:
            assert n0 + n1 > cap


# ---- k_bnpc_pack, k_bnpc_criteria, k_bnpc_cluster_counts: the BnpC estimate over ~32 800 samples -----------------------------------------
def test_bnpc_estimate_past_the_caps(engine):
    from scipy.cluster.hierarchy import linkage
    from tests.test_bnpc_gpu import generated
    cu = gc.cu_count()
    N, K, pitch = 65, 4, 128
    cap_pack, cap_crit, cap_cnt = cap_of("k_bnpc_pack", cu), cap_of("k_bnpc_criteria", cu), cap_of("k_bnpc_cluster_counts", cu)
    S = -(-gc.past(cap_pack, 37 * pitch) // pitch)
    sized("k_bnpc_pack", S * pitch, cap_pack)
    sized("k_bnpc_cluster_counts", S, cap_cnt)
    sized("k_bnpc_criteria", S, cap_crit)
    t0 = time.time()
    a, p = generated(N * 1000 + S, N, S, K)
    host = bnpc._Host(a, p)
    want_D = host.codist()
    print("twin: %d samples generated and measured in %.1f s" % (S, time.time() - t0))
    engine.bnpc_load_samples(a, p)
    try:
        avg, want_avg = engine.bnpc_avg_cluster_number(), bnpc.avg_cluster_number(a)
        assert isinstance(avg, np.float64) and avg == want_avg, "k_bnpc_cluster_counts: %r, numpy %r over %d samples" % (avg, want_avg, S)
        D = engine.bnpc_codist()
        assert np.array_equal(D, want_D)                                            # (reads every packed label: k_bnpc_pack's later trips)
        rng = np.random.default_rng(S)
        cuts = np.stack([rng.integers(0, 1 + k % N, N) for k in range(7)])
        pairs, sim, dsum = engine.bnpc_mpear(cuts)
        hp, hs, hd = host.mpear_sums(cuts)
        assert np.array_equal(pairs, hp) and np.array_equal(sim, hs) and dsum == hd
        Z, want_Z = engine.bnpc_linkage(), linkage(D / S, method="ward")
        assert Z.shape == want_Z.shape and np.array_equal(Z.view(np.uint64), want_Z.view(np.uint64))
        random = rng.integers(0, K, N)
        random[0] = K                                                               # a one-cell cluster
        branches, later = set(), False
        for final in (a[0], random):
            got, hw = engine.bnpc_mean_params(final), host.mean_params(final)
            for what, g, w in (("branch", got[1], hw[1]), ("n_used", got[2], hw[2])):
                assert np.array_equal(g, w), "%s of the clusters: device %s, twin %s (%d samples, %d in a first trip)" % (what, g.tolist(), w.tolist(), S, cap_crit)
            branches |= set(hw[1].tolist())
            clusters = np.unique(final)
            for k, b in enumerate(hw[1]):
                cells = np.flatnonzero(final == clusters[k])
                if b != 2:
                    assert np.array_equal(got[0][k].view(np.uint64), hw[0][k].view(np.uint64)), (k, b)
                else:
                    bound = 4 * S * len(cells) * 2.0 ** -53
                    assert np.all(np.abs(got[0][k] - hw[0][k]) <= bound * np.abs(hw[0][k])), (k, b)
                if 0 < hw[2][k] < S:                                                 # the samples that decide this cluster's mean, from the labels alone
                    first = a[:, cells[0]]
                    same = (a[:, cells] == first[:, None]).all(axis=1)
                    both = same & ((a == first[:, None]).sum(axis=1) == len(cells))
                    use = both if both.any() else same
                    assert int(use.sum()) == hw[2][k]
                    later = later or (use[:cap_crit].any() and use[cap_crit:].any() and not use[cap_crit:].all())
        assert {0, 2, 3} <= branches, branches
        assert later, "no cluster's used samples lie on both sides of the first trip"
    finally:
        engine.bnpc_unload()


# ---- k_cell_classify, k_cells_status: a thread per cell ----------------------------------------------------------------------------------
N_CB = 130


def cell_sites(cap):
    """sites of 130 barcodes that hold past(cap, 130 * 37) cells, rounded up to whole sites"""
    n_sites = -(-gc.past(cap, N_CB * 37) // N_CB)
    return n_sites, n_sites * N_CB


def test_cell_verdicts_past_the_cap(engine):
    from tests.test_cellclust_gpu import A2, B2, STATUS, reference_cell
    cap = cap_of("k_cell_classify", gc.cu_count())
    n_sites, n = cell_sites(cap)
    sized("k_cell_classify", n, cap)
    grid = [(dp, alt) for dp in range(1, 65) for alt in range(1, dp + 1)] + [(dp, alt) for dp in (100, 257, 1000, 4096) for alt in range(1, 41)]
    assert len(grid) == 2240
    pattern = np.array(grid + [(0, 0), (1, 0), (3, 0), (64, 0), (4096, 0), (0, 0)], np.uint32)
    idx = repeated(len(pattern), n, cap)
    rng = np.random.default_rng(n)
    is_chrm = np.zeros(n_sites, np.uint8)
    is_chrm[rng.permutation(n_sites)[:n_sites // 2]] = 1
    dp, alt = pattern[idx, 0].reshape(n_sites, N_CB), pattern[idx, 1].reshape(n_sites, N_CB)
    # the reference once per distinct (DP, ALT, chrM), spread by index
    table = np.zeros((len(pattern), 2, 4), np.int32)
    for j, (d, al) in enumerate(pattern.tolist()):
        for m in range(2):
            vaf, bb, mutated, binarized = reference_cell(d, al, "chrM" if m else "chr1", "True", A2, B2, 0.01)
            table[j, m] = (-1 if vaf == '.' else int(round(vaf * 10000)), -1 if bb == '.' else int(round(bb * 10000)), STATUS.index(mutated), binarized)
    code = idx * 2 + np.repeat(is_chrm.astype(np.int64), N_CB)
    assert len(np.unique(code[cap:])) == 2 * len(pattern)                       # every case on both kinds of site, behind the first trip
    want = table.reshape(-1, 4)[code]
    for col, name in enumerate(("vaf4", "p4", "status", "bin")):
        differs_from_a_stride_earlier(name, want[:, col], cap)
    engine.cellgeno_load_counts(dp, alt, is_chrm, A2, B2, 0.01)
    got = engine.cellgeno_fetch()
    same_everywhere("dp", got["dp"], dp, cap); same_everywhere("alt", got["alt"], alt, cap)
    for col, name in enumerate(("vaf4", "p4", "status", "bin")):
        same_everywhere(name, got[name], want[:, col], cap)
    assert set(want[:, 2].tolist()) == {0, 1, 2, 3, 4}
    status = want[:, 2].reshape(n_sites, N_CB)
    np.testing.assert_array_equal(got["n_covered"], (dp > 0).sum(axis=0))
    np.testing.assert_array_equal(got["n_pass"], (status == 4).sum(axis=0))


def test_loaded_cells_past_the_cap(engine):
    cap = cap_of("k_cells_status", gc.cu_count())
    n_sites, n = cell_sites(cap)
    sized("k_cells_status", n, cap)
    rng = np.random.default_rng(n + 1)
    bins = np.array([0, 1, 3], np.uint8)[rng.integers(0, 3, (n_sites, N_CB))]
    vaf4 = rng.integers(-1, 10001, (n_sites, N_CB)).astype(np.int32)
    assert vaf4.min() == -1 and vaf4.max() == 10000
    want = np.where(bins == 3, 0, np.where(bins == 1, 4, 1)).astype(np.uint8)      # NoCoverage, PASS, NoAltReads
    differs_from_a_stride_earlier("status", want, cap)
    engine.cellgeno_load_cells(bins, vaf4)
    got = engine.cellgeno_fetch()
    assert sorted(got) == ["bin", "n_covered", "n_pass", "status", "vaf4"]
    same_everywhere("status", got["status"], want, cap)
    same_everywhere("bin", got["bin"], bins, cap); same_everywhere("vaf4", got["vaf4"], vaf4, cap)
    np.testing.assert_array_equal(got["n_covered"], (bins != 3).sum(axis=0))
    np.testing.assert_array_equal(got["n_pass"], (bins == 1).sum(axis=0))


# ---- k_sf4_batch: a thread per (k, n) pair -------------------------------------------------------------------------------------------------
def test_betabinom_sf4_past_the_cap(engine):
    cap = cap_of("k_sf4_batch", gc.cu_count())
    n = gc.past(cap, 1000)
    sized("k_sf4_batch", n, cap)
    with open(os.path.join(G, "betabinom_sf_table.json")) as f:
        t = json.load(f)
    rows = t["rows"]
    want4 = np.array([int(round(float(r[2]) * 10000)) for r in rows], np.int32)
    assert [str(v / 10000.0) for v in want4.tolist()] == [r[2] for r in rows]        # the table's strings, as four-digit integers
    idx = repeated(len(rows), n, cap)
    nn, kk = np.array([r[0] for r in rows], np.uint32)[idx], np.array([r[1] for r in rows], np.uint32)[idx]
    want = want4[idx]
    differs_from_a_stride_earlier("sf4", want, cap)
    got = engine.betabinom_sf4(kk, nn, t["alpha2"], t["beta2"])
    same_everywhere("sf4", got, want, cap)


# ---- k_bbfit_accumulate: a wave per 64-position unit ---------------------------------------------------------------------------------------
def test_bbfit_accumulate_past_the_cap(engine):
    from tests.test_bbfit_gpu import CAP, CONTIG, LDS, make_rows
    cap = cap_of("k_bbfit_accumulate", gc.cu_count())
    n = gc.past(cap, 100)
    sized("k_bbfit_accumulate", n, cap)
    _, refs, counts = make_rows(n, 7 * n, 0)
    pos = 1 + 70 * np.arange(n, dtype=np.int64)                                      # a row to a 64-position unit
    assert np.all(np.diff(pos // 64) >= 1) and pos[-1] < CONTIG
    engine.set_contigs([CONTIG])
    engine.load_counts([pos], [counts])
    v = bbfit.site_counts(refs, counts)
    for sample_n in (0, 1000):
        want, seen, kept = bbfit.histograms(refs, counts, CAP, 0, sample_n)
        left = bbfit.thin(n, 0, sample_n, 1992)
        keep = np.zeros(n, bool)
        keep[left] = bbfit.kept(v[0][left], v[2][left], v[3][left], v[5][left])
        assert int(left.sum()) == seen and int(keep.sum()) == kept
        dp = np.asarray(v[5])
        later = keep[cap:]                                                          # the LDS bins and the HBM bins both depend on later trips
        assert np.any(later & (dp[cap:] >= LDS)) and np.any(later & (dp[cap:] < LDS)), sample_n
        engine.bbfit_reset(CAP)
        got = engine.bbfit_accumulate(0, ref=refs, table=0, sample_n=sample_n)
        print("sample_n %d: %d rows seen, %d kept (%d of them behind the first trip)" % (sample_n, seen, kept, int(keep[cap:].sum())))
        assert got == (seen, kept), "rows (seen, kept): device %s, twin %s of %d (cap %d)" % (got, (seen, kept), n, cap)
        hist = engine.bbfit_fetch()
        assert np.array_equal(hist, want), [np.flatnonzero(hist[h] != want[h])[:5].tolist() for h in range(6)]
        if sample_n:
            assert 700 < seen < 1300
