"""CPU: the long-read file of tests/support/longread_cases.py is what it claims to be, and the three CPU statements of the count agree on
it: the host decoder's arrays under the events-level oracle (hostio.decode_bam + loader.count) against the BAM-level column oracle
(loader.plp_count, oracle/plp_oracle.c, which shares no code with either decoder).  Exact; tests/test_longread_gpu.py holds the device to
the same tables."""
import struct
import zlib

import numpy as np
import pytest

from longsom_amd import hostio
from oracle import loader
from tests.support import longread_cases as lc

DEFAULTS = (20, 60, 5, 5)                                     # CountParams.longsom_defaults(): min_bq, min_mq, min_dp, min_cc
LOOSE = (10, 30, 1, 1)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return lc.written(tmp_path_factory)


def members_and_records(bam):
    """the file read with zlib and struct alone: [(first byte, end) of every BGZF member in the inflated stream], [(start, end, tid, pos, n_cigar) per record]"""
    raw = open(bam, "rb").read()
    members, parts, off, at = [], [], 0, 0
    while off < len(raw):
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        assert raw[off + 12:off + 14] == b"BC"
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        data = zlib.decompress(raw[off + 12 + xlen:off + bsize - 8], -15)
        members.append((at, at + len(data))); parts.append(data)
        at += len(data); off += bsize
    data = b"".join(parts)
    l_text = struct.unpack_from("<I", data, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<I", data, p)[0]; p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<I", data, p)[0] + 4
    records = []
    while p < len(data):
        bs, tid, pos, _, _, _, n_cigar = struct.unpack_from("<IiiBBHH", data, p)
        records.append((p, p + 4 + bs, tid, pos, n_cigar))
        p += 4 + bs
    assert p == len(data)
    return members, records


def test_the_file_has_the_shapes_it_is_for(case):
    members, records = members_and_records(case.bam)
    assert len(records) == 80
    starts = np.array([r[0] for r in records])
    big = max(records, key=lambda r: r[1] - r[0])
    assert big[1] - big[0] >= 390_000 and big[4] == 65535
    assert sum(1 for r in records if r[4] == 65535) == 20
    spanned = [m for m in members if m[0] < big[1] and m[1] > big[0]]
    assert len(spanned) >= 6                                                                     # one record over seven or eight members ...
    empty = [m for m in members if m[1] > m[0] and not ((starts >= m[0]) & (starts < m[1])).any()]
    assert len(empty) >= 4                                                                       # ... whose middle ones hold no record start
    assert sum(1 for m in spanned if m in empty) >= 4
    rec = case.decoded().records
    tiles = (rec.seg_start.astype(np.int64) + rec.seg_len - 1) // 64 - rec.seg_start.astype(np.int64) // 64 + 1
    st = rec.seg_start.astype(np.int64)
    first_edge = 1 + lc.WINDOW * (np.maximum(st - 1, 0) // lc.WINDOW + 1)                        # windows are [1 + k W, 1 + (k + 1) W): store.hip win_edge_after
    edges_inside = np.where(first_edge <= st + rec.seg_len - 1, (st + rec.seg_len - 1 - first_edge) // lc.WINDOW + 1, 0)
    assert ((tiles >= 1800) & (edges_inside == 2)).any() and ((tiles >= 1800) & (edges_inside == 3)).any()
    assert np.bincount(rec.seg_read).max() >= 400
    # neighbouring segments of one read inside one tile (many_exons' shortest introns)
    same = (rec.seg_read[1:] == rec.seg_read[:-1]) & ((rec.seg_start[1:].astype(np.int64) // 64) == ((rec.seg_start[:-1].astype(np.int64) + rec.seg_len[:-1] - 1) // 64))
    assert same.any()
    for r in case.by_family["long_indels"]:
        assert r["pos"] + r["ref_len"] == case.lens[1]
    on_m = np.flatnonzero(rec.read_tid == 1)
    last_seg_end = np.zeros(rec.n_reads, np.int64)
    last_seg_end[rec.seg_read] = rec.seg_start.astype(np.int64) + rec.seg_len                    # (ascending within a read: the last one stays)
    assert len(on_m) and (rec.read_pos[on_m] == 0).all() and (last_seg_end[on_m] == case.lens[1]).all()
    a = [r["pos"] for r in case.by_family["long_match"]]
    assert any((x - 1) % lc.WINDOW == 0 for x in a)                                              # a copy starts on a window's first column ...
    assert any((x + 120_000 - 1) % lc.WINDOW == 0 for x in a)                                    # ... one ends on a window's last ...
    assert any(x % lc.WINDOW == 0 for x in a) and {x % 2 for x in a} == {0, 1}                   # ... and one has a single column in the window before
    counted = [r for r in case.by_family["long_match"] if not r["flag"] & 0x900 and r["mapq"] == 60 and r["tags"]]
    assert any((r["pos"] - 1) % lc.WINDOW == 0 for r in counted) and any((r["pos"] + 120_000 - 1) % lc.WINDOW == 0 for r in counted)
    # the filters are not vacuous
    flags = np.array([r["flag"] for r in case.reads])
    assert ((flags & 0x10) != 0).sum() == 40 and ((flags & 0x800) != 0).sum() == 4 and ((flags & 0x100) != 0).sum() == 4
    assert sum(1 for r in case.reads if r["mapq"] == 20) == 4 and sum(1 for r in case.reads if not r["tags"]) == 4
    assert sum(1 for r in case.reads if "N" in r["seq"]) == 80 and sum(1 for r in case.reads if "R" in r["seq"]) > 0


def both_oracles(case, ct, p, legacy=False, **kw):
    min_bq, min_mq, min_dp, min_cc = p
    old = hostio.set_legacy_del_merge(legacy)
    loader.plp_set_legacy_del_merge(legacy)
    try:
        rec = case.decoded(min_mq).records
        k, r, c = loader.plp_count(case.bam, case.barcodes, case.celltype_of, ct, case.lens, case.refs, min_bq, min_mq, min_dp, min_cc, **kw)
    finally:
        hostio.set_legacy_del_merge(old)
        loader.plp_set_legacy_del_merge(False)
    ok, orf, oc, _ = loader.count(rec, case.lens, case.refs, case.celltype_of, ct, min_bq, min_mq, min_dp, min_cc)
    np.testing.assert_array_equal(k, ok); np.testing.assert_array_equal(r, orf); np.testing.assert_array_equal(c, oc)
    return k, r, c


@pytest.mark.parametrize("legacy", [False, True], ids=["htslib", "legacy_del_merge"])
@pytest.mark.parametrize("p", [DEFAULTS, LOOSE], ids=["defaults", "bq10_mq30_dp1_cc1"])
@pytest.mark.parametrize("ct", [0, 1])
def test_host_decoder_and_events_oracle_equal_the_bam_level_oracle(case, ct, p, legacy):
    k, r, c = both_oracles(case, ct, p, legacy)
    if p == DEFAULTS:
        assert len(k) >= 100_000
        for fam in lc.FAMILIES:                                                                  # where the family's reads are the only ones
            assert case.inside(k, case.alone[fam]).sum() >= 1_000, fam


def test_the_legacy_deletion_merge_changes_rows_on_this_file(case):
    """1D2D and D then I sit in the 65 535-operation reads: htslib <= 1.10's rule counts other events there, so the legacy cases above test it"""
    a = both_oracles(case, 0, LOOSE, legacy=False)
    b = both_oracles(case, 0, LOOSE, legacy=True)
    assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]))


@pytest.mark.parametrize("ct", [0, 1])
def test_a_depth_cap_of_8_drops_rows_in_every_chr1_family(case, ct):
    """Each family is looked at where its reads are the only ones with columns (case.alone), so that no neighbour's rows stand in for its
    own.  A family puts eight countable reads of a cell type into a window's pileup, nine in the cell type of its supplementary copy (the
    pileup's pool keeps 0x800); htslib drops a read that is not the first of its start position once eight are buffered.  max_cigar and
    many_exons lose rows in both cell types: their windows still hold reads of the family before them in the file.  long_match is first in
    the file: it loses rows where it lies alone only in the cell type with nine of its own, and in both where it shares columns with
    max_cigar."""
    free = loader.plp_count(case.bam, case.barcodes, case.celltype_of, ct, case.lens, case.refs, max_depth=0, window=lc.WINDOW)
    capped = loader.plp_count(case.bam, case.barcodes, case.celltype_of, ct, case.lens, case.refs, max_depth=8, window=lc.WINDOW)

    def rows_depth(stretch):
        m0, m1 = case.inside(free[0], stretch), case.inside(capped[0], stretch)
        return (int(m0.sum()), int(free[2][m0, 0].sum())), (int(m1.sum()), int(capped[2][m1, 0].sum()))
    for name in ("max_cigar", "many_exons"):
        a, b = rows_depth(case.alone[name])
        print(name, "alone", case.alone[name], "(rows, depth)", a, "->", b)
        assert b[0] < a[0] and b[1] < a[1], name
    for name, stretch in case.shared.items():
        a, b = rows_depth(stretch)
        print(name, stretch, "(rows, depth)", a, "->", b)
        assert b[0] < a[0] and b[1] < a[1], name
    pooled = sum(1 for r in case.by_family["long_match"] if r["tags"] and r["mapq"] == 60 and not r["flag"] & 0x100
                 and case.celltype_of[case.barcodes.index(r["tags"]["CB"])] == ct)
    a, b = rows_depth(case.alone["long_match"])
    print("long_match alone", case.alone["long_match"], "reads in the pool", pooled, "(rows, depth)", a, "->", b)
    assert pooled in (8, 9) and a[0] > 50_000
    assert (b[0] < a[0] and b[1] < a[1]) if pooled == 9 else (a == b)
    narrow = loader.plp_count(case.bam, case.barcodes, case.celltype_of, ct, case.lens, case.refs, max_depth=8, window=1000)
    assert not (np.array_equal(narrow[0], capped[0]) and np.array_equal(narrow[2], capped[2]))  # the windows are pileups of their own


@pytest.mark.parametrize("world", [2, 3, 5])
def test_a_region_boundary_falls_inside_the_long_intron(case, world):
    """regions.BaiPlan over the file's own index cuts chr1 (no read at the head of the file spans it), and one cut lies strictly inside the
    600 000-base intron of every many_exons copy: the slice before it ends on records that start before the cut, so the first guess of its
    end - four 16 kb windows on - stops short (tests/test_longread_gpu.py counts the attempts)"""
    import os
    from longsom_amd import regions
    plan = regions.BaiPlan(hostio.read_bai(hostio.build_bai(case.bam)), len(case.contigs), world, os.path.getsize(case.bam))
    cuts = [p for t, p in plan.bounds[1:-1] if t == 0]
    assert cuts and any(all(a < p < b for a, b in case.long_introns()) for p in cuts)
    assert any(p + 4 * regions.BAI_WINDOW < min(b for _, b in case.long_introns()) for p in cuts)      # the guess's margin ends inside the intron too
