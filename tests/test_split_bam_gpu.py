"""GPU: SplitBamCellTypes on the device (csrc/split.hip lsg_split_bam -> tables LSG_TABLE_SPLIT_BAM + t; csrc/deflate_core.h a lane per BGZF
block) against the reference's own run over tests/golden/readfilter.bam and against the host twin (hostio.split_bam), and the BGZF
writer for any bytes (lsg_bgzf_compress).  Every comparison is exact: inflated bytes, block cuts, CRC32s, counters, ordinals.  The
encoder itself on the host: tests/test_deflate_core_cpu.py."""
import ctypes as C
import gzip
import hashlib
import json
import os
import struct
import zlib

import numpy as np
import pytest

from longsom_amd import _lib, cli, hostio
from tests.support import bamwrite
from tests.support import fastq_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SETTINGS = {"nm": (5, None, 0), "nh": (None, 1, 0), "trim": (None, None, 5), "all": (5, 1, 5)}     # tools/make_readfilter_goldens.py
BAM, BC = (os.path.join(G, "readfilter." + x) for x in ("bam", "barcodes.tsv"))
EOF = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HEAD = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0])
BLOCK = 0xff00


def read(path):
    with open(path, "rb") as f:
        return f.read()


def blocks_of(raw):
    """a BGZF file's blocks as (inflated bytes, CRC32 field, ISIZE field); every header is the fixed 16 bytes + BSIZE - 1, BSIZE the true size"""
    out, off = [], 0
    while off < len(raw):
        assert raw[off:off + 16] == HEAD, "no BGZF header at %d" % off
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        assert off + bsize <= len(raw)
        data = zlib.decompress(raw[off + 18:off + bsize - 8], -15)       # (raises on a stream that does not end inside the block)
        crc, isize = struct.unpack_from("<II", raw, off + bsize - 8)
        out.append((data, crc, isize))
        off += bsize
    assert off == len(raw)
    return out


def check_file(raw):
    """the framing of one device-written file; returns (inflated bytes, ISIZEs)"""
    assert raw[-28:] == EOF
    blk = blocks_of(raw)
    for data, crc, isize in blk:
        assert crc == zlib.crc32(data) and isize == len(data) and isize <= BLOCK
    assert gzip.decompress(raw) == b"".join(b[0] for b in blk)
    return b"".join(b[0] for b in blk), [b[2] for b in blk]


def raw_records(raw):
    """tests/test_readfilter_cpu.py's raw_records over a file's bytes: every record (bytes after block_size)"""
    d = b"".join(b[0] for b in blocks_of(raw))
    p = 8 + struct.unpack_from("<I", d, 4)[0]
    n_ref = struct.unpack_from("<I", d, p)[0]; p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<I", d, p)[0] + 4
    out = []
    while p + 4 <= len(d):
        bs = struct.unpack_from("<I", d, p)[0]
        out.append(d[p + 4:p + 4 + bs]); p += 4 + bs
    return out


def host_split(bam, table, outs, min_mapq, filters):
    """lsio_split_bam_filtered as hostio.split_bam calls it, with the arrays its report is made of: (counters, reasons_n, reasons_first)"""
    lib = hostio.load()
    ct = np.ascontiguousarray(table.celltype_of, np.uint8)
    cnt = (C.c_int64 * 5)()
    rn, rf = (C.c_int64 * hostio.N_REASONS)(), (C.c_int64 * hostio.N_REASONS)()
    rc = lib.lsio_split_bam_filtered(os.fsencode(bam), "\n".join(table.barcodes).encode(), len(table.barcodes), ct.ctypes.data_as(C.c_void_p), len(table.celltype_names),
                                     "\n".join(outs).encode(), int(min_mapq), cnt, *(filters or hostio.SplitFilters()).args(), rn, rf)
    if rc != 0:
        raise RuntimeError(lib.lsio_last_error().decode())
    return list(cnt), list(rn), list(rf)


def device_split(engine, bam, table, min_mapq, filters):
    engine.set_split_filters(filters)
    try:
        info = engine.split_bam(bam, table.barcodes, table.celltype_of, len(table.celltype_names), min_mapq)
    finally:
        engine.set_split_filters(None)
    return info, [engine.table_bytes(engine.TABLE_SPLIT_BAM + t, info["n_file_bytes"][t]) for t in range(len(table.celltype_names))]


def same_as_host(engine, bam, table, min_mapq, filters, tmp_path):
    """the device's files against the host twin's: inflated bytes, block cuts, framing, counters; returns (info, device files, host paths)"""
    outs = [str(tmp_path / ("h.%d.bam" % t)) for t in range(len(table.celltype_names))]
    cnt, rn, rf = host_split(bam, table, outs, min_mapq, filters)
    info, files = device_split(engine, bam, table, min_mapq, filters)
    assert (info["counters"], info["reasons_n"], info["reasons_first"]) == (cnt, rn, rf)
    for t, raw in enumerate(files):
        data, isizes = check_file(raw)
        host = blocks_of(read(outs[t]))
        assert data == b"".join(b[0] for b in host), "cell type %d" % t
        assert isizes == [b[2] for b in host], "cell type %d: the cut rule" % t
        assert info["n_ubytes"][t] == len(data) and info["n_blocks"][t] == len(isizes) - 1 and info["n_file_bytes"][t] == len(raw)
    assert sum(info["n_written"]) == cnt[1]
    return info, files, outs


OVERSIZE_BARCODES, OVERSIZE_CELLTYPE_OF = ["GGGT", "CCCA", "AAAC"], [0, 0, 1]


def oversize_records():
    """reads every --n_trim 3 window fits, among them one of 70 000 bases (longer than a BGZF block) with soft clips at both ends"""
    recs = [fc.record("r%d" % k, 40 + 900 * k, True, {"CB": ("GGGT-1", "AAAC-1", "CCCA-1")[k % 3], "nM": k % 4}, True, 100 + 10 * k, shift=k) for k in range(12)]
    big = fc.record("long.read", 70000, True, {"CB": "CCCA-1", "nM": 1}, True, 155, shift=5)
    big["cigar"] = "25S69950M25S"                    # a clip of 20-29 bases trims 30 + n_trim (the adapter rule)
    return recs[:6] + [big] + recs[6:]


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("split")
    out = {}
    for name, recs in (("edge", fc.edge_records()[0]), ("routed", fc.routed_records()), ("fuzz", fc.fuzz_records(3000, 5000)), ("oversize", oversize_records())):
        out[name] = str(d / (name + ".bam"))
        fc.write(out[name], recs)
    meta = str(d / "routed.meta.tsv")
    with open(meta, "w") as f:
        f.write(fc.ROUTED_META)
    out["routed_table"] = hostio.read_barcodes(meta)
    out["edge_table"] = hostio.BarcodeTable(list(fc.EDGE_BARCODES), np.asarray(fc.EDGE_CELLTYPE_OF, np.uint8), ["Cancer", "Non-Cancer"])
    out["fuzz_table"] = hostio.BarcodeTable(list(fc.FUZZ_BARCODES), np.asarray(fc.FUZZ_CELLTYPE_OF, np.uint8), ["Cancer", "Non-Cancer"])
    out["oversize_table"] = hostio.BarcodeTable(list(OVERSIZE_BARCODES), np.asarray(OVERSIZE_CELLTYPE_OF, np.uint8), ["Cancer", "Non-Cancer"])
    return out


# ---- against the reference's own run ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_cli_device_writes_the_reference_outputs(tmp_path, name):
    """cli.split_bam --device 0: the report (columns in first-seen order) and every record of both BAMs, trimmed qualities included, as
    the reference's SplitBamCellTypes.py wrote them"""
    max_nm, max_nh, n_trim = SETTINGS[name]
    argv = ["--bam", BAM, "--meta", BC, "--id", "s", "--outdir", str(tmp_path), "--min_MQ", "60", "--n_trim", str(n_trim), "--device", "0"]
    argv += ["--max_nM", str(max_nm)] if max_nm is not None else []
    argv += ["--max_NH", str(max_nh)] if max_nh is not None else []
    cli.split_bam(argv)
    head, row = open(tmp_path / "s.report.txt").read().rstrip("\n").split("\n")
    ghead, grow = open(os.path.join(G, "readfilter.%s.report.txt" % name)).read().rstrip("\n").split("\n")
    h, r = head.split("\t"), row.split("\t")
    assert h[-1] == "Total_time" and h[:-1] == ghead.split("\t") and r[:-1] == grow.split("\t")
    want = json.load(open(os.path.join(G, "readfilter.%s.digests.json" % name)))
    for ct, digests in want.items():
        raw = read(str(tmp_path / ("s.%s.bam" % ct)))
        check_file(raw)
        assert [hashlib.sha1(x).hexdigest()[:12] for x in raw_records(raw)] == digests, ct


# ---- against the host twin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,min_mapq,filters", [
    ("edge", 60, None), ("edge", 30, hostio.SplitFilters(max_nM=2)), ("routed", 30, None), ("routed", 10, hostio.SplitFilters(max_nM=2)),
    ("fuzz", 60, None), ("fuzz", 10, hostio.SplitFilters(max_nM=1)), ("fuzz", 30, hostio.SplitFilters(max_nM=0)),
    ("oversize", 60, hostio.SplitFilters(n_trim=3)), ("oversize", 60, hostio.SplitFilters(max_nM=2, n_trim=3)),
])
def test_files_equal_the_host_twins(engine, bams, tmp_path, which, min_mapq, filters):
    """(the edge BAM holds reads of 0 and 1 bases and one without qualities: under --n_trim the host twin refuses it as the reference
    raises, so the trimmed cases run over the `oversize` BAM, whose 70 000-base read is trimmed by 33 at both ends)"""
    info, files, _ = same_as_host(engine, bams[which], bams[which + "_table"], min_mapq, filters, tmp_path)
    assert info["n_written"][0] > 0 and info["n_written"][1] > 0
    assert info["ms_deflate"] > 0 and info["ms_total"] > 0
    if which in ("edge", "oversize"):                       # the record longer than a block: spilled in 0xff00 pieces
        _, isizes = check_file(files[0])
        assert isizes.count(BLOCK) >= 1
    if which == "oversize":
        big = [r for r in raw_records(files[0]) if r[32:41] == b"long.read"][0]
        q = big[32 + big[8] + 4 * 3 + 35000:][:70000]
        assert set(q[:33]) == {0} and set(q[-33:]) == {0} and q[33:-33] == bytes(fc.quals(70000, 5))[33:-33]
    if which == "fuzz":                                     # smaller than the inflated stream: the encoder compresses
        assert sum(info["n_file_bytes"]) < sum(info["n_ubytes"])


def count_rows(engine, bam, table):
    from longsom_amd._lib import CountParams
    names, lens, first = hostio.bam_header(bam)
    engine.set_contigs(lens)
    for t, n in enumerate(lens):
        engine.load_reference(t, np.full(int(n), ord("A"), np.uint8))
    engine.set_barcodes(table.celltype_of, len(table.celltype_names))
    engine.set_region()
    info, _, _ = engine.load_bam(bam, table.barcodes, min_mapq=0, first_record_offset=first)       # (rc -4 would raise)
    return info["n_records"], engine.pileup_count(CountParams.longsom_defaults()), [engine.fetch_counts(ct) for ct in range(len(table.celltype_names))]


@pytest.mark.parametrize("which,filters", [("fuzz", None), ("oversize", hostio.SplitFilters(n_trim=3))])
def test_device_written_bams_read_back(engine, bams, tmp_path, which, filters):
    """each device-written BAM loads on the device (its blocks start on record boundaries: no -4) to the count rows of the host-written
    one, and the host decoder reads it"""
    table = bams[which + "_table"]
    info, files, outs = same_as_host(engine, bams[which], table, 30, filters, tmp_path)
    for t, raw in enumerate(files):
        dev_path = str(tmp_path / ("d.%d.bam" % t))
        with open(dev_path, "wb") as f:
            f.write(raw)
        n_dev, shape_dev, rows_dev = count_rows(engine, dev_path, table)
        n_host, shape_host, rows_host = count_rows(engine, outs[t], table)
        assert n_dev == n_host == info["n_written"][t] and shape_dev == shape_host
        for (k1, r1, c1), (k2, r2, c2) in zip(rows_dev, rows_host):
            np.testing.assert_array_equal(k1, k2); np.testing.assert_array_equal(c1, c2)
        dec_d, dec_h = hostio.decode_bam(dev_path, table.barcodes, 0), hostio.decode_bam(outs[t], table.barcodes, 0)
        assert dec_d.report == dec_h.report and dec_d.records.n_reads == dec_h.records.n_reads


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_cell_type_is_a_header_block_and_eof(engine, bams, tmp_path):
    table = hostio.BarcodeTable(["GGGT", "CCCA"], np.asarray([0, 0], np.uint8), ["Cancer", "Non-Cancer"])
    info, files, _ = same_as_host(engine, bams["routed"], table, 30, None, tmp_path)
    assert info["n_written"][0] > 0 and info["n_written"][1] == 0 and info["n_blocks"][1] == 1
    data, isizes = check_file(files[1])
    assert len(isizes) == 2 and isizes[1] == 0 and data[:4] == b"BAM\1"


def test_a_bam_without_records(engine, bams, tmp_path):
    bam = str(tmp_path / "none.bam")
    fc.write(bam, [])
    info, files, _ = same_as_host(engine, bam, bams["routed_table"], 30, None, tmp_path)
    assert info["n_records"] == 0 and info["counters"] == [0] * 5 and info["n_blocks"][:2] == [1, 1]


def test_a_header_longer_than_a_block(engine, bams, tmp_path):
    """4 000 contigs: the header goes through write(), which fills blocks to 0xff00, and the first record closes its tail"""
    bam = str(tmp_path / "wide.bam")
    contigs = [("chr1", 400000)] + [("contig_with_a_long_name_%05d" % i, 1000 + i) for i in range(4000)]
    bamwrite.write_bam(bam, contigs, fc.routed_records())
    assert hostio.bam_header(bam)[2] > 2 * BLOCK
    info, files, _ = same_as_host(engine, bam, bams["routed_table"], 30, None, tmp_path)
    assert check_file(files[0])[1][:2] == [BLOCK, BLOCK]


def test_more_blocks_than_a_wave_has_lanes(engine, tmp_path):
    """65 blocks in the call's one launch, all of one cell type: the deflate kernel's second workgroup runs with a single live lane (the
    blocks of all cell types are compressed together, so there is one cell type here: 65 = 64 + 1 blocks in all)"""
    recs = [fc.record("q%d" % k, 43000, True, {"CB": "GGGT-1"}, True, 10 + k, shift=k) for k in range(65)]
    bam = str(tmp_path / "many.bam")
    fc.write(bam, recs)
    table = hostio.BarcodeTable(["GGGT"], np.asarray([0], np.uint8), ["Cancer"])
    info, files, _ = same_as_host(engine, bam, table, 30, None, tmp_path)
    assert info["n_blocks"] == [65, 0, 0, 0]          # a block a record (two 64 KB records do not share one), the header in the first
    assert sum(info["n_blocks"]) % 64 == 1 and info["n_written"][0] == 65


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def one_read_bam(path, reads, contig=("chr1", 200)):
    """tests/test_readfilter_cpu.py's one_read_bam: records with raw aux bytes behind a CB:Z:AAAA-1"""
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n" % contig
    out = b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", 1)
    out += struct.pack("<I", len(contig[0]) + 1) + contig[0].encode() + b"\0" + struct.pack("<I", contig[1])
    for r in reads:
        rec = bamwrite.encode_record(0, r.get("pos", 10), r["name"], 0, r.get("mapq", 60), r["cigar"], r["seq"], r.get("qual", [30] * len(r["seq"])), {"CB": "AAAA-1"})
        body = rec[4:] + r.get("aux", b"")
        out += struct.pack("<I", len(body)) + body
    with open(path, "wb") as f:
        f.write(bamwrite._bgzf_block(out)); f.write(bamwrite._bgzf_block(b""))
    return str(path)


@pytest.mark.parametrize("case,filt,kind", [
    ("long", hostio.SplitFilters(n_trim=5), 1), ("noqual", hostio.SplitFilters(n_trim=1), 2), ("ztag", hostio.SplitFilters(max_nM=5), 3),
])
def test_where_the_reference_raises_the_call_names_the_hosts_read(engine, tmp_path, case, filt, kind):
    fine = dict(name="fine", cigar="20M", seq="A" * 20, aux=b"nMC\0NHC\1")
    bad = {"long": dict(name="short_one", pos=12, cigar="2S3M", seq="ACGTA", aux=b"nMC\0"),
           "ztag": dict(name="z_tagged", pos=12, cigar="20M", seq="A" * 20, aux=b"nMZ3\0"),
           "noqual": dict(name="no_qual", pos=12, cigar="20M", seq="A" * 20, qual=[], aux=b"nMC\0")}[case]
    also = dict(bad, name="second", pos=14)                                  # a second such read behind it: the smallest ordinal is named
    bam = one_read_bam(tmp_path / "e.bam", [fine, fine, bad, fine, also])
    table = hostio.BarcodeTable(["AAAA"], np.zeros(1, np.uint8), ["Cancer"])
    with pytest.raises(RuntimeError, match=r"read '%s' \(record 2\)" % bad["name"]) as h:
        host_split(bam, table, [str(tmp_path / "o.bam")], 60, filt)
    engine.set_split_filters(filt)
    try:
        with pytest.raises(_lib.LsgError, match=r"read '%s' \(record 2\)" % bad["name"]) as d:
            engine.split_bam(bam, table.barcodes, table.celltype_of, 1, 60)
    finally:
        engine.set_split_filters(None)
    assert d.value.rc == -1 and (d.value.info["bad_ordinal"], d.value.info["bad_kind"]) == (2, kind)
    assert str(d.value).split("lsg_split_bam: ", 1)[1] == str(h.value).split(bam + ": ", 1)[1]       # the same message behind the caller's name
    with pytest.raises(_lib.LsgError, match="not formatted"):                                          # no table is kept
        engine.table_bytes(engine.TABLE_SPLIT_BAM, 0)
    info, files = device_split(engine, bam, table, 60, None)              # without the filter that trips over it the same file is fine
    assert info["counters"][0] == 5 and len(raw_records(files[0])) == 5
    with pytest.raises(_lib.LsgError, match="lsg_split_bam"):             # the slot is not lsg_format_table's to make
        engine.format_table(engine.TABLE_SPLIT_BAM)


# ---- lsg_bgzf_compress --------------------------------------------------------------------------------------------------------------------
def contents(kind, n, seed=7):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "one_byte":
        return b"\x5a" * n
    if kind == "period3":
        return (b"abc" * (n // 3 + 1))[:n]
    if kind == "string64":
        s = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
        return (s * (n // 64 + 1))[:n]
    if kind == "far_repeat":
        s = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
        return (s * (n // 40000 + 1))[:n]
    if kind == "four_values":
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    if kind == "two_values":
        return np.frombuffer(b"\x11\xee", np.uint8)[rng.integers(0, 2, n)].tobytes()
    assert kind == "all_values"
    return bytes(i & 0xff for i in range(n))


KINDS = ["random", "one_byte", "period3", "string64", "far_repeat", "four_values", "two_values", "all_values"]


@pytest.mark.parametrize("n", [0, 1, BLOCK, BLOCK + 1, 64 * BLOCK + 1, 65 * BLOCK + 1])      # 64 * BLOCK + 1: 65 blocks, a second workgroup with one live lane
def test_bgzf_compress_reads_back(engine, n):
    for kind in KINDS:
        data = contents(kind, n)
        raw = engine.bgzf_compress(data)
        assert gzip.decompress(raw) == data, kind
        inflated, isizes = check_file(raw)
        assert inflated == data and isizes == [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else []) + [0], kind
        if kind == "random" and n >= BLOCK:                  # stored: 5 bytes a block above the input, the framing apart
            assert len(raw) == n + 31 * (len(isizes) - 1) + 28
    with pytest.raises(_lib.LsgError, match="not formatted"):      # bgzf_compress hands the bytes over and frees the table
        engine.table_bytes(engine.TABLE_BGZF, 0)


def test_bgzf_compress_really_compresses(engine):
    """the two size conditions of tests/native/test_deflate.cpp on the device's output: Huffman codes (four byte values at random:
    fixed codes give 0.549 n, zlib level 1 0.338 n) and LZ77 matches (a 64-byte string repeated: Huffman alone gives 0.72 n)"""
    n = BLOCK
    for kind, bound in (("four_values", 0.40), ("string64", 0.10)):
        raw = engine.bgzf_compress(contents(kind, n))
        payload = len(raw) - 26 - 28
        print("%s: %d -> %d (%.4f n)" % (kind, n, payload, payload / n))
        assert payload <= bound * n, kind
