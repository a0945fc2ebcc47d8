"""CPU: SplitBamCellTypes' read filters (--max_nM, --max_NH, --n_trim; SplitBamCellTypes.py:92-173) in the host decoder and the host
splitter, against what the reference's own split_bam + BaseCellCounter wrote for tests/golden/readfilter.bam (tools/make_readfilter_goldens.py).
The device ingest's twin: tests/test_readfilter_gpu.py."""
import ctypes
import hashlib
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

from longsom_amd import cli, hostio, tsvio
from oracle import loader
from tests.support import bamwrite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SETTINGS = {"nm": (5, None, 0), "nh": (None, 1, 0), "trim": (None, None, 5), "all": (5, 1, 5)}     # tools/make_readfilter_goldens.py
BAM, FA, BC = (os.path.join(G, "readfilter." + x) for x in ("bam", "fa", "barcodes.tsv"))


def golden_report(name):
    head, row = open(os.path.join(G, "readfilter.%s.report.txt" % name)).read().rstrip("\n").split("\n")
    return dict(zip(head.split("\t"), (int(x) for x in row.split("\t"))))


def golden_table(name, ct):
    p = os.path.join(G, "readfilter.%s.%s.tsv" % (name, ct))
    return open(p).read() if os.path.exists(p) else None


def no_date(text):
    return "".join(l for l in text.splitlines(True) if not l.startswith("##fileDate="))


def table(keys, refs, counts, names, sample_id):
    if len(keys) == 0:
        return None
    return no_date(tsvio.format_counts_tsv(keys, refs, counts, names, sample_id, "##fileDate=x\n"))


def raw_records(path):
    """every record of a BGZF BAM written by this repository's fixtures (bytes after block_size)"""
    raw, d, off = open(path, "rb").read(), b"", 0
    while off + 18 <= len(raw):
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        d += zlib.decompress(raw[off + 12 + xlen:off + bsize - 8], -15)
        off += bsize
    p = 8 + struct.unpack_from("<I", d, 4)[0]
    n_ref = struct.unpack_from("<I", d, p)[0]; p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<I", d, p)[0] + 4
    out = []
    while p + 4 <= len(d):
        bs = struct.unpack_from("<I", d, p)[0]
        out.append(d[p + 4:p + 4 + bs]); p += 4 + bs
    return out


def filters(name):
    return hostio.SplitFilters(*SETTINGS[name])


# ---- the splitter (SplitBamCellTypes.py's own outputs) --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_split_bam_cli_writes_the_reference_outputs(tmp_path, name):
    """report (columns in first-seen order) and every record of both cell-type BAMs, trimmed qualities included, as the reference wrote them"""
    max_nm, max_nh, n_trim = SETTINGS[name]
    argv = ["--bam", BAM, "--meta", BC, "--id", "s", "--outdir", str(tmp_path), "--min_MQ", "60", "--n_trim", str(n_trim)]
    argv += ["--max_nM", str(max_nm)] if max_nm is not None else []
    argv += ["--max_NH", str(max_nh)] if max_nh is not None else []
    cli.split_bam(argv)
    head, row = open(tmp_path / "s.report.txt").read().rstrip("\n").split("\n")
    h, r = head.split("\t"), row.split("\t")
    assert h[-1] == "Total_time"
    assert dict(zip(h[:-1], map(int, r[:-1]))) == golden_report(name) and h[:-1] == list(golden_report(name))
    want = json.load(open(os.path.join(G, "readfilter.%s.digests.json" % name)))
    for ct, digests in want.items():
        got = [hashlib.sha1(x).hexdigest()[:12] for x in raw_records(str(tmp_path / ("s.%s.bam" % ct)))]
        assert got == digests, ct


def test_rule_renders_off_as_empty_limits():
    """the .gpu.smk rules forward SNVCalling.SplitBam's keys as --max_nM=<v> --max_NH=<v> --n_trim=<v>: empty = off"""
    for fn in (cli.split_bam, cli.snv):
        import argparse
        captured = {}
        orig = argparse.ArgumentParser.parse_args

        def grab(self, args=None, namespace=None):
            captured["a"] = orig(self, ["--bam", "b", "--meta", "m", "--ref", "r", "--id", "i", "--outdir", "o", "--max_nM=", "--max_NH=None", "--n_trim=0"]
                                 if fn is cli.snv else ["--bam", "b", "--meta", "m", "--max_nM=", "--max_NH=3", "--n_trim=2"])
            raise SystemExit(0)
        argparse.ArgumentParser.parse_args = grab
        try:
            with pytest.raises(SystemExit):
                fn([])
        finally:
            argparse.ArgumentParser.parse_args = orig
        a = captured["a"]
        assert a.max_nM is None
        assert (a.max_NH, a.n_trim) == ((None, 0) if fn is cli.snv else (3, 2))


def test_gpu_rules_forward_the_config_keys():
    text = open(os.path.join(ROOT, "workflow", "rules", "SNVCalling.gpu.smk")).read()
    for rule in ("SNVCalling_gpu", "SplitBam_gpu"):
        body = re.search(r"^rule %s:\n(.*?)(?=^rule |\Z)" % rule, text, re.S | re.M).group(1)
        assert "--max_nM={params.max_nm} --max_NH={params.max_nh} --n_trim={params.n_trim}" in body.replace('"\n        "', ""), rule
    from tests.test_rules_cpu import entry_point, parser_of, render, rule_blocks
    for name, script, shell in rule_blocks(text):
        parser = parser_of(entry_point(script))
        a = parser.parse_args(render(shell))             # (every placeholder = 1: the keys set in the config)
        if "--max_nM" in shell:
            assert (a.max_nM, a.max_NH, a.n_trim) == (1, 1, 1)
        argv = render(shell)
        argv = [x.replace("--max_nM=1", "--max_nM=").replace("--max_NH=1", "--max_NH=").replace("--n_trim=1", "--n_trim=0") for x in argv]
        a = parser.parse_args(argv)                     # ... and as the reference's config renders them: off
        if "--max_nM" in shell:
            assert (a.max_nM, a.max_NH, a.n_trim) == (None, None, 0)


# ---- the host decoder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_host_decoder_report_and_tables(name):
    """report (keys in the reference's column order) and both count tables (host decoder + the CPU count oracle) equal the reference's"""
    bc = hostio.read_barcodes(BC)
    names, seqs = tsvio.read_fasta(FA)
    refs = [np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8) for s in seqs]
    dec = hostio.decode_bam(BAM, bc.barcodes, min_mapq=60, filters=filters(name))
    want = golden_report(name)
    assert list(dec.report) == list(want) and dec.report == want
    for ct, cname in enumerate(bc.celltype_names):
        k, r, c, _ = loader.count(dec.records, [len(x) for x in refs], refs, bc.celltype_of, ct)
        assert table(k, r, c, names, "s." + cname) == golden_table(name, cname), cname


def test_filters_off_is_todays_decode():
    bc = hostio.read_barcodes(BC)
    a = hostio.decode_bam(BAM, bc.barcodes, min_mapq=60)
    b = hostio.decode_bam(BAM, bc.barcodes, min_mapq=60, filters=hostio.SplitFilters())
    assert a.report == b.report and list(a.report) == ["Total_reads", "Pass_reads", "CB_not_found", "CB_not_matched", "MAPQ"]
    for n, _ in a.records._SPEC:
        assert np.array_equal(getattr(a.records, n), getattr(b.records, n)), n


def trim_rule(cigar_ops, n_trim):
    """SplitBamCellTypes.py:129-158 restated"""
    def end(op, ln):
        return (30 + n_trim if 20 <= ln < 30 else ln + n_trim) if op == 4 else n_trim
    if len(cigar_ops) > 1:
        return end(*cigar_ops[0]), end(*cigar_ops[-1])
    return n_trim, n_trim


def event_query_indices(ops, legacy=False):
    """per pileup event of a read (the decoder's order), the query index whose quality it carries (deletions and indel-flagged N
    columns: the next query base)"""
    out, y = [], 0
    for k, (op, ln) in enumerate(ops):
        nxt = ops[k + 1][0] if k + 1 < len(ops) else None
        if op in (1, 4):
            y += ln
        elif op in (0, 7, 8):
            out += [y + i for i in range(ln)]; y += ln
        elif op == 2:
            out += [y] * ln
        elif op == 3:
            if ln > 0 and nxt in (1, 2):
                out.append(y)
            elif ln > 0 and nxt == 6:
                l3 = 0
                for o, l in ops[k + 2:]:
                    if o == 1:
                        l3 += l
                    elif o in (2, 0, 3, 7, 8):
                        break
                if l3 > 0:
                    out.append(y)
    return out


@pytest.mark.parametrize("n_trim", [1, 3, 5])
def test_trimmed_qualities_are_zero_exactly_in_the_window(n_trim):
    """every event of every kept read: quality 0 inside the read's trim window, the read's own quality elsewhere"""
    bc = hostio.read_barcodes(BC)
    plain = hostio.decode_bam(BAM, bc.barcodes, min_mapq=0)
    cut = hostio.decode_bam(BAM, bc.barcodes, min_mapq=0, filters=hostio.SplitFilters(n_trim=n_trim))
    for n in ("read_tid", "read_pos", "read_flag", "seg_start", "seg_len", "seg_ev_off"):
        assert np.array_equal(getattr(plain.records, n), getattr(cut.records, n)), n
    listed = set(bc.barcodes)
    kept = []
    for raw in raw_records(BAM):
        tid, pos, l_name, mapq, _b, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", raw, 0)
        m = re.search(rb"CBZ([^\0]*)\0", raw[32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:])
        if tid < 0 or m is None or m.group(1).decode().split("-")[0] not in listed or flag & 4 or n_cigar == 0:
            continue
        kept.append(raw)
    rec = cut.records
    assert len(kept) == rec.n_reads
    ev_of_read = {}
    for s in range(rec.n_segs):
        ev_of_read.setdefault(int(rec.seg_read[s]), []).extend(rec.events[rec.seg_ev_off[s]:rec.seg_ev_off[s] + rec.seg_len[s]].tolist())
    n_zeroed = 0
    for r, raw in enumerate(kept):
        _t, _p, l_name, mapq, _b, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", raw, 0)
        ops = [(c & 0xF, c >> 4) for c in struct.unpack_from("<%dI" % n_cigar, raw, 32 + l_name)]
        qual = raw[32 + l_name + 4 * n_cigar + (l_seq + 1) // 2:][:l_seq]
        ts, te = trim_rule(ops, n_trim)
        qs = event_query_indices(ops)
        ev = ev_of_read.get(r, [])
        assert len(ev) == len(qs)
        for e, q in zip(ev, qs):
            if not e & 0x0800:                          # an IUPAC / '=' base: no event recorded (NA), nothing to trim
                continue
            want = 0 if (q < ts or q >= l_seq - te or q >= l_seq) else qual[q]
            assert e & 0xFF == want, (r, q, ts, te, l_seq)
            n_zeroed += want == 0 and q < l_seq and qual[q] != 0
    assert n_zeroed > 0


# ---- the rules the reference applies to the tags --------------------------------------------------------------------------------------
def one_read_bam(path, reads, contig=("chr1", 200)):
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


def tag(name, ty, v):
    return name.encode() + ty.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[ty], v)


def test_tag_types_duplicates_and_report_order(tmp_path):
    """every integer type and f compare numerically; a duplicated tag is read at its first occurrence (htslib bam_aux_get); the
    reasons' columns follow the file (NH_not_found before nM)"""
    bam = one_read_bam(tmp_path / "t.bam", [
        dict(name="a", cigar="20M", seq="A" * 20, aux=tag("nM", "c", -3)),                                 # NH_not_found
        dict(name="b", cigar="20M", seq="A" * 20, aux=tag("NH", "S", 1) + tag("nM", "I", 4000000000)),     # nM
        dict(name="c", cigar="20M", seq="A" * 20, aux=tag("nM", "f", 5.5) + tag("NH", "C", 1)),            # nM (5.5 > 5)
        dict(name="d", cigar="20M", seq="A" * 20, aux=tag("nM", "f", 5.0) + tag("NH", "s", 1)),            # pass
        dict(name="e", cigar="20M", seq="A" * 20, aux=tag("nM", "C", 1) + tag("nM", "C", 9) + tag("NH", "i", 1)),   # first nM = 1: pass
        dict(name="f", cigar="20M", seq="A" * 20, aux=tag("nM", "C", 9) + tag("nM", "C", 1) + tag("NH", "i", 1)),   # first nM = 9: nM
        dict(name="g", cigar="20M", seq="A" * 20, mapq=3, aux=tag("NH", "c", 2)),                         # nM_not_found;NH;MAPQ
    ])
    table_ = hostio.BarcodeTable(["AAAA"], np.zeros(1, np.uint8), ["Cancer"])
    want = {"Total_reads": 7, "Pass_reads": 2, "CB_not_found": 0, "CB_not_matched": 0, "NH_not_found": 1, "nM": 3, "nM_not_found;NH;MAPQ": 1}
    rep = hostio.split_bam(bam, table_, [str(tmp_path / "o.bam")], 60, hostio.SplitFilters(5, 1, 0))
    assert rep == want and list(rep) == list(want)
    dec = hostio.decode_bam(bam, ["AAAA"], 60, filters=hostio.SplitFilters(5, 1, 0))
    assert dec.report == want and list(dec.report) == list(want)
    assert dec.records.n_reads == 2 and sorted(dec.records.read_cb.tolist()) == [0, 0]


@pytest.mark.parametrize("case,filt,why", [
    ("long", hostio.SplitFilters(n_trim=5), "longer than the read"),
    ("ztag", hostio.SplitFilters(max_nM=5), "nM tag is not a number"),
    ("noqual", hostio.SplitFilters(n_trim=1), "no base qualities"),
])
def test_where_the_reference_raises_the_run_fails_naming_the_read(tmp_path, case, filt, why):
    reads = [dict(name="fine", cigar="20M", seq="A" * 20, aux=tag("nM", "C", 0) + tag("NH", "C", 1))]
    if case == "long":
        reads.append(dict(name="short_one", pos=12, cigar="2S3M", seq="ACGTA", aux=tag("nM", "C", 0)))
    elif case == "ztag":
        reads.append(dict(name="z_tagged", pos=12, cigar="20M", seq="A" * 20, aux=b"nMZ3\0"))
    else:
        reads.append(dict(name="no_qual", pos=12, cigar="20M", seq="A" * 20, qual=[], aux=tag("nM", "C", 0)))
    bam = one_read_bam(tmp_path / "e.bam", reads)
    bad = reads[-1]["name"]
    table_ = hostio.BarcodeTable(["AAAA"], np.zeros(1, np.uint8), ["Cancer"])
    with pytest.raises(RuntimeError, match=r"read '%s'.*%s" % (bad, why)):
        hostio.decode_bam(bam, ["AAAA"], 60, filters=filt)
    with pytest.raises(RuntimeError, match=r"read '%s'.*%s" % (bad, why)):
        hostio.split_bam(bam, table_, [str(tmp_path / "o.bam")], 60, filt)
    with pytest.raises(RuntimeError, match=r"read '%s'.*%s" % (bad, why)):
        list(hostio.stream_bam(bam, ["AAAA"], 60, filters=filt))
    # without the filter that trips over it the same file is fine
    assert hostio.decode_bam(bam, ["AAAA"], 60).report["Total_reads"] == 2


def test_negative_limits_are_refused():
    with pytest.raises(ValueError):
        hostio.SplitFilters(max_nM=-1)


# ---- the report -----------------------------------------------------------------------------------------------------------------------
def test_split_report_orders_reasons_by_load_then_ordinal():
    n0, f0 = [0] * 18, [-1] * 18
    assert hostio.split_report((10, 7, 1, 1, 1), None) == {"Total_reads": 10, "Pass_reads": 7, "CB_not_found": 1, "CB_not_matched": 1, "MAPQ": 1}
    assert hostio.split_report((9, 9, 0, 0, 0), None) == {"Total_reads": 9, "Pass_reads": 9, "CB_not_found": 0, "CB_not_matched": 0}
    a_n, a_f = list(n0), list(f0)
    a_n[6], a_f[6] = 2, 40          # nM at ordinal 40 of load 0
    a_n[2], a_f[2] = 1, 3           # NH at ordinal 3 of load 0
    b_n, b_f = list(n0), list(f0)
    b_n[1], b_f[1] = 4, 0           # MAPQ first in load 1
    b_n[6], b_f[6] = 1, 1
    rep = hostio.split_report((20, 13, 0, 0, 4), [(a_n, a_f), (b_n, b_f)])
    assert list(rep)[4:] == ["NH", "nM", "MAPQ"] and rep["nM"] == 3 and rep["MAPQ"] == 4
    assert len(set(hostio.REASON_KEYS[1:])) == 17 and hostio.REASON_KEYS[17] == "nM_not_found;NH_not_found;MAPQ"


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_the_header_and_the_libraries():
    text = open(os.path.join(ROOT, "include", "longsom_hip.h")).read()
    for n in ("lsg_set_split_filters", "lsg_get_split_reasons"):
        assert re.search(r"^int %s\(lsg_ctx\* ctx" % n, text, re.M), n
        assert hasattr(ctypes.CDLL(os.path.join(ROOT, "longsom_amd", "lib", "liblongsom_hip.so")), n), n
    io = ctypes.CDLL(os.path.join(ROOT, "longsom_amd", "lib", "liblongsom_io.so"))
    for n in ("lsio_split_bam_filtered", "lsio_decode_bam_filtered", "lsio_stream_set_split_filters"):
        assert hasattr(io, n), n
    assert ctypes.sizeof(hostio.Decoded) == hostio.Decoded.split_first.offset + 18 * 8
