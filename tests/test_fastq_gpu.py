"""GPU: the FASTQ printer (csrc/fastq.hip lsg_bam_fastq -> table LSG_TABLE_FASTQ) against its host twin (hostio.bam_fastq), which
tests/test_fastq_cpu.py pins to the reference script's files and to the hand-stated edge cases.  Every comparison is exact: bytes, counts,
ordinals."""
import os

import numpy as np
import pytest

from longsom_amd import _lib, cli, hostio
from tests.support import fastq_cases as fc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INFO_KEYS = ("n_records", "n_printed", "n_bytes", "bad_ordinal", "bad_kind")


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    """the BAMs of this module, written once: the edge cases, the routed cases, the seeded fuzz of 3 000 records of 0 to 5 000 bases"""
    d = tmp_path_factory.mktemp("fastq")
    out = {}
    for name, recs in (("edge", fc.edge_records()[0]), ("routed", fc.routed_records()), ("fuzz", fc.fuzz_records(3000, 5000))):
        out[name] = str(d / (name + ".bam"))
        fc.write(out[name], recs)
    meta = str(d / "routed.meta.tsv")
    with open(meta, "w") as f:
        f.write(fc.ROUTED_META)
    out["routed_table"] = hostio.read_barcodes(meta)
    out["edge_table"] = hostio.BarcodeTable(list(fc.EDGE_BARCODES), np.asarray(fc.EDGE_CELLTYPE_OF, np.uint8), ["Cancer", "Non-Cancer"])
    out["fuzz_table"] = hostio.BarcodeTable(list(fc.FUZZ_BARCODES), np.asarray(fc.FUZZ_CELLTYPE_OF, np.uint8), ["Cancer", "Non-Cancer"])
    out["dir"] = str(d)
    return out


def device_text(engine, bam, table=None, min_mapq=60):
    info = engine.bam_fastq(bam, None if table is None else table.barcodes, None if table is None else table.celltype_of,
                            0 if table is None else len(table.celltype_names), min_mapq)
    return info, engine.table_bytes(engine.TABLE_FASTQ, sum(info["n_bytes"]))


def same_info(dev, host):
    assert {k: dev[k] for k in INFO_KEYS} == {k: host[k] for k in INFO_KEYS}


@pytest.mark.parametrize("which", ["edge", "fuzz"])
def test_plain_mode_equals_the_host_twin(engine, bams, tmp_path, which):
    host = hostio.bam_fastq(bams[which], str(tmp_path / "h.fastq"))
    dev, text = device_text(engine, bams[which])
    same_info(dev, host)
    want = read(str(tmp_path / "h.fastq"))
    if text != want:                                              # name the first record that differs
        k = next(i for i in range(min(len(text), len(want))) if text[i] != want[i]) if len(text) == len(want) else -1
        pytest.fail("device FASTQ differs from the host twin's at byte %d (record %d): %r / %r" % (k, want[:max(k, 0)].count(b"\n") // 4, text[k - 20:k + 20], want[k - 20:k + 20]))
    if which == "edge":
        assert text == fc.edge_records()[1].encode("latin-1")    # the hand-stated text itself
    assert dev["ms_print"] > 0 and dev["ms_total"] > 0


@pytest.mark.parametrize("which,min_mapq,filters", [("edge", 60, None), ("edge", 60, hostio.SplitFilters(max_nM=2)), ("routed", 30, None), ("routed", 30, hostio.SplitFilters(max_nM=2)), ("fuzz", 60, None),
                                                     ("fuzz", 10, hostio.SplitFilters(max_nM=1))])
def test_routed_mode_equals_the_host_twin(engine, bams, tmp_path, which, min_mapq, filters):
    table = bams[which + "_table"]
    host = hostio.bam_fastq(bams[which], str(tmp_path / "h.fastq"), table, min_mapq, filters)
    engine.set_split_filters(filters)
    try:
        dev, text = device_text(engine, bams[which], table, min_mapq)
    finally:
        engine.set_split_filters(None)
    same_info(dev, host)
    assert text == read(str(tmp_path / "h.fastq"))
    assert sum(dev["n_printed"]) > 0 and dev["n_printed"][0] > 0 and dev["n_printed"][1] > 0
    if which == "edge":      # the hand-stated text: the 70 000-base read behind its cell type's other records, both cell types, no unmapped read
        want, counts = fc.edge_routed_text(None if filters is None else filters.max_nM)
        assert text == want.encode("latin-1") and dev["n_printed"][:2] == counts
        assert b"@CCCA^U1^long.read\n" in text and b"@FIRST^NA^abcdefg\n" in text and b"un.mapped.q" not in text
    if which == "routed" and filters is None:
        assert text == read(os.path.join(G, "fusion", "routed.fastq"))      # what the reference's script wrote over the split BAMs


@pytest.mark.parametrize("kind,code", [("no_cb", _lib.FASTQ_NO_CB), ("cb_type", _lib.FASTQ_CB_TYPE), ("ub_type", _lib.FASTQ_UB_TYPE)])
def test_error_kinds_come_back_with_the_hosts_ordinals(engine, tmp_path, kind, code):
    recs, ordinal = fc.bad_records(kind)
    bam = str(tmp_path / "bad.bam")
    fc.write(bam, recs)
    with pytest.raises(hostio.FastqError) as h:
        hostio.bam_fastq(bam, str(tmp_path / "h.fastq"))
    with pytest.raises(_lib.LsgError, match=r"record %d\)" % ordinal) as d:
        engine.bam_fastq(bam)
    assert (d.value.info["bad_ordinal"], d.value.info["bad_kind"]) == (h.value.info["bad_ordinal"], h.value.info["bad_kind"]) == (ordinal, code)
    assert str(d.value).split("lsg_bam_fastq: ", 1)[1] == str(h.value).split("lsio_bam_fastq: ", 2)[2]      # the same message behind the caller's name
    with pytest.raises(_lib.LsgError, match="not formatted"):                                                # no text is kept
        engine.table_bytes(engine.TABLE_FASTQ, 0)


@pytest.mark.parametrize("kind,code", [("nm_type", _lib.FASTQ_NM_TYPE), ("nh_type", _lib.FASTQ_NH_TYPE)])
def test_a_string_nM_or_NH_comes_back_with_the_hosts_ordinal(engine, bams, tmp_path, kind, code):
    """routed mode under --max_nM / --max_NH: lsf::route's refusal, through k_fq_len's atomicMin"""
    recs, ordinal = fc.bad_records(kind)
    bam = str(tmp_path / "bad.bam")
    fc.write(bam, recs)
    limit = hostio.SplitFilters(max_nM=2) if kind == "nm_type" else hostio.SplitFilters(max_NH=2)
    table = bams["edge_table"]
    with pytest.raises(hostio.FastqError) as h:
        hostio.bam_fastq(bam, str(tmp_path / "h.fastq"), table, 60, limit)
    engine.set_split_filters(limit)
    try:
        with pytest.raises(_lib.LsgError, match=r"read 'tagstr' \(record %d\)" % ordinal) as d:
            engine.bam_fastq(bam, table.barcodes, table.celltype_of, 2, 60)
    finally:
        engine.set_split_filters(None)
    assert d.value.rc == -1
    assert (d.value.info["bad_ordinal"], d.value.info["bad_kind"]) == (h.value.info["bad_ordinal"], h.value.info["bad_kind"]) == (ordinal, code)
    assert str(d.value).split("lsg_bam_fastq: ", 1)[1] == str(h.value).split("lsio_bam_fastq: ", 2)[2]
    dev, text = device_text(engine, bam, table, 60)                 # without the limit nobody reads the tag: the call succeeds,
    assert b"^tagstr\n" not in text                                 # and the read only fails its MAPQ
    assert sum(dev["n_printed"]) == sum(fc.edge_routed_text(None)[1])


def test_append_table_writes_the_copy(engine, bams, tmp_path):
    dev, text = device_text(engine, bams["edge"])
    out = str(tmp_path / "a.fastq")
    with open(out, "wb") as f:
        f.write(b"kept\n")
    engine.append_table(engine.TABLE_FASTQ, out)
    assert read(out) == b"kept\n" + text
    engine.free_table(engine.TABLE_FASTQ)
    with pytest.raises(_lib.LsgError, match="not formatted"):
        engine.table_bytes(engine.TABLE_FASTQ, 0)
    with pytest.raises(_lib.LsgError, match="lsg_bam_fastq"):    # the slot is not lsg_format_table's to make
        engine.format_table(engine.TABLE_FASTQ)


def test_a_resident_load_is_left_alone(engine, bams):
    from longsom_amd import tsvio
    bam = os.path.join(G, "pileup.rand.bam")
    bc = hostio.read_barcodes(os.path.join(G, "pileup.rand.barcodes.tsv"))
    _, seqs = tsvio.read_fasta(os.path.join(G, "pileup.rand.fa"))
    names, lens, first = hostio.bam_header(bam)
    engine.set_contigs(lens)
    for t, s in enumerate(seqs):
        engine.load_reference(t, np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8))
    engine.set_barcodes(bc.celltype_of, 2)
    engine.set_region()
    loaded, _, _ = engine.load_bam(bam, bc.barcodes, min_mapq=60, first_record_offset=first)
    shape = engine.reads_shape()
    before = (engine.pileup_count(), [tuple(a.tobytes() for a in engine.fetch_counts(ct)) for ct in range(2)])
    device_text(engine, bams["edge"])                             # other files' FASTQ, both modes, between two counts of the load
    device_text(engine, bams["routed"], bams["routed_table"], 30)
    dev, _ = device_text(engine, bam, bc, 60)                     # ... and the loaded file's own (some of its reads have no CB: routed)
    assert dev["n_records"] == loaded["n_records"] and sum(dev["n_printed"]) == loaded["pass_reads"]
    assert engine.reads_shape() == shape
    after = (engine.pileup_count(), [tuple(a.tobytes() for a in engine.fetch_counts(ct)) for ct in range(2)])
    assert after == before


def test_n_trim_is_refused(engine, bams):
    engine.set_split_filters(hostio.SplitFilters(n_trim=2))
    try:
        with pytest.raises(_lib.LsgError, match="n_trim"):
            engine.bam_fastq(bams["routed"], bams["routed_table"].barcodes, bams["routed_table"].celltype_of, 2, 30)
        engine.bam_fastq(bams["edge"])                            # plain mode has no filters
    finally:
        engine.set_split_filters(None)


def test_fusion_fastq_script_equals_the_host_chain(bams, tmp_path):
    """the rule's line through cli.fusion_fastq (an engine of its own): {id}.fastq and the per-cell-type files"""
    meta = os.path.join(bams["dir"], "routed.meta.tsv")
    cli.fusion_fastq(["--bam", bams["routed"], "--meta", meta, "--id", "S", "--outdir", str(tmp_path / "dev"), "--min_MQ", "30", "--max_nM=2", "--max_NH=",
                      "--per_celltype"])
    cli.fusion_fastq(["--bam", bams["routed"], "--meta", meta, "--id", "S", "--outdir", str(tmp_path / "host"), "--min_MQ", "30", "--max_nM=2", "--max_NH=",
                      "--per_celltype", "--host"])
    for name in ("S.fastq", "S.Cancer.fastq", "S.Non-Cancer.fastq"):
        assert read(str(tmp_path / "dev" / name)) == read(str(tmp_path / "host" / name)), name
    assert read(str(tmp_path / "dev" / "S.fastq")) == read(os.path.join(G, "fusion", "routed.nM2.fastq"))
    out = str(tmp_path / "p.fastq")
    cli.bam_to_fastq(["--bam", os.path.join(G, "fusion", "plain.bam"), "--fastq", out])
    assert read(out) == read(os.path.join(G, "fusion", "plain.fastq"))
