"""GPU: the cell-by-gene read count on the device (csrc/genecounts.hip) against the numpy twin (longsom_amd/genecounts.py) and the
hand-stated answers of tests/support/genecount_cases.py: matrix, tallies and the bytes of LSG_TABLE_GENE_COUNTS, for reads loaded as
arrays (load_reads) and as a BAM (load_bam); accumulation over two loads; the CLI; the fused run_snv hook; the refusals.  Exact."""
import os

import numpy as np
import pytest

from longsom_amd import cli, genecounts, hostio
from longsom_amd._lib import LsgError
from longsom_amd.engine import Engine
from tests.support import genecount_cases as gc

pytestmark = pytest.mark.gpu

HAND = {c["name"]: c for c in gc.HAND_CASES}


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    f = gc.fuzz_case()
    d = tmp_path_factory.mktemp("fuzz")
    f.update(name="fuzz", gtf_path=str(d / "fuzz.gtf"), min_mapq=gc.FUZZ_MIN_MAPQ, flag_exclude=gc.FUZZ_FLAG_EXCLUDE, gene_names="third", tsv=False)
    gc.write_gtf(f["gtf_path"], f["gtf"])
    f["ann"] = genecounts.load_annotation(f["gtf_path"], [n for n, _ in f["contigs"]])
    f["rows"], f["row_of_gene"] = genecounts.name_rows(f["ann"], f["gtf_path"], None, "third")
    f["rec"] = gc.records(f["reads"])
    f["order"] = genecounts.column_order(f["barcodes"])
    f["matrix"], f["tallies"] = genecounts.count(f["rec"], f["ann"], f["row_of_gene"], len(f["rows"]), len(f["barcodes"]), f["min_mapq"], f["flag_exclude"])
    f["text"] = genecounts.matrix_text(f["matrix"], f["rows"], f["barcodes"], f["order"])
    return f


def prepared(case, tmp_path):
    """a hand case with its annotation, rows and the twin's answers"""
    if "ann" in case:
        return case
    c = dict(case)
    p = gc.paths(tmp_path, c["name"])
    gc.write_gtf(p["gtf"], c["gtf"])
    c["gtf_path"] = p["gtf"]
    c["ann"] = genecounts.load_annotation(p["gtf"], [n for n, _ in c["contigs"]])
    c["rows"], c["row_of_gene"] = genecounts.name_rows(c["ann"], p["gtf"], None, c["gene_names"])
    c["rec"] = gc.records(c["reads"])
    c["order"] = genecounts.column_order(c["barcodes"])
    c["matrix"], tallies = genecounts.count(c["rec"], c["ann"], c["row_of_gene"], len(c["rows"]), len(c["barcodes"]), c["min_mapq"], c["flag_exclude"])
    np.testing.assert_array_equal(tallies, c["tallies"])
    return c


def bind(eng, c):
    eng.set_contigs([l for _, l in c["contigs"]])
    eng.set_barcodes(np.arange(len(c["barcodes"])) % 2, 2)


def count_resident(eng, c, reset=True):
    """annotation, count, text: (matrix, tallies, text, info) of the device"""
    if reset:
        eng.gene_counts_reset()
        eng.load_annotation(c["ann"], c["row_of_gene"], len(c["rows"]))
    info = eng.gene_counts(c["min_mapq"], c["flag_exclude"])
    eng.gene_counts_set_text(c["rows"], c["order"], c["barcodes"], "\t" if c["tsv"] else ",")
    n = eng.format_table(eng.TABLE_GENE_COUNTS)
    matrix, tallies = eng.gene_counts_fetch()
    return matrix, tallies, eng.table_bytes(eng.TABLE_GENE_COUNTS, n), info


def check(got, c):
    matrix, tallies, text, info = got
    np.testing.assert_array_equal(matrix.astype(np.int64), c["matrix"])
    np.testing.assert_array_equal(tallies.astype(np.int64), c["tallies"])
    assert text == c["text"]
    return info


@pytest.mark.parametrize("name", list(HAND) + ["fuzz"])
def test_device_equals_the_twin_for_arrays_and_for_a_bam(eng, name, fuzz, tmp_path):
    c = fuzz if name == "fuzz" else prepared(HAND[name], tmp_path)
    bind(eng, c)
    eng.load_reads(c["rec"])
    info = check(count_resident(eng, c), c)
    t = c["tallies"].sum(axis=0)
    assert [info[k] for k in ("n_assigned", "n_no_features", "n_ambiguity", "n_filtered")] == t.tolist()
    assert info["n_unlisted"] == int((c["rec"].read_cb < 0).sum()) and info["n_reads"] == c["rec"].n_reads and info["n_segs"] == c["rec"].n_segs
    # ... and the same reads as a BAM through the device ingest
    bam = os.path.join(str(tmp_path), name + ".bam")
    gc.write_bam(bam, c["contigs"], c["reads"], c["barcodes"])
    eng.load_bam(bam, c["barcodes"], min_mapq=0)
    check(count_resident(eng, c), c)
    eng.unload_reads()
    m, t2 = eng.gene_counts_fetch()                        # lsg_unload_reads leaves the matrix alone
    np.testing.assert_array_equal(m.astype(np.int64), c["matrix"])
    eng.gene_counts_reset()


def test_two_loads_accumulate(eng, fuzz):
    c = fuzz
    bind(eng, c)
    half = np.arange(c["rec"].n_reads) % 2 == 0
    eng.load_reads(c["rec"].subset(half))
    count_resident(eng, c)
    eng.load_reads(c["rec"].subset(~half))
    check(count_resident(eng, c, reset=False), c)
    eng.gene_counts_reset()


def test_refusals_and_a_smaller_annotation_after_reset(eng, tmp_path):
    c = prepared(HAND["main"], tmp_path)
    small = prepared(HAND["wide_one_row"], tmp_path)
    eng.gene_counts_reset()
    bind(eng, c)
    eng.load_reads(c["rec"])
    with pytest.raises(LsgError, match="no annotation"):
        eng.gene_counts()
    eng.load_annotation(c["ann"], c["row_of_gene"], len(c["rows"]))
    eng.unload_reads()
    with pytest.raises(LsgError, match="no reads"):
        eng.gene_counts()
    eng.load_reads(c["rec"])
    eng.gene_counts()
    eng.set_barcodes(np.zeros(7, np.uint8), 1)
    with pytest.raises(LsgError, match="barcodes"):
        eng.gene_counts()
    with pytest.raises(LsgError):                          # a label past the genes is refused at load, not followed
        bad = genecounts.Annotation(["g"], np.asarray([5], np.uint64), np.asarray([3], np.uint32), np.asarray([1], np.uint32))
        eng.load_annotation(bad, np.zeros(1, np.int32), 1)
    # after a reset a smaller annotation (one gene, one row) over other barcodes works
    bind(eng, small)
    eng.load_reads(small["rec"])
    check(count_resident(eng, small), small)
    eng.gene_counts_reset()
    with pytest.raises(LsgError):
        eng.format_table(eng.TABLE_GENE_COUNTS)


def test_cli_on_the_device_equals_host(tmp_path, fuzz):
    p = gc.paths(tmp_path, "cli")
    gc.write_meta(p["meta"], fuzz["barcodes"]); gc.write_bam(p["bam"], fuzz["contigs"], fuzz["reads"], fuzz["barcodes"])
    outs = {}
    for how in ("device", "host"):
        out = os.path.join(p["out"], how)
        cli.gene_counts(["--bam", p["bam"], "--meta", p["meta"], "--gtf", fuzz["gtf_path"], "--id", "S", "--outdir", out, "--min_MQ", str(gc.FUZZ_MIN_MAPQ), "--primary_only"]
                        + (["--host"] if how == "host" else []))
        outs[how] = [open(os.path.join(out, "S.counts." + n), "rb").read() for n in ("formated.txt", "summary.tsv")]
    assert outs["device"] == outs["host"] and outs["host"][0] == fuzz["text"]


def test_fused_run_snv_writes_the_same_file_and_the_same_snv_tables(tmp_path):
    from longsom_amd import pipeline, synth
    model = synth.named("C1", n_reads=3000)
    d = str(tmp_path)
    bam, fa, meta, gtf = (os.path.join(d, n) for n in ("s.bam", "ref.fa", "barcodes.tsv", "anno.gtf"))
    hostio.synth_bam(model, bam, fa)
    barcodes = hostio.synth_barcodes(model)
    hostio.write_barcodes_tsv(meta, barcodes, model.celltype_of, ["Cancer", "Non-Cancer"])
    names, lens, _ = hostio.bam_header(bam)
    rng = np.random.default_rng(5)
    lines = []
    for g in range(40):
        t = int(rng.integers(0, len(names))); at = int(rng.integers(0, max(1, int(lens[t]) - 3000)))
        lines.append('%s\tt\tgene\t1\t2\t.\t+\t.\tgene_id "E%d"; gene_type "pc"; gene_name "N%d";\n' % (names[t], g, g % 30))
        for _ in range(3):
            ln = int(rng.integers(50, 500))
            lines.append('%s\tt\texon\t%d\t%d\t.\t+\t.\tgene_id "E%d";\n' % (names[t], at + 1, min(at + ln, int(lens[t])), g)); at += ln + 200
    gc.write_gtf(gtf, "".join(lines))
    plain = pipeline.run_snv(bam, meta, fa, os.path.join(d, "plain"), "S")
    fused = pipeline.run_snv(bam, meta, fa, os.path.join(d, "fused"), "S", gene_counts=genecounts.Request(gtf, os.path.join(d, "fused", "gc")))
    for k in ("merged", "step1", "step2", "step3", "step3_unfiltered"):
        assert open(getattr(plain, k), "rb").read() == open(getattr(fused, k), "rb").read(), k
    for k in plain.counts:
        assert open(plain.counts[k], "rb").read() == open(fused.counts[k], "rb").read(), k
    cli.gene_counts(["--bam", bam, "--meta", meta, "--gtf", gtf, "--id", "S", "--outdir", os.path.join(d, "alone")])
    for n in ("S.counts.formated.txt", "S.counts.summary.tsv"):
        alone = open(os.path.join(d, "alone", n), "rb").read()
        assert alone == open(os.path.join(d, "fused", "gc", n), "rb").read(), n
    assert alone.count(b"\n") == 5 and sum(int(v) for v in alone.split(b"\n")[1].split(b"\t")[1:]) > 0      # the summary: some reads are assigned
