"""CPU: the cell-by-gene read count's host side (longsom_amd/genecounts.py) - the GTF reader, the flattening into elementary intervals,
the numpy twin that states the contract, the text - against the hand-stated cases of tests/support/genecount_cases.py, a brute-force
all-reads x all-exons count on the seeded fuzz case, and pandas for format_featureCount's own steps (CNACalling.smk:66-72).  Every
comparison is exact."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from longsom_amd import cli, genecounts
from tests.support import genecount_cases as gc

HAND = {c["name"]: c for c in gc.HAND_CASES}


def annotate(case, tmp_path):
    p = gc.paths(tmp_path, case["name"])
    gc.write_gtf(p["gtf"], case["gtf"])
    ann = genecounts.load_annotation(p["gtf"], [n for n, _ in case["contigs"]])
    rows, row_of_gene = genecounts.name_rows(ann, p["gtf"], None, case["gene_names"])
    return p, ann, rows, row_of_gene


def twin(case, tmp_path):
    p, ann, rows, row_of_gene = annotate(case, tmp_path)
    order = genecounts.column_order(case["barcodes"])
    matrix, tallies = genecounts.count(gc.records(case["reads"]), ann, row_of_gene, len(rows), len(case["barcodes"]), case["min_mapq"], case["flag_exclude"])
    return rows, matrix, tallies, genecounts.matrix_text(matrix, rows, case["barcodes"], order, "\t" if case["tsv"] else ",")


def test_the_flattening_is_the_hand_stated_one(tmp_path):
    _, ann, _, _ = annotate(HAND["main"], tmp_path)
    assert ann.gene_ids == gc.MAIN_GENE_IDS and ann.n_dropped_exons == 1
    got = [(int(k) >> 32, int(k) & 0xFFFFFFFF, int(l), "*" if lab == genecounts.AMBIG else ann.gene_ids[lab]) for k, l, lab in zip(ann.keys, ann.lens, ann.labels)]
    assert got == gc.MAIN_INTERVALS


@pytest.mark.parametrize("name", ["main", "wide_one_row"])
def test_the_flattening_equals_a_per_base_labelling(name, tmp_path):
    case = HAND[name]
    p, ann, _, _ = annotate(case, tmp_path)
    ex = genecounts.read_exons(p["gtf"])
    names = [n for n, _ in case["contigs"]]
    flat = {}                                             # (tid, pos) -> label, from the intervals
    for k, l, lab in zip(ann.keys, ann.lens, ann.labels):
        for q in range(int(l)):
            assert (int(k) + q) not in flat, "intervals overlap"
            flat[int(k) + q] = int(lab)
    brute = {}                                            # ... and base by base from the exons
    for g, c, s, e in zip(ex.gene, ex.contig, ex.start0, ex.end0):
        if c in names:
            for q in range(int(s), int(e)):
                brute.setdefault((names.index(c) << 32) + q, set()).add(int(g))
    assert flat == {k: (next(iter(v)) if len(v) == 1 else genecounts.AMBIG) for k, v in brute.items()}
    assert np.all(ann.keys[1:] >= ann.keys[:-1] + ann.lens[:-1].astype(np.uint64)) and np.all(ann.lens > 0)


@pytest.mark.parametrize("name", list(HAND))
def test_the_twin_gives_the_hand_stated_answers(name, tmp_path):
    case = HAND[name]
    rows, matrix, tallies, text = twin(case, tmp_path)
    assert rows == case["rows"]
    np.testing.assert_array_equal(tallies, case["tallies"])
    assert text == case["text"]
    assert int(matrix.sum()) <= int(tallies[:, 0].sum())          # (an assigned read of an unnamed gene is in no row)


def test_the_summary_is_the_hand_stated_one(tmp_path):
    case = HAND["main"]
    _, _, tallies, _ = twin(case, tmp_path)
    assert genecounts.summary_text(tallies, case["barcodes"], genecounts.column_order(case["barcodes"])) == gc.MAIN_SUMMARY


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    f = gc.fuzz_case()
    d = tmp_path_factory.mktemp("fuzz")
    f["gtf_path"] = str(d / "fuzz.gtf")
    gc.write_gtf(f["gtf_path"], f["gtf"])
    f["ann"] = genecounts.load_annotation(f["gtf_path"], [n for n, _ in f["contigs"]])
    f["rec"] = gc.records(f["reads"])
    return f


def brute_force(f, min_mapq, flag_exclude):
    """every read against every exon: per read the set of genes whose exons its blocks overlap.  Returns (per gene [n_genes][n_cb], tallies)"""
    rec, n_cb = f["rec"], len(f["barcodes"])
    ex = np.asarray(f["exons"], np.int64)
    seg_tid = rec.read_tid[rec.seg_read].astype(np.int64)
    s0 = rec.seg_start.astype(np.int64); s1 = s0 + rec.seg_len
    pairs = set()
    for tid in range(len(f["contigs"])):
        segs = np.nonzero(seg_tid == tid)[0]; e = ex[ex[:, 1] == tid]
        hit = (s0[segs, None] < e[None, :, 3]) & (e[None, :, 2] < s1[segs, None])
        si, ei = np.nonzero(hit)
        pairs.update(zip(rec.seg_read[segs[si]].tolist(), e[ei, 0].tolist()))
    genes_of = {}
    for r, g in pairs:
        genes_of.setdefault(r, set()).add(g)
    per_gene = np.zeros((f["n_genes"], n_cb), np.int64); tallies = np.zeros((n_cb, 4), np.int64)
    for r in range(rec.n_reads):
        cb = int(rec.read_cb[r])
        if cb < 0:
            continue
        if (int(rec.read_flag[r]) & flag_exclude) or int(rec.read_mapq[r]) < min_mapq:
            tallies[cb, 3] += 1
            continue
        gs = genes_of.get(r, ())
        tallies[cb, 0 if len(gs) == 1 else 1 if not gs else 2] += 1
        if len(gs) == 1:
            per_gene[next(iter(gs)), cb] += 1
    return per_gene, tallies


def test_the_twin_equals_a_brute_force_count_on_the_fuzz_case(fuzz):
    assert fuzz["ann"].gene_ids == fuzz["gene_ids"]       # (every gene has an exon line, in order)
    per_gene, tallies = genecounts.count_genes(fuzz["rec"], fuzz["ann"], len(fuzz["barcodes"]), gc.FUZZ_MIN_MAPQ, gc.FUZZ_FLAG_EXCLUDE)
    want_genes, want_tallies = brute_force(fuzz, gc.FUZZ_MIN_MAPQ, gc.FUZZ_FLAG_EXCLUDE)
    np.testing.assert_array_equal(tallies, want_tallies)
    np.testing.assert_array_equal(per_gene, want_genes)
    per_outcome = tallies.sum(axis=0)
    print("fuzz case: reads per outcome (Assigned, NoFeatures, Ambiguity, Filtered) = %s, ambiguous intervals %d of %d" %
          (per_outcome.tolist(), int((fuzz["ann"].labels == genecounts.AMBIG).sum()), fuzz["ann"].n_intervals))
    assert per_outcome.min() >= 500, "an outcome is nearly empty: %s" % per_outcome.tolist()
    assert int((fuzz["rec"].read_cb < 0).sum()) >= 500


@pytest.mark.parametrize("rule", ["third", "gene_name", "none"])
def test_the_text_is_what_pandas_writes(fuzz, rule):
    """format_featureCount's own last steps over the per-gene-id table: map, notnull, groupby('Geneid').sum(), to_csv (CNACalling.smk:69-72)"""
    ann, barcodes = fuzz["ann"], fuzz["barcodes"]
    order = genecounts.column_order(barcodes)
    per_gene, _ = genecounts.count_genes(fuzz["rec"], ann, len(barcodes), gc.FUZZ_MIN_MAPQ, gc.FUZZ_FLAG_EXCLUDE)
    rows, row_of_gene = genecounts.name_rows(ann, fuzz["gtf_path"], None, rule)
    matrix, _ = genecounts.count(fuzz["rec"], ann, row_of_gene, len(rows), len(barcodes), gc.FUZZ_MIN_MAPQ, gc.FUZZ_FLAG_EXCLUDE)
    df = pd.DataFrame(per_gene[:, order], columns=[barcodes[i] for i in order])
    df.insert(0, "Geneid", ann.gene_ids)
    if rule != "none":
        dico = genecounts.read_name_map(fuzz["gtf_path"], rule)
        assert 0 < len(dico) < ann.n_genes and len(set(dico.values())) < len(dico)      # unnamed ids and shared names both occur
        df["Geneid"] = df["Geneid"].map(dico)
        df = df[df["Geneid"].notnull()]
    df = df.groupby("Geneid").sum()
    for sep in (",", "\t"):
        assert genecounts.matrix_text(matrix, rows, barcodes, order, sep) == df.to_csv(sep=sep).encode()


def test_a_name_with_a_comma_is_refused(tmp_path):
    p = gc.paths(tmp_path, "comma")
    gc.write_gtf(p["gtf"], gc.WIDE_GTF.replace('"Solo"', '"So,lo"'))
    ann = genecounts.load_annotation(p["gtf"], ["chr1"])
    with pytest.raises(ValueError, match="So,lo"):
        genecounts.name_rows(ann, p["gtf"], None, "third")
    assert genecounts.name_rows(ann, p["gtf"], None, "none")[0] == ["G1"]
    with pytest.raises(ValueError, match="gene_names"):
        genecounts.name_rows(ann, p["gtf"], None, "fourth")


@pytest.mark.parametrize("name", ["main", "main_min_mq_10", "main_primary_only", "main_tsv", "main_gene_name", "main_ids"])
def test_cli_host_over_a_bam(name, tmp_path, capsys):
    case = HAND[name]
    p = gc.paths(tmp_path, name)
    gc.write_gtf(p["gtf"], case["gtf"]); gc.write_meta(p["meta"], case["barcodes"]); gc.write_bam(p["bam"], case["contigs"], case["reads"], case["barcodes"])
    argv = ["--bam", p["bam"], "--meta", p["meta"], "--gtf", p["gtf"], "--id", "S1", "--outdir", p["out"], "--host", "--min_MQ", str(case["min_mapq"]),
            "--gene_names", case["gene_names"]] + (["--primary_only"] if case["primary_only"] else []) + (["--tsv"] if case["tsv"] else [])
    cli.gene_counts(argv)
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert open(os.path.join(p["out"], "S1.counts.formated.txt"), "rb").read() == case["text"]
    summary = open(os.path.join(p["out"], "S1.counts.summary.tsv"), "rb").read()
    if name == "main":
        assert summary == gc.MAIN_SUMMARY
    order = genecounts.column_order(case["barcodes"])
    assert summary == genecounts.summary_text(case["tallies"], case["barcodes"], order)
    assert said["counted_on"] == "host" and said["exons_on_absent_contigs"] == 1 and said["reads"]["Assigned"] == int(case["tallies"][:, 0].sum())


def test_cli_refuses_an_unknown_name_rule(tmp_path):
    with pytest.raises(SystemExit):
        cli.gene_counts(["--bam", "b", "--meta", "m", "--gtf", "g", "--gene_names", "1"])


def test_sharded_and_windowed_runs_refuse_the_fused_hook(tmp_path):
    from longsom_amd import pipeline

    class Two:
        world, rank, local_device_index = 2, 0, 0
    req = genecounts.Request("g.gtf", str(tmp_path))
    with pytest.raises(ValueError, match="counted twice"):
        pipeline.run_snv("b", "m", "r", str(tmp_path), "S", gene_counts=req, comm=Two())
    with pytest.raises(ValueError, match="counted twice"):
        pipeline.run_snv("b", "m", "r", str(tmp_path), "S", gene_counts=req, window_bytes=1 << 20)
