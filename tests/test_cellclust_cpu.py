"""CPU: the host half of the SingleCellGenotype step (longsom_amd/cellclust.py) against the reference-made fixtures
tests/golden/cellclust.* (tools/make_cellclust_goldens.py): the matrices' row order, their columns, the fusion rows, and the flag
surface of the CLI.  The cells themselves are the device's (tests/test_cellclust_gpu.py)."""
import gzip
import os
import random

import pytest

from longsom_amd import cellclust, cli, hostio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
RUNS = ["rand.All", "rand.Alt", "randsfx.All", "rand.p002", "rand.fusions"]
MATRIX_FILES = ["DpMatrix", "AltMatrix", "VAFMatrix", "BinaryMatrix"]
FUSIONS = os.path.join(G, "cellclust.fusions.tsv")


def golden(run, name):
    """a fixture's text (all but the fusion run's matrices are committed gzipped)"""
    path = os.path.join(G, "cellclust.%s.%s.tsv" % (run, name))
    return open(path).read() if os.path.exists(path) else gzip.open(path + ".gz", "rt", newline="").read()


def barcodes_of(run):
    return hostio.read_barcodes(os.path.join(G, "pileup.%s.barcodes.tsv" % run.split(".")[0])).barcodes


@pytest.mark.parametrize("name", MATRIX_FILES)
@pytest.mark.parametrize("run", RUNS)
def test_row_order_from_shuffled_rows(run, name):
    """sort_chr_index: every golden matrix's first column comes back, in order, from its own rows shuffled"""
    labels = [l.split("\t")[0] for l in golden(run, name).split("\n")[1:] if l]
    fusion_names = {f for f, _ in cellclust.read_fusions(FUSIONS)} if run == "rand.fusions" else set()
    assert len(labels) == 59 + len(fusion_names) and labels[0] == "chr1:17:A"
    index = [("zzz:" + l) if l in fusion_names else l for l in labels]                 # the pivot's index, before sort_chr_index renames it
    rng = random.Random(len(run) * 31 + len(name))
    for _ in range(3):
        shuffled = index[:]
        rng.shuffle(shuffled)
        order = cellclust.matrix_row_order(shuffled)
        assert [cellclust.matrix_label(shuffled[i]) for i in order] == labels
    chroms = [l.split(":")[0] for l in labels if ":" in l]
    assert [c for i, c in enumerate(chroms) if i == 0 or chroms[i - 1] != c] == ["chr1", "chr2", "chr10", "chrM"]      # natural, chrM last


def test_natural_key():
    k = cellclust.natural_key
    assert k("chr10:491:D") == ("chr", 10, ":", 491, ":D") and k("7abc") == ("", 7, "abc") and k("x") == ("x",) and k("") == ()
    names = ["chr2:5:A", "chr10:5:A", "chr1:50000:C", "chr1:49999:A", "chrX:1:T", "chrM:3:G", "zzz:B--C", "chr1:7:I"]
    assert [names[i] for i in cellclust.matrix_row_order(names)] == ["chr1:7:I", "chr1:49999:A", "chr1:50000:C", "chr2:5:A", "chr10:5:A", "chrX:1:T", "chrM:3:G", "zzz:B--C"]


@pytest.mark.parametrize("run", RUNS)
def test_columns_and_float_switch(run):
    """columns, col_src and float_cells from (barcodes, fusion file) against the golden headers and cells"""
    barcodes = barcodes_of(run)
    fusions = cellclust.read_fusions(FUSIONS if run == "rand.fusions" else None)
    columns, col_src, float_cells = cellclust.matrix_columns(barcodes, fusions, 59)
    for name in MATRIX_FILES:
        assert golden(run, name).split("\n")[0] == "\t".join([""] + columns)
    assert [barcodes[s] if s >= 0 else None for s in col_src] == [c if c in barcodes else None for c in columns]
    first_dp_cell = golden(run, "DpMatrix").split("\n")[1].split("\t")[1]
    assert float_cells == ("." in first_dp_cell) == (run == "rand.fusions")
    if run == "rand.fusions":
        assert col_src.count(-1) == 1 and columns[col_src.index(-1)] == "GGGG9999TT" and len(columns) == len(barcodes) + 1
    else:
        assert columns == sorted(barcodes) and -1 not in col_src


def test_float_switch_without_gaps():
    """every (row, column) pair present: the pivot holds no NaN and pandas keeps the integers"""
    assert cellclust.matrix_columns(["A", "B"], [("F", "A"), ("F", "B")], 0) == (["A", "B"], [-1, -1], False)
    assert cellclust.matrix_columns(["A", "B"], [("F", "A"), ("G", "B")], 0) == (["A", "B"], [-1, -1], True)
    assert cellclust.matrix_columns(["A", "B"], [("F", "A")], 2) == (["A", "B"], [0, 1], True)
    assert cellclust.matrix_columns(["A", "B"], [], 3) == (["A", "B"], [0, 1], False)


def test_fusion_pairs_and_rows():
    fusions = cellclust.read_fusions(FUSIONS)
    assert len(fusions) == 5 and len(set(fusions)) == 5                                  # six lines, one pair twice
    assert cellclust.read_fusions(None) == [] and cellclust.read_fusions("") == []
    columns, _, float_cells = cellclust.matrix_columns(barcodes_of("rand.fusions"), fusions, 59)
    rows = cellclust.fusion_rows(fusions, columns, float_cells)
    for m, name in zip(cellclust.MATRICES, MATRIX_FILES):
        want = [l + "\n" for l in golden("rand.fusions", name).split("\n")[60:] if l]
        by_label = {line.split("\t")[0]: line for _, line in rows[m]}
        assert [by_label[w.split("\t")[0]] for w in want] == want and len(by_label) == len(want) == 3
    assert "\t1.0\t" in rows["Dp"][0][1] and "\t1\t" in rows["VAF"][0][1]


def test_fusion_file_without_rows(tmp_path):
    p = tmp_path / "empty.tsv"
    p.write_text("#FusionName\tBC\tLeftBreakpoint\n")
    assert cellclust.read_fusions(str(p)) == []


def test_sites_of_the_target_file():
    """plan_sites: 60 lines, 59 sites (chr2:330 is named twice: the last line's ALT wins), the long table's site order = the golden's"""
    keys, alt_sym, is_chrm, group_off, heads, indexes, long_order = cellclust.plan_sites(os.path.join(G, "cellclust.targets.tsv"), ["chr1", "chr10", "chr2", "chrM"], 50000, "True")
    assert len(keys) == 59 and sorted(long_order) == list(range(59)) and list(keys) == sorted(keys)
    assert "chr2:330:G" in indexes and "chr2:330:D" not in indexes
    rows = [l.split("\t") for l in golden("rand.All", "SingleCellGenotype").split("\n")[1:] if l]
    seen = list(dict.fromkeys(r[15] for r in rows))
    assert [indexes[i] for i in long_order] == seen
    assert ["\t".join(r[:7]) for r in rows[::25]] == [heads[i] for i in long_order]
    assert [bool(f) for f in is_chrm] == [s.startswith("chrM:") for s in indexes]
    assert len(group_off) - 1 == 5                                                       # chr1 below / from 50000, chr10, chr2, chrM
    assert not cellclust.plan_sites(os.path.join(G, "cellclust.targets.tsv"), ["chr1", "chr10", "chr2", "chrM"], 50000, "False")[2].any()


def test_cli_parser_takes_the_reference_rule_line():
    from tests.test_rules_cpu import parser_of
    p = parser_of(cli.cell_genotype_matrices)
    line = ("--infile s.calling.step3.tsv --outfile CellClustering/SingleCellGenotype/s --bam s.bam --meta s.tsv --ref genome.fa --fusions %s --nprocs 32 --min_mq 255 "
            "--pvalue 0.01 --alpha2 0.2474528917555431 --beta2 162.03696139428595 --alt_flag All --chrM_contaminant True --tmp_dir CellClustering/SingleCellGenotype/s/")
    a = p.parse_args((line % "s.Fusions.SingleCellGenotype.tsv").split())
    assert a.fusions == "s.Fusions.SingleCellGenotype.tsv" and a.outfile.endswith("/s") and a.min_bq == 30 and a.bin == 50000
    a = p.parse_args((line % "").split())                                                 # Run.FusionCalling False: a bare --fusions
    assert a.fusions == "" and a.alpha2 == 0.2474528917555431 and a.beta2 == 162.03696139428595 and a.pvalue == 0.01
    with pytest.raises(SystemExit):                                                       # required, as in the reference (:387)
        p.parse_args(["--bam", "b", "--infile", "i", "--ref", "r", "--meta", "m"])


def test_rule_and_shim_exist():
    smk = open(os.path.join(ROOT, "workflow", "rules", "CellClustering.gpu.smk")).read()
    assert "rule SingleCellGenotype:" in smk
    for out in ("SingleCellGenotype.tsv", "DpMatrix.tsv", "AltMatrix.tsv", "VAFMatrix.tsv", "BinaryMatrix.tsv"):
        assert "CellClustering/SingleCellGenotype/{id}." + out in smk
    shim = open(os.path.join(ROOT, "workflow", "scripts_gpu", "CellClustering", "SingleCellGenotype.py")).read()
    assert "cli.cell_genotype_matrices()" in shim and len(shim.rstrip("\n").split("\n")) == 11
