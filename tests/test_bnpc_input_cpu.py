"""CPU: the host half of the FormatInputBnpC step (longsom_amd/cellclust.py) against the reference-made fixtures tests/golden/bnpc.*
(tools/make_bnpc_goldens.py): the pandas twin byte for byte, the parser of the matrix files and what it hands back, col_int_ok, the flag
surface of the CLI, the rule and the shim.  The filters and the rows' text are the device's (tests/test_bnpc_input_gpu.py)."""
import os

import numpy as np
import pytest

from longsom_amd import cellclust, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
FUSIONS = os.path.join(G, "cellclust.fusions.tsv")


def matrix(run, name):
    p = os.path.join(G, "cellclust.%s.%s.tsv" % (run, name))
    return p if os.path.exists(p) else p + ".gz"


# (case, BinaryMatrix, VAFMatrix, barcodes, min_cells_per_mut, min_pos_cov)
CASES = [("rand.fusions.c0p8", matrix("rand.fusions", "BinaryMatrix"), matrix("rand.fusions", "VAFMatrix"), os.path.join(G, "bnpc.barcodes.tsv"), 0, 8),
         ("rand.All.c0p8", matrix("rand.All", "BinaryMatrix"), matrix("rand.All", "VAFMatrix"), os.path.join(G, "bnpc.barcodes.tsv"), 0, 8),
         ("rand.All.c1p3", matrix("rand.All", "BinaryMatrix"), matrix("rand.All", "VAFMatrix"), os.path.join(G, "bnpc.barcodes.tsv"), 1, 3),
         ("rand.All.c5p3", matrix("rand.All", "BinaryMatrix"), matrix("rand.All", "VAFMatrix"), os.path.join(G, "bnpc.barcodes.tsv"), 5, 3),
         ("small.c1p2", os.path.join(G, "bnpc.small.in.BinaryMatrix.tsv"), os.path.join(G, "bnpc.small.in.VAFMatrix.tsv"), os.path.join(G, "bnpc.small.barcodes.tsv"), 1, 2)]


def golden(case, name):
    return open(os.path.join(G, "bnpc.%s.%s.tsv" % (case, name))).read()


def assert_outputs_equal_golden(prefix, case):
    for o in cellclust.BNPC_OUTPUTS:
        assert open(prefix + "." + o + ".tsv").read() == golden(case, o), "%s of case %s differs from the reference's" % (o, case)


@pytest.mark.parametrize("case,bin_path,vaf_path,barcodes,c,p", CASES)
def test_twin_reproduces_the_goldens(tmp_path, case, bin_path, vaf_path, barcodes, c, p):
    prefix = str(tmp_path / "t")
    n_rows, n_cols = cellclust.format_bnpc_input_host(bin_path, vaf_path, barcodes, prefix, c, p)
    assert_outputs_equal_golden(prefix, case)
    body = golden(case, "BinaryMatrix").split("\n")[1:-1]
    assert n_rows == len(body) and n_cols == (len(body[0].split("\t")) - 1 if body else 0)


def test_goldens_are_not_trivial():
    """what the cases were chosen for is in the files"""
    fus = golden("rand.fusions.c0p8", "BinaryMatrix").split("\n")
    assert len(fus[0].split("\t")) == 24 and "GGGG9999TT" not in fus[0] and [l.split("\t")[0] for l in fus[-4:-1]] == ["ABC1--DEF2", "ABC1--DEF10", "GENEA--GENEB"]
    assert golden("rand.All.c1p3", "BinaryMatrix") == '""\nchr10:1501:N\n' and golden("rand.All.c5p3", "VAFMatrix") == '""\n'
    small = golden("small.c1p2", "BinaryMatrix").split("\n")
    assert small[0].split("\t") == ["", "B01", "B02", "B03", "B04"]                      # B06's coverage equals min_pos_cov: dropped; B04's is one more
    assert [l.split("\t")[0] for l in small[1:-1]] == ["chr1:10:A", "chr1:30:G", "chr2:5:T", "chr2:9:A", "G1--G2"]      # chr1:20:C has min_cells_per_mut 1s
    assert small[2] == "chr1:30:G\t1\t1.0\t1\t0.0" and small[5] == "G1--G2\t1\t1.0\t1\t1.0"      # integer columns beside float ones
    bc = golden("small.c1p2", "Barcodes").split("\n")
    assert bc[0].split("\t")[-1] == "Cell_Reanno_Colors" and [l.split("\t")[0] for l in bc[1:-1]] == ["B03", "B01", "B04", "B02"]
    assert bc[1].endswith("\tCancer\t#8F79A1") and bc[3].endswith("\tNon-Cancer\t#94C773")


def test_parser_of_the_matrix_files():
    columns, labels, bin_, vaf4, f_labels, f_bin, f_vaf4, int_ok = cellclust.read_bnpc_matrices(*CASES[4][1:3])
    assert columns == ["B%02d" % i for i in range(1, 8)] and labels[:2] == ["chr1:10:A", "chr1:20:C"] and f_labels == ["G1--G2"]
    assert bin_.shape == (6, 7) and bin_[0].tolist() == [1, 1, 0, 3, 3, 0, 3] and vaf4[0].tolist() == [5000, 10000, 0, -1, -1, 0, -1]
    assert f_bin.tolist() == [[1] * 7] and f_vaf4.tolist() == [[10000] * 7]
    assert int_ok.tolist() == [1, 0, 1, 0, 0, 0, 0]                                      # a 3 anywhere makes the column float
    columns, labels, bin_, vaf4, f_labels, f_bin, f_vaf4, int_ok = cellclust.read_bnpc_matrices(*CASES[0][1:3])
    assert len(columns) == 26 and len(labels) == 59 and len(f_labels) == 3 and not int_ok.any()      # every cell of the fusion run is float text
    assert f_bin[:, columns.index("GGGG9999TT")].tolist() == [1, 3, 3] and (bin_[:, columns.index("GGGG9999TT")] == 3).all()
    assert ((vaf4 < 0) == (bin_ == 3)).all()


def write_pair(tmp_path, bin_rows, vaf_rows, columns=("A", "B")):
    paths = []
    for name, rows in (("b.tsv", bin_rows), ("v.tsv", vaf_rows)):
        p = tmp_path / name
        p.write_text("\t".join(("",) + tuple(columns)) + "\n" + "".join("\t".join(r) + "\n" for r in rows))
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("what,bin_rows,vaf_rows", [
    ("a VAF text of five decimals", [("r1", "1", "0"), ("r2", "1", "3")], [("r1", "0.33333", "0.0"), ("r2", "1.0", ".")]),
    ("a duplicated label", [("r1", "1", "0"), ("r1", "1", "3")], [("r1", "0.5", "0.0"), ("r1", "1.0", ".")]),
    ("a Binary value of 2", [("r1", "2", "0"), ("r2", "1", "3")], [("r1", "0.5", "0.0"), ("r2", "1.0", ".")]),
    ("a VAF column of integers", [("r1", "1", "0"), ("r2", "1", "3")], [("r1", "1", "0.0"), ("r2", "1", ".")]),
    ("a VAF text inf", [("r1", "1", "0"), ("r2", "1", "3")], [("r1", "inf", "0.0"), ("r2", "1.0", ".")]),
])
def test_hand_back_gives_the_twins_bytes(tmp_path, what, bin_rows, vaf_rows):
    """a file the device form does not state: the parser refuses it and format_bnpc_input_files writes what the twin writes, without a device"""
    b, v = write_pair(tmp_path, bin_rows, vaf_rows)
    with pytest.raises(cellclust.HandBack):
        cellclust.read_bnpc_matrices(b, v)
    barcodes = tmp_path / "bc.tsv"
    barcodes.write_text("Index\tCell_type\tReannotated_cell_type\nB\tCancer\tNon-Cancer\nA\tCancer\tCancer\n")
    got = cellclust.format_bnpc_input_files(None, b, v, str(barcodes), str(tmp_path / "dev"), 0, 0)
    assert got[2] == "host"
    cellclust.format_bnpc_input_host(b, v, str(barcodes), str(tmp_path / "twin"), 0, 0)
    for o in cellclust.BNPC_OUTPUTS:
        assert open(str(tmp_path / "dev") + "." + o + ".tsv").read() == open(str(tmp_path / "twin") + "." + o + ".tsv").read()
    if what == "a VAF text of five decimals":
        assert "\t0.33333\t" in open(str(tmp_path / "dev") + ".VAFMatrix.tsv").read()


def test_col_int_ok_with_and_without_fusions():
    cols = ["A", "B", "C"]
    assert cellclust.bnpc_col_int_ok(cols, [], False) == [1, 1, 1]                       # no fusion, no gap: the device's coverage decides alone
    assert cellclust.bnpc_col_int_ok(cols, [], True) == [0, 0, 0]
    every = [("F--G", c) for c in cols]
    assert cellclust.bnpc_col_int_ok(cols, every, False) == [1, 1, 1]                    # every barcode carries the one fusion
    assert cellclust.bnpc_col_int_ok(cols, every[:2], True) == [0, 0, 0]                 # a gap: SingleCellGenotype printed floats everywhere
    assert cellclust.bnpc_col_int_ok(cols, every[:2], False) == [1, 1, 0]                # (not a state matrix_columns gives: the rule per column)
    # the fixtures: the fusion run's matrices are all floats, the plain run's columns are left to their coverage
    from tests.test_cellclust_cpu import barcodes_of
    fusions = cellclust.read_fusions(FUSIONS)
    columns, _, float_cells = cellclust.matrix_columns(barcodes_of("rand.fusions"), fusions, 59)
    assert float_cells and not any(cellclust.bnpc_col_int_ok(columns, fusions, float_cells))
    columns, _, float_cells = cellclust.matrix_columns(barcodes_of("rand.All"), [], 59)
    assert not float_cells and all(cellclust.bnpc_col_int_ok(columns, [], float_cells))


def test_cli_parser_takes_the_reference_rule_line():
    from tests.test_rules_cpu import parser_of
    p = parser_of(cli.format_input_bnpc)
    a = p.parse_args("--bin s.BinaryMatrix.tsv --vaf s.VAFMatrix.tsv --barcodes s.tsv --min_pos_cov 3 --min_cells_per_mut 5 --outfile CellClustering/BnpC_input//s".split())
    assert (a.bin, a.vaf, a.barcodes, a.min_pos_cov, a.min_cells_per_mut, a.outfile) == ("s.BinaryMatrix.tsv", "s.VAFMatrix.tsv", "s.tsv", 3, 5, "CellClustering/BnpC_input//s")
    a = p.parse_args("--bin b --vaf v --barcodes m".split())
    assert (a.min_cells_per_mut, a.min_pos_cov, a.outfile) == (5, 3, "Matrix.tsv")         # FormatInputBnpC.py:42-44
    with pytest.raises(SystemExit):
        p.parse_args(["--bin", "b", "--vaf", "v"])
    # the fused form: SingleCellGenotype's parser with the three optional flags, unchanged without them
    q = parser_of(cli.cell_genotype_matrices)
    base = "--bam b --infile i --ref r --meta m --fusions".split()
    a = q.parse_args(base)
    assert not a.bnpc_outfile and not q.parse_args(base + ["--bnpc_outfile", "--min_pos_cov", "3"]).bnpc_outfile and (a.min_cells_per_mut, a.min_pos_cov) == (5, 3)
    a = q.parse_args(base + "--bnpc_outfile CellClustering/BnpC_input/s --min_cells_per_mut 2 --min_pos_cov 7".split())
    assert (a.bnpc_outfile, a.min_cells_per_mut, a.min_pos_cov) == ("CellClustering/BnpC_input/s", 2, 7)
    # ... and on that script alone: the HCCV genotyping drop-in (CellTypeReannotation) does not know the flags
    hccv = parser_of(cli.single_cell_genotype)
    assert not {"--bnpc_outfile", "--bnpc_barcodes", "--min_cells_per_mut", "--min_pos_cov"} & set(hccv._option_string_actions)


def test_rule_and_shim_exist():
    smk = open(os.path.join(ROOT, "workflow", "rules", "CellClustering.gpu.smk")).read()
    assert "rule FormatInputBnpC:" in smk and "fuse_bnpc_input" in smk and "stay the reference's" not in smk
    for out in cellclust.BNPC_OUTPUTS:
        assert "CellClustering/BnpC_input/{id}." + out + ".tsv" in smk
    for key in ("min_cells_per_mut", "min_pos_cov"):
        assert "config['CellClust']['FormatInput']['%s']" % key in smk
    shim = open(os.path.join(ROOT, "workflow", "scripts_gpu", "CellClustering", "FormatInputBnpC.py")).read()
    assert "cli.format_input_bnpc()" in shim
