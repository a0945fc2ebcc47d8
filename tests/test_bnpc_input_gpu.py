"""GPU: the FormatInputBnpC step (csrc/cellgeno.hip lsg_cellgeno_filter / LSG_TABLE_BNPC_*, longsom_amd/cellclust.py) - the file-in form
and the fused form against the reference-made fixtures tests/golden/bnpc.* byte for byte, grids of cells against numpy (the filter's
counts and flags) and against the pandas twin run on the matrices the device itself printed (the three files), and the error paths.
Every comparison is exact: bytes or integers."""
import os

import numpy as np
import pytest

from longsom_amd import cellclust, cli
from tests.test_bnpc_input_cpu import CASES, G, assert_outputs_equal_golden

pytestmark = pytest.mark.gpu


# ---- 1. the file-in form against the reference's files ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,bin_path,vaf_path,barcodes,c,p", CASES)
def test_file_in_form_equals_the_reference(engine, tmp_path, case, bin_path, vaf_path, barcodes, c, p):
    prefix = str(tmp_path / "d")
    n_rows, n_cols, how = cellclust.format_bnpc_input_files(engine, bin_path, vaf_path, barcodes, prefix, c, p)
    assert how == "device"
    assert_outputs_equal_golden(prefix, case)
    body = open(prefix + ".BinaryMatrix.tsv").read().split("\n")[1:-1]
    assert n_rows == len(body) and n_cols == (len(body[0].split("\t")) - 1 if body else 0)
    if case == "small.c1p2":
        f = engine.cellgeno_filter_fetch()
        assert f["row_mut"].tolist() == [2, 1, 3, 3, 3, 0] and f["row_keep"].tolist() == [1, 0, 1, 1, 1, 0]
        assert f["col_cov_kept"].tolist() == [4, 4, 4, 3, 1, 2, 0] and f["col_keep"].tolist() == [1, 1, 1, 1, 0, 0, 0]
        assert f["col_cov_all"].tolist() == [6, 5, 6, 4, 2, 2, 0] and f["col_int"].tolist() == [1, 0, 1, 0, 0, 0, 0]


def test_drop_in_script_entry(tmp_path):
    """the rule's line through cli.format_input_bnpc (an engine of its own)"""
    case, bin_path, vaf_path, barcodes, c, p = CASES[4]
    prefix = str(tmp_path / "BnpC_input" / "s")
    cli.format_input_bnpc(["--bin", bin_path, "--vaf", vaf_path, "--barcodes", barcodes, "--min_pos_cov", str(p), "--min_cells_per_mut", str(c), "--outfile", prefix])
    assert_outputs_equal_golden(prefix, case)


# ---- 2. the fused form: SingleCellGenotype writes BnpC's input from the resident cells --------------------------------------------
@pytest.mark.parametrize("run,case,extra", [("rand.All", "rand.All.c0p8", []), ("rand.fusions", "rand.fusions.c0p8", [os.path.join(G, "cellclust.fusions.tsv")])])
def test_fused_form_equals_the_reference(tmp_path, run, case, extra):
    from tests.test_cellclust_cpu import golden as matrix_golden
    prefix, bnpc = str(tmp_path / "s"), str(tmp_path / "bnpc")
    cli.cell_genotype_matrices(["--bam", os.path.join(G, "pileup.rand.bam"), "--infile", os.path.join(G, "cellclust.targets.tsv"), "--ref", os.path.join(G, "pileup.rand.fa"),
                                "--meta", os.path.join(G, "pileup.rand.barcodes.tsv"), "--outfile", prefix, "--nprocs", "1", "--min_mq", "60", "--tmp_dir", str(tmp_path / "tmp"),
                                "--chrM_contaminant", "True", "--alt_flag", "All", "--bnpc_outfile", bnpc, "--bnpc_barcodes", os.path.join(G, "bnpc.barcodes.tsv"),
                                "--min_cells_per_mut", "0", "--min_pos_cov", "8", "--fusions"] + extra)
    for o in ("BinaryMatrix", "VAFMatrix"):                                               # the matrices the goldens were made from
        assert open(prefix + "." + o + ".tsv").read() == matrix_golden(run, o)
    assert_outputs_equal_golden(bnpc, case)


# ---- 3. grids of cells: the filter against numpy, the files against the twin on the device's own matrices ------------------------
def make_grid(n_rows, n_cb, seed):
    """dp / alt of cells that are NoCoverage (3), NoAltReads / BetaBin_problem (0) or PASS (1); barcode 0 covered at every site, the
    last row (of two or more) covered nowhere"""
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, size=(n_rows, n_cb), p=[0.4, 0.25, 0.1, 0.25])
    kind[:, 0] = np.where(kind[:, 0] == 0, 1, kind[:, 0])
    if n_rows >= 2:
        kind[-1, :] = 0
    dp = np.select([kind == 0, kind == 1, kind == 2], [0, rng.integers(1, 60, kind.shape), 400], rng.integers(5, 41, kind.shape)).astype(np.uint32)
    alt = np.select([kind <= 1, kind == 2], [0, 1], np.minimum(dp, rng.integers(3, 41, kind.shape))).astype(np.uint32)
    return dp, alt


def thresholds(counts):
    """a value v with both v and v + 1 among the counts (count == min is dropped, min + 1 kept), else the largest count - 1"""
    have = set(int(x) for x in counts)
    both = sorted(v for v in have if v + 1 in have)
    return both[len(both) // 2] if both else (max(have) - 1 if have else 0)


def write_matrices(engine, prefix, columns, fusions, n_mat):
    """<prefix>.{Dp,Alt,VAF,Binary}Matrix.tsv as cell_genotype_matrices writes them (integer form), from the device's tables; returns the four texts"""
    frows = cellclust.fusion_rows(fusions, columns, False)
    slots = {"Dp": engine.TABLE_CELL_DP, "Alt": engine.TABLE_CELL_ALT, "VAF": engine.TABLE_CELL_VAF, "Binary": engine.TABLE_CELL_BIN}
    for m in cellclust.MATRICES:
        n = engine.format_table(slots[m])
        body = engine.table_bytes(slots[m], n).decode() if n_mat else ""
        with open(prefix + "." + m + "Matrix.tsv", "w") as f:
            f.write("\t".join([""] + columns) + "\n" + body + "".join(line for _, line in frows[m]))
    return {m: open(prefix + "." + m + "Matrix.tsv").read() for m in cellclust.MATRICES}


@pytest.mark.parametrize("n_rows", [1, 70, 300])                       # 300: more rows than one workgroup of the column kernel takes (128)
@pytest.mark.parametrize("n_cb", [1, 40, 257, 300])                    # across the 256-column chunk of k_cell_matrix and the column kernel's block edge
def test_grids_against_numpy_and_the_twin(engine, tmp_path, n_rows, n_cb):
    dp, alt = make_grid(n_rows, n_cb, 1000 * n_rows + n_cb)
    engine.cellgeno_load_counts(dp, alt, np.zeros(n_rows, np.uint8))
    bin_ = engine.cellgeno_fetch()["bin"]
    assert set(np.unique(bin_).tolist()) <= {0, 1, 3} and (bin_[:, 0] != 3).sum() == (n_rows - 1 if n_rows >= 2 else n_rows)
    barcodes = ["BC%04d" % i for i in range(n_cb)]
    ghost = min(3, n_cb)                                               # a column no barcode stands behind (a barcode of the fusion file alone)
    columns = barcodes[:ghost] + ["BC%04dX" % (ghost - 1)] + barcodes[ghost:]
    col_src = list(range(ghost)) + [-1] + list(range(ghost, n_cb))
    fusions = [("GA--GB", c) for c in columns if c != columns[-1]] + [("HA--HB", columns[0]), ("HA--HB", columns[ghost])]
    labels = ["chr1:%d:A" % (10 + i) for i in range(n_rows)]
    bc_file = str(tmp_path / "barcodes.tsv")
    with open(bc_file, "w") as f:
        f.write("Index\tCell_type\tReannotated_cell_type\n" + "".join("%s\tCancer\t%s\n" % (b, "Non-Cancer" if i % 3 else "Cancer") for i, b in enumerate(["NOBODY"] + columns[::-1])))
    # all rows in order (the uncovered row makes every column float), then without that row and reversed (barcode 0 prints as integers)
    orders = [list(range(n_rows))] + ([list(range(n_rows - 1))[::-1]] if n_rows >= 2 else [])
    for k, mat_order in enumerate(orders):
        engine.cellgeno_set_text([""] * n_rows, [""] * n_rows, labels, barcodes, [""] * n_cb, [], mat_order, col_src, False)
        prefix = str(tmp_path / ("m%d" % k))
        before = write_matrices(engine, prefix, columns, fusions, len(mat_order))
        b = np.where(np.array(col_src) >= 0, bin_[mat_order][:, np.maximum(col_src, 0)], 3)
        ok = np.array(cellclust.bnpc_col_int_ok(columns, fusions, False), bool)
        assert ok.sum() == 2 or n_cb < 3
        c_edge = thresholds((b == 1).sum(1))
        p_edge = thresholds((b[(b == 1).sum(1) > c_edge] != 3).sum(0))
        cov_edge = (b[(b == 1).sum(1) > c_edge] != 3).sum(0)
        if n_rows >= 70 and n_cb >= 40:
            assert p_edge in cov_edge and p_edge + 1 in cov_edge                         # both sides of the column filter's threshold are in the grid
        # the edges of both filters, everything dropped, everything kept, and no row kept with every column kept (a header and the fusion rows)
        for c, p in ((c_edge, p_edge), (10 ** 6, 10 ** 6), (-1, -1), (10 ** 6, -1)):
            out = str(tmp_path / ("dev%d_%d_%d" % (k, c, p)))
            got = cellclust.format_bnpc_input(engine, columns, fusions, bc_file, out, c, p, float_cells=False)
            f = engine.cellgeno_filter_fetch()
            row_mut = (b == 1).sum(1); row_keep = row_mut > c
            cov_all = (b != 3).sum(0); cov_kept = (b[row_keep] != 3).sum(0)
            np.testing.assert_array_equal(f["row_mut"], row_mut); np.testing.assert_array_equal(f["row_keep"], row_keep)
            np.testing.assert_array_equal(f["col_cov_all"], cov_all); np.testing.assert_array_equal(f["col_cov_kept"], cov_kept)
            np.testing.assert_array_equal(f["col_keep"], cov_kept > p); np.testing.assert_array_equal(f["col_int"], ok & (cov_all == len(mat_order)))
            assert f["col_cov_all"][ghost] == 0 and got == (int(row_keep.sum()) + 2, int((cov_kept > p).sum()))
            if c < 0 and p < 0:                                                          # (c_edge itself is -1 where the one row carries no 1)
                assert row_keep.all() and f["col_keep"].all()
            if c == 10 ** 6:
                assert not row_keep.any() and f["col_keep"].all() == (p < 0) and f["col_keep"].any() == (p < 0)
            twin = str(tmp_path / ("twin%d_%d_%d" % (k, c, p)))
            cellclust.format_bnpc_input_host(prefix + ".BinaryMatrix.tsv", prefix + ".VAFMatrix.tsv", bc_file, twin, c, p)
            for o in cellclust.BNPC_OUTPUTS:
                assert open(out + "." + o + ".tsv").read() == open(twin + "." + o + ".tsv").read(), (o, k, c, p)
        if n_rows >= 70:
            assert c_edge in row_mut and c_edge + 1 in row_mut                           # both sides of the row filter's threshold are in the grid
        if k == 1 and n_cb >= 3:
            assert f["col_int"][0] == 1 and f["col_int"].sum() == 1                       # the covered barcode that carries both fusions
        # the four existing matrices print what they printed before the filter
        assert len(before) == 4 and before == write_matrices(engine, str(tmp_path / ("after%d" % k)), columns, fusions, len(mat_order))


# ---- 4. errors and invalidation -----------------------------------------------------------------------------------------------------
def test_order_of_calls_and_refusals(engine):
    dp = np.array([[4, 0, 9], [7, 7, 0]], np.uint32)
    engine.cellgeno_load_counts(dp, dp, np.zeros(2, np.uint8))
    with pytest.raises(RuntimeError, match="lsg_cellgeno_set_text first"):
        engine.cellgeno_filter(0, 0, [1, 1, 1])
    text = dict(heads=["h"] * 2, indexes=["i"] * 2, labels=["r0", "r1"], barcodes=["a", "b", "c"], celltypes=["t"] * 3, long_order=[0, 1], mat_order=[0, 1], col_src=[0, 1, 2], float_cells=False)
    engine.cellgeno_set_text(**text)
    with pytest.raises(RuntimeError, match="lsg_cellgeno_filter first"):
        engine.format_table(engine.TABLE_BNPC_BIN)
    dp_before = engine.table_bytes(engine.TABLE_CELL_DP, engine.format_table(engine.TABLE_CELL_DP))
    assert engine.cellgeno_filter(0, 0, [1, 1, 1]) == (2, 3)
    assert engine.table_bytes(engine.TABLE_BNPC_BIN, engine.format_table(engine.TABLE_BNPC_BIN)) == b"r0\t1\t\t1.0\nr1\t1\t1.0\t\n"
    assert engine.table_bytes(engine.TABLE_BNPC_VAF, engine.format_table(engine.TABLE_BNPC_VAF)) == b"r0\t1.0\t\t1.0\nr1\t1.0\t1.0\t\n"
    assert engine.table_bytes(engine.TABLE_CELL_DP, engine.format_table(engine.TABLE_CELL_DP)) == dp_before == b"r0\t4\t0\t9\nr1\t7\t7\t0\n"
    engine.cellgeno_set_text(**text)                                                      # a new text: the filter is gone with the old one
    with pytest.raises(RuntimeError, match="lsg_cellgeno_filter first"):
        engine.format_table(engine.TABLE_BNPC_VAF)
    with pytest.raises(RuntimeError, match="cellgeno_filter first"):
        engine.cellgeno_filter_fetch()


def test_loaded_cells_hold_no_counts(engine):
    bin_ = np.array([[1, 3, 0], [3, 3, 1]], np.uint8)
    vaf4 = np.array([[5000, -1, 0], [-1, -1, 3333]], np.int32)
    with pytest.raises(RuntimeError, match="is not 0, 1 or 3"):
        engine.cellgeno_load_cells(np.array([[1, 2, 0]], np.uint8), vaf4[:1])
    engine.cellgeno_load_cells(bin_, vaf4)
    got = engine.cellgeno_fetch()
    assert set(got) == {"vaf4", "status", "bin", "n_covered", "n_pass"}
    np.testing.assert_array_equal(got["bin"], bin_); np.testing.assert_array_equal(got["vaf4"], vaf4)
    np.testing.assert_array_equal(got["status"], [[4, 0, 1], [0, 0, 4]]); np.testing.assert_array_equal(got["n_covered"], [1, 0, 2])
    text = dict(heads=[""] * 2, indexes=[""] * 2, labels=["r0", "r1"], barcodes=["a", "b", "c"], celltypes=[""] * 3, long_order=[0, 1], mat_order=[1, 0], col_src=[2, 0], float_cells=False)
    for bad in (dict(mat_order=[2]), dict(col_src=[3]), dict(mat_order=[-1])):            # a bad order is refused, and leaves nothing to filter
        with pytest.raises(RuntimeError, match="is not a"):
            engine.cellgeno_set_text(**dict(text, **bad))
        with pytest.raises(RuntimeError, match="lsg_cellgeno_set_text first"):
            engine.cellgeno_filter(0, 0, [1, 1])
    engine.cellgeno_set_text(**text)
    for table in (engine.TABLE_CELL_LONG, engine.TABLE_CELL_DP, engine.TABLE_CELL_ALT):
        with pytest.raises(RuntimeError, match="loaded by lsg_cellgeno_load_cells"):
            engine.format_table(table)
    assert engine.cellgeno_filter(0, 0, [1, 1]) == (2, 2)
    assert engine.table_bytes(engine.TABLE_BNPC_VAF, engine.format_table(engine.TABLE_BNPC_VAF)) == b"r1\t0.3333\t\nr0\t0.0\t0.5\n"
    assert engine.table_bytes(engine.TABLE_BNPC_BIN, engine.format_table(engine.TABLE_BNPC_BIN)) == b"r1\t1\t\nr0\t0\t1.0\n"
    dp = np.ones((1, 3), np.uint32)
    engine.cellgeno_load_counts(dp, dp, np.zeros(1, np.uint8))                             # counts again: everything is back
    assert set(engine.cellgeno_fetch()) >= {"dp", "alt", "p4"}
