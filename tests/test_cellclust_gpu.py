"""GPU: the SingleCellGenotype step (csrc/cellgeno.hip, longsom_amd/cellclust.py) - the per-cell verdicts against scipy, the five files
against the reference-made fixtures tests/golden/cellclust.* byte for byte, the long table and the tallies against the host twin
(reanno.single_cell_genotype), the matrices against the long table pivoted here, and the error paths."""
import os

import numpy as np
import pytest

from longsom_amd import cellclust, cli, hostio, reanno
from longsom_amd._lib import CountParams
from tests.test_cellclust_cpu import golden
from tests.test_genotype_gpu import case, load, write_variants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
A2, B2 = 0.2474528917555431, 162.03696139428595          # the script's defaults (SingleCellGenotype.py:396-397)
OUTPUTS = ["SingleCellGenotype", "DpMatrix", "AltMatrix", "VAFMatrix", "BinaryMatrix"]
STATUS = ["NoCoverage", "NoAltReads", "LowVAFChrM", "BetaBin_problem", "PASS"]


# ---- 1. the classify kernel against scipy ---------------------------------------------------------------------------------------
def reference_cell(DP, ALT, chrom, chrm_conta, alpha2, beta2, pval):
    """SingleCellGenotype.py:188-218, line for line"""
    from scipy.stats import betabinom
    VAF = '.'
    BETABIN = '.'
    MUTATED = 'NoCoverage'
    if DP > 0:
        VAF = round(ALT / DP, 4)
        if ALT > 0:
            if chrm_conta == 'True' and str(chrom) == 'chrM':
                if VAF < 0.3:
                    MUTATED = 'LowVAFChrM'
                else:
                    MUTATED = 'PASS'
            else:
                BETABIN = round(betabinom.sf(ALT - 0.001, DP, alpha2, beta2), 4)
                if BETABIN < pval:
                    MUTATED = 'PASS'
                else:
                    MUTATED = 'BetaBin_problem'
        else:
            MUTATED = 'NoAltReads'
    if MUTATED == "PASS":
        BINARIZED = 1
    elif MUTATED == "NoCoverage":
        BINARIZED = 3
    else:
        BINARIZED = 0
    return VAF, BETABIN, MUTATED, BINARIZED


def test_classify_against_scipy(engine):
    """DP 1..64 with every ALT 1..DP and DP in {100, 257, 1000, 4096} with ALT 1..40 (2 240 cells), each on a chrM-flagged site and on a
    plain one, with DP = 0 and ALT = 0 cells, 130 barcodes to a site: vaf4, p4, status, the binary value and both tallies are equal."""
    n_cb = 130
    grid = [(dp, alt) for dp in range(1, 65) for alt in range(1, dp + 1)] + [(dp, alt) for dp in (100, 257, 1000, 4096) for alt in range(1, 41)]
    assert len(grid) == 2240
    cells = grid + [(0, 0), (1, 0), (3, 0), (64, 0), (4096, 0), (0, 0)]
    cells += [(0, 0)] * (-len(cells) % n_cb)
    half = len(cells) // n_cb
    dp = np.array([c[0] for c in cells] * 2, np.uint32).reshape(2 * half, n_cb)
    alt = np.array([c[1] for c in cells] * 2, np.uint32).reshape(2 * half, n_cb)
    is_chrm = np.array([0] * half + [1] * half, np.uint8)
    engine.cellgeno_load_counts(dp, alt, is_chrm, A2, B2, 0.01)
    got = engine.cellgeno_fetch()
    np.testing.assert_array_equal(got["dp"], dp); np.testing.assert_array_equal(got["alt"], alt)
    want = {k: np.zeros(dp.shape, np.int64) for k in ("vaf4", "p4", "status", "bin")}
    n_tail_pass = n_tail_problem = 0
    for s in range(2 * half):
        for cb in range(n_cb):
            vaf, bb, mutated, binarized = reference_cell(int(dp[s, cb]), int(alt[s, cb]), "chrM" if is_chrm[s] else "chr1", "True", A2, B2, 0.01)
            want["vaf4"][s, cb] = -1 if vaf == '.' else int(round(vaf * 10000))
            want["p4"][s, cb] = -1 if bb == '.' else int(round(bb * 10000))
            want["status"][s, cb] = STATUS.index(mutated)
            want["bin"][s, cb] = binarized
            if bb != '.':
                n_tail_pass += mutated == "PASS"; n_tail_problem += mutated == "BetaBin_problem"
    assert (n_tail_problem, n_tail_pass) == (135, 2105)                       # both sides of the threshold are in the grid
    assert {97, 100, 103} <= set(want["p4"].ravel().tolist())                 # ... and the rounded values next to it
    for k in want:
        bad = np.argwhere(got[k].astype(np.int64) != want[k])
        assert not len(bad), "%s differs at %d cells, first (DP, ALT, chrM) = %s: got %d, want %d" % (
            k, len(bad), (int(dp[tuple(bad[0])]), int(alt[tuple(bad[0])]), int(is_chrm[bad[0][0]])), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    assert set(want["status"].ravel().tolist()) == {0, 1, 2, 3, 4}
    np.testing.assert_array_equal(got["n_covered"], (dp > 0).sum(axis=0))
    np.testing.assert_array_equal(got["n_pass"], (want["status"] == 4).sum(axis=0))


# ---- 2. the five files against the reference's, through the CLI ----------------------------------------------------------------
@pytest.mark.parametrize("run,bam,extra", [("rand.All", "rand", ["--alt_flag", "All"]), ("rand.Alt", "rand", ["--alt_flag", "Alt"]),
                                           ("randsfx.All", "randsfx", ["--alt_flag", "All"]), ("rand.p002", "rand", ["--pvalue", "0.002"]),
                                           ("rand.fusions", "rand", [os.path.join(G, "cellclust.fusions.tsv")])])
def test_files_equal_the_reference(tmp_path, run, bam, extra):
    prefix = str(tmp_path / "s")
    cli.cell_genotype_matrices(["--bam", os.path.join(G, "pileup.%s.bam" % bam), "--infile", os.path.join(G, "cellclust.targets.tsv"), "--ref", os.path.join(G, "pileup.rand.fa"),
                                "--meta", os.path.join(G, "pileup.%s.barcodes.tsv" % bam), "--outfile", prefix, "--nprocs", "1", "--min_mq", "60",
                                "--tmp_dir", str(tmp_path / "tmp"), "--chrM_contaminant", "True", "--fusions"] + extra)
    for o in OUTPUTS:
        src = "rand.All" if (run == "rand.fusions" and o == "SingleCellGenotype") else run      # (the fusion run's long table is the base run's)
        want = golden(src, o)
        got = open(prefix + "." + o + ".tsv").read()
        assert got == want, "%s of run %s differs from the reference's" % (o, run)
    if run == "rand.p002":
        assert "\tBetaBin_problem\t0\t" in open(prefix + ".SingleCellGenotype.tsv").read()


# ---- 3. / 4. the host twin and the pivot ---------------------------------------------------------------------------------------
NAMES = ["chr7", "chrM"]
WINDOW = 300


@pytest.fixture(scope="module")
def sample_run(engine, tmp_path_factory):
    """(n_cb, max_depth, with fusions) -> the files of one device run on tests/test_genotype_gpu.py's case(11) shape, made once"""
    made = {}

    def run(n_cb, max_depth, fusions):
        key = (n_cb, max_depth, fusions)
        if key in made:
            return made[key]
        d = tmp_path_factory.mktemp("cellclust")
        rec, lens, celltype_of, keys, alt = case(11, n_cb=n_cb)
        celltype_of = np.where(celltype_of == 255, 1, celltype_of).astype(np.uint8)      # barcodes.tsv lists only typed cells
        load(engine, rec, lens, celltype_of)
        table = hostio.BarcodeTable(["BC%04d" % i for i in range(n_cb)], celltype_of, ["Cancer", "Non-Cancer"])
        vf = str(d / "v.tsv")
        write_variants(vf, NAMES, keys, alt)
        fus = None
        if fusions:
            fus = str(d / "fusions.tsv")
            with open(fus, "w") as f:
                f.write("#FusionName\tBC\n" + "".join("%s\t%s\n" % p for p in [("A1--B10", "BC0003"), ("A1--B2", "NOTACELL"), ("A1--B10", "BC0003"), ("A1--B10", "BC0000"), ("G--H", "BC%04d" % (n_cb - 1))]))
        stats = {}
        prefix = str(d / "dev")
        n = cellclust.cell_genotype_matrices(engine, vf, table, NAMES, prefix, fus, window=WINDOW, min_bq=30, min_mq=60, alpha2=A2, beta2=B2, pvalue=0.01,
                                             chrm_contaminant="True", max_depth=max_depth, stats=stats)
        made[key] = dict(dir=d, prefix=prefix, n=n, stats=stats, vf=vf, table=table, n_sites=len(keys), fusions=fus, case=(rec, lens, celltype_of))
        return made[key]
    return run


@pytest.mark.parametrize("n_cb,max_depth", [(40, 200000), (40, 25), (130, 200000)])
def test_long_table_and_tallies_equal_the_host_twin(engine, sample_run, n_cb, max_depth):
    """the device's long table with its last two columns cut is the file reanno.single_cell_genotype writes for the same engine and
    targets (a covered cell without alt reads prints VAF 0.0 in both), its tallies are the twin's stats; max_depth = 25 caps the hot windows"""
    r = sample_run(n_cb, max_depth, False)
    load(engine, *r["case"])                                                              # (another case may be resident by now)
    twin_path = str(r["dir"] / "twin.tsv")
    twin_stats = {}
    n = reanno.single_cell_genotype(engine, r["vf"], r["table"], NAMES, twin_path, window=WINDOW, min_bq=30, min_mq=60, alpha2=A2, beta2=B2, pvalue=0.01,
                                    chrm_contaminant="True", strict_cb=False, max_depth=max_depth, stats=twin_stats)
    assert n == r["n"] == r["n_sites"] * n_cb
    dev = open(r["prefix"] + ".SingleCellGenotype.tsv").read().split("\n")
    twin = open(twin_path).read().split("\n")
    assert dev[0] == "\t".join(cellclust.LONG_HEADER) and dev[-1] == "" and len(dev) == n + 2
    assert ["\t".join(l.split("\t")[:14]) for l in dev[:-1]] == twin[:-1]
    assert r["stats"] == twin_stats and sum(twin_stats["mutated"].values()) > 10
    text = "\n".join(dev)
    for s in ("PASS", "NoAltReads", "NoCoverage"):
        assert "\t%s\t" % s in text
    assert "\t0.0\t.\tNoAltReads\t0\t" in text
    if max_depth == 25:
        free = open(sample_run(n_cb, 200000, False)["prefix"] + ".SingleCellGenotype.tsv").read()
        assert text != free                                                         # the cap really dropped reads


@pytest.mark.parametrize("n_cb,fusions", [(40, False), (40, True), (130, True)])
def test_matrices_equal_the_pivoted_long_table(sample_run, n_cb, fusions):
    r = sample_run(n_cb, 200000, fusions)
    rows = [l.split("\t") for l in open(r["prefix"] + ".SingleCellGenotype.tsv").read().split("\n")[1:] if l]
    cell = {(x[15], x[7]): {"Dp": x[9], "Alt": x[10], "VAF": x[11], "Binary": x[14]} for x in rows}
    assert len(cell) == len(rows) == r["n_sites"] * n_cb
    pairs = set(cellclust.read_fusions(r["fusions"]))
    fusion_names = {f for f, _ in pairs}
    barcodes = r["table"].barcodes
    want_cols = sorted(set(barcodes) | {b for _, b in pairs})
    want_rows = [cellclust.matrix_label(i) for i in (lambda idx: [idx[k] for k in cellclust.matrix_row_order(idx)])(sorted({x[15] for x in rows}) + ["zzz:" + f for f in sorted(fusion_names)])]
    for m in cellclust.MATRICES:
        lines = open(r["prefix"] + "." + m + "Matrix.tsv").read().split("\n")
        assert lines[-1] == "" and lines[0].split("\t") == [""] + want_cols
        body = [l.split("\t") for l in lines[1:-1]]
        assert [b[0] for b in body] == want_rows and all(len(b) == 1 + len(want_cols) for b in body)
        for b in body:
            for cb, got in zip(want_cols, b[1:]):
                if b[0] in fusion_names:
                    want = ("1" if m == "VAF" else "1.0") if (b[0], cb) in pairs else ""
                elif cb not in barcodes:
                    want = ""
                else:
                    want = cell[(b[0], cb)][m] + (".0" if fusions and m != "VAF" else "")
                assert got == want, (m, b[0], cb, got, want)
    assert (len(want_cols) == n_cb + 1) == fusions


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_a_load_without_a_store_is_an_error(engine):
    rec, lens, celltype_of, keys, alt = case(12, n_reads=300)
    rng = np.random.default_rng(3)
    engine.set_contigs(lens)
    for t, n in enumerate(lens):
        engine.load_reference(t, rng.choice(np.frombuffer(b"ACGT", np.uint8), int(n)))
    engine.set_barcodes(celltype_of, 2)
    saved = engine.load_settings()
    engine.set_count_at_load(CountParams.longsom_defaults())
    engine.set_store_policy(engine.STORE_SKIP_WHEN_COUNTED)
    try:
        engine.load_reads(rec)
    finally:
        engine.restore_load_settings(saved)
    assert engine.layout_info()[0] >= 4                                                   # the load kept no store
    groups = [0, int((keys >> 32 == 0).sum()), len(keys)]                                 # one window per contig
    with pytest.raises(RuntimeError, match="lsg_cellgeno_count: the load kept no store"):
        engine.cellgeno_count(keys, alt, np.zeros(len(keys), np.uint8), groups)
    engine.load_reads(rec)                                                                # with a store again
    engine.cellgeno_count(keys, alt, np.zeros(len(keys), np.uint8), groups)
    assert engine.cellgeno_fetch()["dp"].shape == (len(keys), len(celltype_of))


def test_bad_orders_are_refused_not_followed(engine):
    dp = np.ones((3, 5), np.uint32)
    engine.cellgeno_load_counts(dp, dp, np.zeros(3, np.uint8))
    ok = dict(heads=["h"] * 3, indexes=["i"] * 3, labels=["l"] * 3, barcodes=["b"] * 5, celltypes=["c"] * 5, long_order=[0, 1, 2], mat_order=[2, 0, 1], col_src=[4, -1, 0], float_cells=False)
    engine.cellgeno_set_text(**ok)
    assert engine.format_table(engine.TABLE_CELL_DP) == len("l\t1\t\t1\n") * 3
    for k, v in (("long_order", [0, 3]), ("mat_order", [-1]), ("col_src", [5]), ("col_src", [-2])):
        with pytest.raises(RuntimeError, match="is not a"):
            engine.cellgeno_set_text(**dict(ok, **{k: v}))
    with pytest.raises(RuntimeError, match="lsg_cellgeno_set_text first"):
        engine.format_table(engine.TABLE_CELL_LONG)                                       # a refused text leaves none behind


def test_no_targets(engine, tmp_path, capsys):
    """no target line: the reference prints 'No temporary files found' and dies reading the table it never wrote; here the same line,
    then an error that says so - no file"""
    empty = tmp_path / "none.tsv"
    empty.write_text("##nothing\n#CHROM\tStart\n")
    with pytest.raises(SystemExit) as e:
        cli.cell_genotype_matrices(["--bam", os.path.join(G, "pileup.rand.bam"), "--infile", str(empty), "--ref", "unused.fa", "--meta", os.path.join(G, "pileup.rand.barcodes.tsv"),
                                    "--outfile", str(tmp_path / "s"), "--tmp_dir", str(tmp_path / "tmp"), "--fusions"])
    assert isinstance(e.value.code, str) and "names no target site" in e.value.code      # (a message as the exit code: status 1)
    assert "No temporary files found" in capsys.readouterr().out
    assert not os.path.exists(str(tmp_path / "s") + ".SingleCellGenotype.tsv")
