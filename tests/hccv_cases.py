"""Step-2 tables for the tests of the HCCV row code (test_hccv_cpu.py: the host twin; test_hccv_gpu.py: the device): tables made of the
golden's rows as test_reanno_cpu.py makes them, and hand-made rows around every comparison the filter makes.  The expected output is
always reanno.hccv_filter's on the same file (which the reference-generated goldens pin)."""
import filecmp
import os

import numpy as np

from longsom_amd import reanno

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP2 = os.path.join(G, "sample.calling.step2.tsv")
GOLDEN_ARGS = [("sample", (50, 0.2, 0.25, 10000)), ("sample.loose", (5, 0.05, 0.1, 400))]
COLS = ("#CHROM Start End REF ALT FILTER Cell_types Up_context Down_context N_ALT Dp Nc Bc Cc VAF MCF BCp CCp Cell_types_min_BC Cell_types_min_CC Rest_BC Rest_CC "
        "Fisher_p Cell_type_Filter INFO Cancer Non-Cancer").split()
HEAD = ["##fileformat=test", "##contig=<ID=chr1>", "\t".join(COLS)]


def golden_parts():
    lines = open(STEP2).read().split("\n")
    return [l for l in lines if l.startswith("#")], [l.split("\t") for l in lines if l and not l.startswith("#")]


def seeded_tables(seed: int):
    """[(name, args, text)]: the golden's rows replicated with shifted positions, some moved to chrM (they interleave), cut to one kind of
    row - the construction of test_reanno_cpu.py::test_hccv_filter_column_form_equals_the_row_form"""
    head, rows = golden_parts()
    rng = np.random.default_rng(seed)
    cases = [("all", None), ("single", lambda r: "," not in r[6]), ("cancer_only", lambda r: r[6] == "Cancer"), ("multi", lambda r: "Multi" in r[5]),
             ("nomulti", lambda r: "Multi" not in r[5] and "|" not in r[4]), ("noncancer", lambda r: r[6] == "Non-Cancer")]
    args = [(50, 0.2, 0.25, 10000), (5, 0.05, 0.1, 400), (20, 0.1, 0.4, 10000)][seed % 3]
    out = []
    for name, pick in cases:
        lines = list(head)
        for k in range(int(rng.integers(1, 4))):
            for r in (rows if pick is None else [r for r in rows if pick(r)]):
                if rng.random() < 0.15:
                    continue
                r2 = list(r)
                shift = k * 1_000_000 + int(rng.integers(0, 3)) * 7
                r2[1] = str(int(r[1]) + shift); r2[2] = str(int(r[2]) + shift)
                if rng.random() < 0.05:
                    r2[0] = "chrM"
                lines.append("\t".join(r2))
        out.append(("%s.s%d" % (name, seed), args, "\n".join(lines) + "\n"))
    return out


def info(dp, nc, cc="0:0:0:0:0:0", bc="0:0:0:0:0:0"):
    return "%d|%d|%s|%s|0:0:0:0:0:0|0:0:0:0:0:0|0:0:0:0:0:0" % (dp, nc, cc, bc)


def row(pos, **kw):
    """a row that passes every test at (50, 0.2, 0.25): two cell types, FILTER PASS, 100 reads in both columns; kw replaces fields by name"""
    f = {"#CHROM": "chr1", "Start": str(pos), "End": str(pos), "REF": "A", "ALT": "G,G", "FILTER": "PASS", "Cell_types": "Cancer,Non-Cancer", "Up_context": "ACGTA",
         "Down_context": "TTGCA", "N_ALT": "1", "Dp": "100,100", "Nc": "40,40", "Bc": "50,0", "Cc": "20,0", "VAF": "0.5,0.0", "MCF": "0.5,0.0", "BCp": "0.0,1.0",
         "CCp": "0.0,1.0", "Cell_types_min_BC": "2", "Cell_types_min_CC": "2", "Rest_BC": "0;1;1", "Rest_CC": "0;1;1", "Fisher_p": ".", "Cell_type_Filter": "PASS,Non-Significant",
         "INFO": "DP|NC|CC|BC|BQ|BCf|BCr", "Cancer": info(100, 40, "0:0:0:20:0:0", "50:0:0:50:0:0"), "Non-Cancer": info(100, 40, "40:0:0:0:0:0", "100:0:0:0:0:0")}
    for k, v in kw.items():
        f[{"CHROM": "#CHROM", "NonCancer": "Non-Cancer"}.get(k, k)] = v
    return "\t".join(f[c] for c in COLS)


def fillers(n=3, at=1_000_000):
    """rows that reach the final table whatever else the table holds (far from every other row)"""
    return [row(at + 50_000 * i) for i in range(n)]


def table(rows, newline_at_end=True):
    return "\n".join(HEAD + list(rows)) + ("\n" if newline_at_end else "")


def multi(pos, cancer_bc, normal_bc="0:0:0:0:0:0", dp=100, **kw):
    """a multi-allelic row of two cell types whose columns hold these A:C:T:G:I:D read counts"""
    kw.setdefault("FILTER", "Multi-allelic")
    kw.setdefault("ALT", "C|T,C")
    return row(pos, Cancer=info(dp, 40, "0:7:9:0:0:0", cancer_bc), NonCancer=info(100, 40, "0:1:2:0:0:0", normal_bc), **kw)


def hand_made():
    """[(name, args, text)] - every table also holds the fillers, so that no frame of the reference's runs empty"""
    A = (50, 0.2, 0.25, 10000)
    t = []
    depth = [row(1000, Cancer=info(50, 40)), row(2000, Cancer=info(49, 40)), row(3000, NonCancer=info(50, 40)), row(4000, NonCancer=info(49, 40)),
             row(5000, Cancer=info(50, 40), NonCancer=info(50, 40))]
    t.append(("depth_at_min_dp", A, table(depth + fillers())))
    t.append(("min_dp_49p5", (49.5, 0.2, 0.25, 10000), table(depth + fillers())))
    t.append(("runner_up", A, table([multi(1000, "0:1:20:0:0:0"), multi(2000, "0:1:21:0:0:0"), multi(3000, "0:21:1:0:0:0", "0:3:0:0:0:0"),
                                    multi(4000, "0:0:30:0:0:0", Cell_types="Non-Cancer,Cancer"), multi(5000, "0:30:30:0:0:0"),
                                    multi(6000, "0:0:30:0:0:0", FILTER="PASS"), multi(7000, "0:0:3:0:0:0", "0:0:1:0:0:0", FILTER="Multi-allelic,PoN_SR"),
                                    row(8000, Cell_types="Cancer", ALT="C|T", FILTER="Cell_type_noise,Multi-allelic", Dp="100", Nc="40", Bc="7|9", Cc="3|4", VAF="0.07|0.09",
                                        MCF="0.075|0.1", Cancer=info(100, 40, "0:0:33:0:0:0", "0:1:61:0:0:0")),
                                    row(9000, Cell_types="Tcell", ALT="C|T", FILTER="Multi-allelic", Dp="100", Nc="40", Bc="7|9", Cc="3|4", VAF="0.07|0.09", MCF="0.075|0.1")] + fillers())))
    vafs = ["0.05,0.0", "0.0499,0.0", "0.5,0.1", "0.5,0.1001", "0.5,0.2", "0.5,0.2001", "0.55,0.15", "0.56,0.16", "0.57,0.17", "0.58,0.18", "0.59,0.19", "0.6,0.2",
            "0.5499,0.15", "0.5501,0.15", "0.7,0.3", "1.0,0.0", "0.0,0.0", "1.0,1.0", "0.3,0.2", "0.45,0.15", "0.4,0.1001"]
    for name, args in (("verdict", A), ("verdict_loose", (5, 0.05, 0.1, 400)), ("verdict_0p15", (50, 0.15, 0.3, 10000))):
        rows = [row(1000 + 20_000 * i, VAF=v) for i, v in enumerate(vafs)]
        rows += [row(600_000 + 20_000 * i, MCF=m) for i, m in enumerate(["0.25,0.0", "0.2499,0.0", "0.35,0.1", "0.3,0.05", "0.4,0.1", "1.0,0.7", "0.3,0.0"])]
        rows += [row(800_000 + 20_000 * i, Cell_types="Cancer", ALT="G", Dp="100", Nc="40", Bc="50", Cc="20", VAF=v, MCF=m)
                 for i, (v, m) in enumerate([("0.2", "0.25"), ("0.1999", "0.25"), ("0.2", "0.2499"), ("1.0", "1.0"), ("0.0", "0.0"), ("0.05", "0.1"), ("0.15", "0.3")])]
        rows += [row(990_000, Cell_types="Tcell", ALT="G", Dp="100", Nc="40", Bc="50", Cc="20", VAF="0.5", MCF="0.5"), row(995_000, Cell_types="Non-Cancer,Cancer", VAF="0.0,0.5", MCF="0.0,0.5")]
        t.append((name, args, table(rows + fillers(at=2_000_000))))
    t.append(("filter_text", A, table([multi(1500, "0:0:30:0:0:0"), row(2000, CHROM="chrM", FILTER="PoN_LR"), row(3000, FILTER="PoN_LR"), row(4000, CHROM="chrM", FILTER="PoN_SR"),
                                      row(5000, CHROM="chrM", FILTER="Min_cell_types"), row(30_000, FILTER="Min_cell_types"), row(60_000, FILTER="Cell_type_noise,LC_Upstream"),
                                      row(90_000, FILTER="RNA_editing_db"), row(120_000, FILTER="gnomAD"), row(150_000, FILTER="Noisy_site"), row(180_000, FILTER="Clust_dist5"),
                                      row(210_000, CHROM="chrM"), row(240_000, Up_context="NA", Down_context="null"), row(270_000, NonCancer=""),
                                      row(300_000, Cell_types="Cancer", ALT="G", Dp="100", Nc="40", Bc="50", Cc="20", VAF="0.5", MCF="0.5", NonCancer=""),
                                      row(330_000, Cancer=""), row(360_000, Fisher_p="nan")] + fillers())))
    near = [row(99), row(100), row(10_500), row(200_000, CHROM="chrM"), row(200_001, CHROM="chrM"), row(99, CHROM="chr2"), row(150, CHROM="chr2")]
    t.append(("cluster_text_order", A, table(near + fillers())))
    t.append(("cluster_wider", (50, 0.2, 0.25, 10_450), table(near + fillers())))
    t.append(("no_last_newline", A, table(fillers() + [row(5000)], newline_at_end=False)))
    t.append(("no_pass_row", A, table([row(1000 + 20_000 * i, VAF="0.04,0.0") for i in range(4)] + [row(500_000, FILTER="PoN_SR,gnomAD")])))
    t.append(("all_clustered", A, table([row(1000 + 100 * i) for i in range(4)])))
    for n in (0, 1, 255, 256, 257):
        t.append(("rows_%d" % n, A, table([row(1000 + 20_000 * i, VAF="0.04,0.0" if i % 3 == 1 else "0.5,0.0") for i in range(n)])))
    return t


def undecided():
    """[(name, args, text, ordinal or None, reason or None)]: tables the row code must hand to reanno.hccv_filter whole"""
    A = (50, 0.2, 0.25, 10000)
    return [("blank_int_cell", A, table(fillers() + [row(5000, Cell_types="Non-Cancer", N_ALT="")]), None, None),
            ("max_zero", A, table(fillers() + [row(5000), multi(6000, "0:0:0:0:0:0")]), 4, 6),                    # (the reference divides by zero: so does the fallback)
            ("max_zero_shallow", A, table(fillers() + [row(5000), multi(6000, "0:0:0:0:0:0", dp=10)]), 4, 6),     # (hccv_filter drops the row by its depth first)
            ("short_row", A, table(fillers(2) + ["\t".join(row(5000).split("\t")[:-1])] + fillers(1, at=3_000_000)), 2, 1)]


def run(fn, path, prefix, args, **kw):
    """fn's output path, or the type of what it raised"""
    try:
        return fn(path, prefix, *args, **kw)
    except Exception as e:                              # noqa: BLE001 - (a table with no row left: the reference's frame operations raise)
        return type(e)


def same_files(a, b):
    return all(filecmp.cmp(a + s, b + s, shallow=False) for s in ("", "2", "3"))


def check_against_reference(tmp_path, name, args, text, fn, **kw):
    """fn(table, prefix, *args) leaves the files reanno.hccv_filter leaves, or raises what it raises; returns fn's output (or the exception type)"""
    path = tmp_path / (name + ".tsv")
    path.write_text(text)
    want = run(reanno.hccv_filter, str(path), str(tmp_path / (name + ".want")), args)
    got = run(fn, str(path), str(tmp_path / (name + ".got")), args, **kw)
    if isinstance(want, type) or isinstance(got, type):
        assert got == want, (name, got, want)
        return got
    for s in ("", "2", "3"):
        assert open(got + s).read() == open(want + s).read(), (name, ".HCCV.tsv" + s)
    return got


def shapes():
    """[(name, args, text)]: row shapes the device's kernels care about - rows far shorter than the 256-byte piece of the newline pass
    (several row starts in one piece) and more of them than one block of lanes, a row of many pieces, a text that ends on a piece's edge with
    and without its last newline, fewer rows than one wave"""
    A = (50, 0.2, 0.25, 10000)
    need = [c for c in COLS if c in reanno.HCCV_COLUMNS]

    def short(i):
        f = dict(zip(COLS, row(1000 + 20_000 * i, VAF="0.04,0.0" if i % 5 == 1 else "0.5,0.0", CHROM="chrM" if i % 7 == 3 else "chr1", FILTER="PoN_SR" if i % 11 == 5 else "PASS",
                               Cancer=info(100 if i % 3 else 20, 40),
                               NonCancer=info(100, 40)).split("\t")))
        return "\t".join(f[c] for c in need)
    t = [("short_rows", A, "\n".join(["##x", "\t".join(need)] + [short(i) for i in range(700)]) + "\n")]
    t.append(("long_row", A, table(fillers(2) + [row(5000, Up_context="ACGT" * 1300)] + fillers(40, at=3_000_000))))
    for newline in (True, False):
        rows = fillers(5)
        n = len("\n".join(rows)) + 1 + len(row(9000)) + (1 if newline else 0)
        pad = (-n) % 256
        rows.append(row(9000, Up_context="ACGTA" + "C" * pad))
        text = table(rows, newline_at_end=newline)
        assert (len(text) - len("\n".join(HEAD)) - 1) % 256 == 0
        t.append(("piece_edge_%s" % ("newline" if newline else "bare"), A, text))
    return t
