"""Step-2 tables for the tests of step 3's row code (test_step3_core_cpu.py: the host twin; test_step3_gpu.py: the device): the goldens, the
replicated tables of test_calling_cpu.py, and hand-made rows (hccv_cases.py's builders) around every tag, every comparison and every reason
the row code hands a table back for.  The expected output is always calling.step3's over the same text (which the reference-generated
goldens pin)."""
import os

from longsom_amd import calling

from . import hccv_cases as hc

G = hc.G
ARGS = (0.05, 0.3, 3, 2, 10000)                      # deltaVAF, deltaMCF, min_ac_reads, min_ac_cells, clust_dist: the goldens' arguments
GOLDENS = [("sample", ARGS), ("sample.dist150", (0.05, 0.3, 3, 2, 150))]
COLS, row, info, table, fillers, multi = hc.COLS, hc.row, hc.info, hc.table, hc.fillers, hc.multi


def rd(name):
    return open(os.path.join(G, name)).read()


def replicated_tables():
    """(the 30 k-row table, the one-cell-type table) of test_calling_cpu.py::_step3_tables"""
    lines = rd("sample.calling.step2.tsv").split("\n")
    comments = [l for l in lines if l.startswith("#")]
    body = [l for l in lines if l and not l.startswith("#")]
    big, k = [], 0
    while len(big) < 30000:
        for l in body:
            f = l.split("\t"); f[1] = str(int(f[1]) + 1000 * k); f[2] = f[1]; big.append("\t".join(f))
        k += 1
    cols = [l for l in comments if l.startswith("#CHROM")][0].split("\t")
    i_nc = cols.index("Non-Cancer")
    one = [l for l in comments if not l.startswith("#CHROM")] + ["\t".join(c for i, c in enumerate(cols) if i != i_nc)]
    for l in big:
        f = l.split("\t")
        if f[cols.index("Cell_types")] == "Cancer":
            one.append("\t".join(x for i, x in enumerate(f) if i != i_nc))
    return "\n".join(comments + big) + "\n", "\n".join(one) + "\n"


def golden_live_rows():
    """(comment lines, header columns, the golden's rows that reach step 3's row functions with FILTER PASS) - the table of
    test_calling_cpu.py::test_step3_native_hands_back_what_pandas_dtypes_could_change"""
    lines = rd("sample.calling.step2.tsv").split("\n")
    comments = [l for l in lines if l.startswith("#")]
    cols = [l for l in comments if l.startswith("#CHROM")][0].split("\t")
    i_ct, i_f = cols.index("Cell_types"), cols.index("FILTER")
    body = [l for l in lines if l and not l.startswith("#")]
    return comments, cols, [l for l in body if l.split("\t")[i_ct] != "Non-Cancer" and "PASS" in l.split("\t")[i_f]]


def one_type(pos, **kw):
    """a row of a single cell type, Cancer, that is PASS at ARGS"""
    d = dict(Cell_types="Cancer", ALT="G", Dp="100", Nc="40", Bc="50", Cc="20", VAF="0.5", MCF="0.5", Cell_type_Filter="PASS", NonCancer="")
    d.update(kw)
    return row(pos, **d)


def hand_made():
    """[(name, args, text)]"""
    t = []
    swapped = dict(Cell_types="Non-Cancer,Cancer", Dp="80,100", Nc="30,40")
    # MultiAllelic_filtering: kept and tagged / resolved, both orders of Cell_types (the pairs print Non-Cancer, Cancer), a FILTER that names
    # Multi-allelic stays with two cell types and is stripped with one
    t.append(("multi_two_types", ARGS, table([
        multi(1000, "0:1:30:0:0:0", "0:0:2:0:0:0"), multi(31_000, "0:20:30:0:0:0", "0:3:1:0:0:0"), multi(61_000, "0:1:30:0:0:0", "0:0:2:0:0:0", **swapped),
        multi(91_000, "0:20:30:0:0:0", "0:3:1:0:0:0", **swapped), multi(121_000, "0:0:30:0:0:0", FILTER="PASS"), multi(151_000, "0:0:30:0:0:0", FILTER="Multi-allelic,Clust5"),
        multi(181_000, "0:30:30:0:0:0"), multi(211_000, "0:1:2:0:0:0"), multi(241_000, "0:0:30:0:0:0", REF="C"),
        multi(271_000, "0:0:30:0:0:0", Cell_types="Non-Cancer,Cancer", Cell_type_Filter="Non-Significant,PASS")] + fillers())))
    t.append(("multi_one_type", ARGS, table([
        one_type(1000, ALT="C|T", FILTER="Multi-allelic", Bc="7|9", Cc="3|4", VAF="0.07|0.09", MCF="0.075|0.1", Cancer=info(100, 40, "0:0:33:0:0:0", "0:1:61:0:0:0")),
        one_type(31_000, ALT="C|T", FILTER="Clust5,Multi-allelic", Bc="7|9", Cc="3|4", VAF="0.07|0.09", MCF="0.075|0.1", Cancer=info(100, 40, "0:5:33:0:0:0", "0:31:61:0:0:0")),
        one_type(61_000, ALT="C|T", FILTER="Multi-allelic,Clust5", Cell_type_Filter="Low-Significance", Cancer=info(100, 40, "0:5:1:0:0:0", "0:2:1:0:0:0")),
        one_type(91_000), one_type(121_000, Cell_type_Filter="Non-Significant")] + fillers())))
    # chrM_filtering: the depth at 99 / 100 in either column, the differences at their thresholds (0.35 - 0.3 < 0.05 and 0.7 - 0.4 < 0.3 in
    # binary), both orders of Cell_types, one cell type at 0.05, a resolved multi-allelic row, the FILTER patterns of chrM rows
    m = dict(CHROM="chrM")
    two = [row(1000 + 100 * i, Dp=d, **m) for i, d in enumerate(["99,100", "100,99", "100,100", "99,99"])]
    two += [row(5000 + 100 * i, VAF=v, **m) for i, v in enumerate(["0.05,0.0", "0.0499,0.0", "0.35,0.3", "0.36,0.3", "0.3,0.35", "1.0,0.0"])]
    two += [row(7000 + 100 * i, MCF=v, **m) for i, v in enumerate(["0.3,0.0", "0.2999,0.0", "0.4,0.1", "0.5,0.2", "0.7,0.4", "0.9,0.6", "0.0,0.5"])]
    two += [row(9000 + 100 * i, Cell_types="Non-Cancer,Cancer", Dp=d, VAF=v, MCF="0.0,0.5", **m) for i, (d, v) in enumerate([("100,100", "0.0,0.5"), ("99,100", "0.0,0.5"), ("100,100", "0.5,0.0")])]
    two += [multi(11_000, "0:1:30:0:0:0", "0:0:2:0:0:0", **m), multi(11_100, "0:1:30:0:0:0", "0:0:29:0:0:0", **m), multi(11_200, "0:1:30:0:0:0", "0:0:2:0:0:0", CHROM="chrM", **swapped),
            multi(11_300, "0:20:30:0:0:0", "0:0:2:0:0:0", Dp="99,100", **m)]
    two += [row(13_000 + 100 * i, FILTER=f, **m) for i, f in enumerate(["PoN_SR", "PoN_LR", "Min_cell_types", "gnomAD", "LC_Upstream", "RNA_editing_db", "Cell_type_noise", "Noisy_site"])]
    one = [one_type(15_000 + 100 * i, Dp=d, VAF=v, MCF=mc, **m) for i, (d, v, mc) in enumerate([("99", "0.5", "0.5"), ("100", "0.5", "0.5"), ("100", "0.05", "0.05"), ("100", "0.0499", "0.5"),
                                                                                                ("100", "0.05", "0.0499"), ("99", "0.01", "0.01")])]
    t.append(("chrm", ARGS, table(fillers(2) + two + one + fillers(2, at=3_000_000))))
    t.append(("chrm_other_deltas", (0.1, 0.25, 3, 2, 10000), table(fillers(2) + two + one)))
    # BC_CC_filtering and BetaBino_filtering: NoCov, the alt's reads and cells at min_ac, every pair with the two significance tags
    low = [("0:0:0:2:0:0", "0:0:0:3:0:0"), ("0:0:0:1:0:0", "0:0:0:3:0:0"), ("0:0:0:2:0:0", "0:0:0:2:0:0"), ("0:0:0:0:0:0", "0:0:0:0:0:0"), ("0:0:0:9:0:0", "0:0:0:2:0:0")]
    rows = [row(1000 + 30_000 * i, Cancer=info(100, 40, cc, bc)) for i, (cc, bc) in enumerate(low)]
    ctf = ["PASS,Non-Significant", "Non-Significant,PASS", "Low-Significance,Non-Significant", "PASS,PASS", "PASS,Low-Significance", "Non-Significant,Non-Significant", "x,y"]
    rows += [row(200_000 + 30_000 * i, Cell_type_Filter=f) for i, f in enumerate(ctf)]
    rows += [row(500_000 + 30_000 * i, Cell_types="Non-Cancer,Cancer", Cell_type_Filter=f) for i, f in enumerate(ctf)]
    rows += [row(800_000 + 30_000 * i, Cancer="", Cell_type_Filter=f) for i, f in enumerate(ctf[:4])]
    rows += [row(2_000_000 + 30_000 * i, Cancer=info(100, 40, "0:0:0:1:0:0", "0:0:0:9:0:0"), Cell_type_Filter=f) for i, f in enumerate(ctf[:4])]
    rows += [one_type(2_500_000 + 30_000 * i, Cell_type_Filter=f, Cancer=c) for i, (f, c) in enumerate([("Non-Significant", ""), ("Low-Significance", info(100, 40, "0:0:0:1:0:0", "0:0:0:9:0:0")),
                                                                                                       ("PASS", ""), ("", info(100, 40, "0:0:0:9:0:0", "0:0:0:9:0:0"))])]
    rows += [multi(3_000_000, "0:1:2:0:0:0", Cell_type_Filter="Non-Significant,PASS"), multi(3_030_000, "0:1:2:0:0:0", Cell_type_Filter="PASS,PASS")]
    t.append(("counts_and_significance", ARGS, table(rows)))
    t.append(("min_ac_5_4", (0.05, 0.3, 5, 4, 10000), table([row(1000 + 30_000 * i, Cancer=info(100, 40, "0:0:0:%d:0:0" % c, "0:0:0:%d:0:0" % b))
                                                            for i, (b, c) in enumerate([(5, 4), (4, 4), (5, 3), (4, 3), (50, 20)])])))
    # the drops: Cell_types, the FILTER patterns of both kinds of row, missing cells that print as nothing
    t.append(("drops", ARGS, table([row(1000, Cell_types="Non-Cancer")] + [row(30_000 * (i + 1), FILTER=f) for i, f in enumerate(
        ["Min_cell_types", "Noisy_site", "LC_Upstream", "LC_Downstream", "RNA_editing_db", "PoN_SR", "PoN_LR", "Cell_type_noise", "gnomAD", "Clust_dist5", "Multi-allelic,gnomAD"])] +
        [row(600_000, Up_context="NA", Down_context="null"), row(630_000, NonCancer=""), row(660_000, Fisher_p="nan"), row(690_000, CHROM="chrM", Cell_types="Non-Cancer")] + fillers())))
    # the cluster test: neighbours in STRING order.  Among 9999, 10001, 100000 and the fillers' 1000000, 1050000, 1100000 on chr1 the
    # string order is 100000, 1000000, 10001, 1050000, 1100000, 9999: at clust_dist 10 no adjacent pair is closer, while in numeric
    # order 9999 and 10001 are neighbours 2 apart.  (The three positions alone have the same adjacent pairs in both orders.)  At 60000 the
    # string order pairs 1050000 with 1100000 only.
    near = [row(9999), row(10_001), row(100_000)]
    for clust in (10, 60_000, 1_000_000, 0):
        t.append(("cluster_string_order_%d" % clust, (0.05, 0.3, 3, 2, clust), table(near + fillers())))
    t.append(("cluster_contigs", ARGS, table([row(99), row(100), row(10_500), row(200_000, CHROM="chrM"), row(200_001, CHROM="chrM"), row(99, CHROM="chr2"), row(150, CHROM="chr2"),
                                              row(20_600, Cancer=""), row(20_700)] + fillers())))
    # two kept rows with one INDEX, of which one is PASS: the set holds INDEX texts, and both rows are tagged
    t.append(("same_index", ARGS, table([row(5000), row(5000, Cancer=info(100, 40, "0:0:0:1:0:0", "0:0:0:9:0:0")), row(5100), row(400_000), row(400_000, Cancer="")] + fillers())))
    t.append(("all_clustered", ARGS, table([row(1000 + 100 * i) for i in range(4)])))
    return t


def undecided():
    """[(name, args, text, why or None, ordinal or None, reason or None)]: tables the row code hands to calling.step3 whole.  The first eight are
    the list of test_step3_native_hands_back_what_pandas_dtypes_could_change; then one per reason."""
    comments, cols, live = golden_live_rows()

    def golden(name, value):
        rows = list(live)
        f = rows[1].split("\t"); f[cols.index(name)] = value; rows[1] = "\t".join(f)
        return "\n".join(comments + rows) + "\n"
    kinds = "column kinds"
    t = [("int_blank", ARGS, golden("N_ALT", ""), kinds, None, None), ("int_leading_zero", ARGS, golden("N_ALT", "01"), kinds, None, None),
         ("int_beside_float", ARGS, golden("N_ALT", "1.50"), kinds, None, None), ("int_exponent", ARGS, golden("N_ALT", "1e3"), kinds, None, None),
         ("hash", ARGS, golden("Up_context", "AC#GT"), None, 1, 3), ("quote", ARGS, golden("Up_context", '"ACGT'), None, 1, 3),
         ("int_nan", ARGS, golden("Cell_types_min_BC", "nan"), kinds, None, None), ("alt_n", ARGS, golden("ALT", "N"), None, 1, 10)]
    f3 = fillers(3)
    one_multi = dict(ALT="C|T", Bc="7|9", Cc="3|4", VAF="0.07|0.09", MCF="0.075|0.1", Cancer=info(100, 40, "0:0:33:0:0:0", "0:1:61:0:0:0"))
    long_chrom = "chr" + "x" * 70
    t += [("short_row", ARGS, table(f3[:2] + ["\t".join(row(5000).split("\t")[:-1])] + f3[2:]), None, 2, 1),
          ("long_row", ARGS, table(f3 + [row(5000) + "\tx"]), None, 3, 2),
          ("empty_line", ARGS, table(f3[:1] + [""] + f3[1:]), None, 1, 3),
          ("carriage_return", ARGS, table(f3 + [row(5000, Up_context="AC\rGT")]), None, 3, 3),
          ("missing_filter", ARGS, table(f3 + [row(5000, FILTER="")]), None, 3, 4),
          ("missing_alt", ARGS, table(f3 + [row(5000, ALT="NA")]), None, 3, 4),
          ("multi_without_the_other_column", ARGS, table(f3 + [row(5000, ALT="C|T,C", NonCancer="")]), None, 3, 4),
          ("chrm_depth_not_a_number", ARGS, table(f3 + [row(5000, CHROM="chrM", Dp="1e2,100")]), None, 3, 5),
          ("chrm_vaf_not_a_number", ARGS, table(f3 + [row(5000, CHROM="chrM", VAF="0.5,x")]), None, 3, 5),
          ("zero_divisor", ARGS, table(f3 + [multi(5000, "0:0:30:0:0:0", Dp="0,100")]), None, 3, 5),
          ("count_not_a_number", ARGS, table(f3 + [row(5000, Cancer=info(100, 40, "0:0:0:20:0:0", "50:0:0:x:0:0"))]), None, 3, 5),
          ("max_zero", ARGS, table(f3 + [multi(5000, "0:0:0:0:0:0")]), None, 3, 6),
          ("one_significance_for_two_types", ARGS, table(f3 + [row(5000, Cell_type_Filter="PASS")]), None, 3, 7),
          ("filter_too_long", ARGS, table(f3 + [one_type(5000, FILTER="Multi-allelic," + "Clust5," * 50 + "x", **one_multi)]), None, 3, 8),
          ("colon_in_chrom", ARGS, table(f3 + [row(5000, CHROM="chr:1")]), None, 3, 9),
          ("alt_not_a_base", ARGS, table(f3 + [row(5000, ALT="-,-")]), None, 3, 10),
          ("index_too_long", ARGS, table(f3 + [row(5000, CHROM=long_chrom), row(5100, CHROM=long_chrom)]), None, 3, 11),
          ("position_not_a_number", ARGS, table(f3 + [row(5000, CHROM="chr2", Start="5x3"), row(5100, CHROM="chr2")]), None, 3, 12),
          ("columns_elsewhere", ARGS, "\n".join(["##x", "\t".join(COLS[1:] + COLS[:1])] + ["\t".join(r.split("\t")[1:] + r.split("\t")[:1]) for r in f3]) + "\n", "columns", None, None),
          ("column_named_twice", ARGS, "\n".join(["##x", "\t".join(COLS + ["INFO"])] + [r + "\tx" for r in f3]) + "\n", "columns", None, None)]
    return t


def decided_oddities():
    """[(name, args, text)]: what looks odd and is decided all the same - a long INDEX or a position that is no number where the cluster
    test never reads it, missing cells in columns of strings"""
    long_chrom = "chr" + "x" * 70
    comments, cols, live = golden_live_rows()

    def golden(name, value):
        rows = list(live)
        f = rows[1].split("\t"); f[cols.index(name)] = value; rows[1] = "\t".join(f)
        return "\n".join(comments + rows) + "\n"
    return [("long_index_alone", ARGS, table(fillers() + [row(5000, CHROM=long_chrom), row(50_000, CHROM=long_chrom)])),
            ("odd_position_alone", ARGS, table(fillers() + [row(5000, CHROM="chr2", Start="5x3")])),
            ("odd_position_not_pass", ARGS, table(fillers() + [row(5000, CHROM="chr2", Start="5x3", Cancer=""), row(5100, CHROM="chr2")])),
            ("string_blank", ARGS, golden("Up_context", "")), ("string_nan", ARGS, golden("Up_context", "nan")), ("string_null", ARGS, golden("Fisher_p", "NULL"))]


def shapes():
    """[(name, args, text)]: row shapes the device's kernels care about"""
    A = ARGS

    def short(i, **kw):
        """a row of under 128 bytes: two or three starts in every 256-byte piece of the newline pass"""
        d = dict(Up_context="A", Down_context="T", BCp="0,1", CCp="0,1", Rest_BC="0", Rest_CC="0", INFO="x", Cancer="9|9|:::%d|:::9" % (1 if i % 3 == 1 else 9), NonCancer="",
                 Nc="4,4", Bc="5,0", Cc="2,0", Cell_type_Filter="PASS,x",
                 CHROM="chrM" if i % 7 == 3 else "chr1", FILTER="PoN_SR" if i % 11 == 5 else "PASS", Cell_types="Non-Cancer" if i % 13 == 6 else "Cancer,Non-Cancer")
        d.update(kw)
        return row(1000 + 20_000 * i, **d)
    assert len(short(0)) < 128
    t = [("rows_0", A, table([])), ("no_survivors", A, table([row(1000, Cell_types="Non-Cancer"), row(2000, FILTER="PoN_SR"), row(3000, CHROM="chrM", FILTER="LC_Upstream")]))]
    for n in (1, 255, 256, 257):
        t.append(("rows_%d" % n, A, table([row(1000 + 20_000 * i, Cancer="" if i % 3 == 1 else info(100, 40, "0:0:0:20:0:0", "50:0:0:50:0:0")) for i in range(n)])))
    t.append(("no_last_newline", A, table(fillers() + [row(5000)], newline_at_end=False)))
    t.append(("short_rows", A, table([short(i) for i in range(700)] + [short(700, Start="14000100", Cancer="9|9|:::9|:::9"), short(701, Start="14000200")])))
    # a newline at a piece's last byte: the first row ends at byte 255 of the data, the text on a piece's edge, with and without its last newline
    for newline in (True, False):
        first = short(0)
        rows = [short(0, Up_context="A" + "C" * (255 - len(first)))] + [short(i) for i in range(1, 6)]
        n = len("\n".join(rows)) + 1 + len(short(6)) + (1 if newline else 0)
        rows.append(short(6, Up_context="A" + "C" * ((-n) % 256)))
        text = table(rows, newline_at_end=newline)
        data = text[len("\n".join(hc.HEAD)) + 1:]
        assert data[255] == "\n" and len(data) % 256 == 0
        t.append(("piece_edge_%s" % ("newline" if newline else "bare"), A, text))
    t.append(("long_row", A, table(fillers(2) + [row(5000, Up_context="ACGT" * 1300)] + fillers(40, at=3_000_000))))
    t.append(("chrm_in_the_middle", A, table(fillers(2) + [row(500, CHROM="chrM"), row(7000), row(600, CHROM="chrM", Dp="99,100"), row(90_000, CHROM="chr2"), row(700, CHROM="chrM", FILTER="LR")] +
                                       fillers(2, at=3_000_000))))
    return t


def outcome(fn):
    """fn's result, or the type of what it raised"""
    try:
        return fn()
    except Exception as e:                              # noqa: BLE001 - (a table the reference's script dies on: the same death on every path)
        return type(e)


def run_files(fn, tmp_path, name, tag, args, **kw):
    """fn(table file, final file, unfiltered file, *args) -> (final text, unfiltered text), or the type of what it raised"""
    f, u = str(tmp_path / ("%s.%s.step3.tsv" % (name, tag))), str(tmp_path / ("%s.%s.step3.unfiltered.tsv" % (name, tag)))

    def go():
        fn(str(tmp_path / (name + ".tsv")), f, u, *args, **kw)
        return open(f).read(), open(u).read()
    return outcome(go)


def check_against_reference(tmp_path, name, args, text, fn, **kw):
    """fn leaves the two files calling.step3 returns for the same text, or raises what it raises"""
    (tmp_path / (name + ".tsv")).write_text(text)
    want = outcome(lambda: calling.step3(text, *args))
    got = run_files(fn, tmp_path, name, "got", args, **kw)
    if isinstance(want, type) or isinstance(got, type):
        assert got == want, (name, got, want)
    else:
        assert got[1] == want[1], (name, "unfiltered")
        assert got[0] == want[0], (name, "final")
    return got
