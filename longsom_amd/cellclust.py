"""Per-cell genotypes at the final SNVs and the cell-by-variant matrices LongSom clusters cells by, host side:

  cell_genotype_matrices   <- main, run_interval, concatenate_sort_temp_files_and_write,
                              collect_cells_with_fusions, sort_chr_index, pivot_long_dataframe
                              scripts/CellClustering/SingleCellGenotype.py:84-228,277-379,402-471

The counting, the verdict of every (site, barcode) cell and the text of <prefix>.SingleCellGenotype.tsv, DpMatrix, AltMatrix, VAFMatrix and
BinaryMatrix are the device's (csrc/cellgeno.hip).  What is decided here is what the reference decides with Python containers and
pandas: which sites there are and in which order the long table lists them (reanno.read_target_windows and the set order of the
twin step), the matrices' row order (natsorted INDEX, chrM last, fusions after it), their columns (the distinct CB, sorted) and the
handful of fusion rows.  natsort is restated (natural_key): the module is not a dependency of this package.
"""
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import reanno

LONG_HEADER = reanno.GENOTYPE_HEADER + ["BinMutationStatus", "INDEX"]                      # SingleCellGenotype.py:305
MATRICES = ("Dp", "Alt", "VAF", "Binary")                                                  # <prefix>.<name>Matrix.tsv, :363-379
_DIGITS = re.compile(r"(\d+)")


class NoTargets(RuntimeError):
    pass


def natural_key(text: str) -> tuple:
    """natsort's default key: the string cut into (text, unsigned integer, text, ...), empty pieces dropped, an empty text in front when
    the string starts with a digit — so that position 0, 2, 4.. always hold text and 1, 3, 5.. integers."""
    parts = [int(p) if p.isdigit() else p for p in _DIGITS.split(text) if p != ""]
    if parts and isinstance(parts[0], int):
        parts.insert(0, "")
    return tuple(parts)                                 # (two integers never meet: the pattern takes every run of digits whole)


def matrix_row_order(indexes: Sequence[str]) -> List[int]:
    """sort_chr_index (:342-345) on the pivot's index: the pivot sorts the INDEX values as plain strings, natsorted then orders them by
    their natural key with every 'chrM' spelled 'chrZ' (stable: equal keys stay in string order).  Returns positions into `indexes`."""
    order = sorted(range(len(indexes)), key=lambda i: indexes[i])
    order.sort(key=lambda i: natural_key(indexes[i].replace("chrM", "chrZ")))
    return order


def matrix_label(index: str) -> str:
    """what sort_chr_index leaves as the row's name (:343,346)"""
    return index.replace("chrM", "chrZ").replace("chrZ", "chrM").replace("zzz:", "")


def read_fusions(path: Optional[str]) -> List[Tuple[str, str]]:
    """collect_cells_with_fusions (:325-340): (#FusionName, BC) pairs, the last of equal pairs kept, file order otherwise.  No file
    (--fusions without a value) or no data rows: no pairs."""
    if not path:
        return []
    import pandas as pd
    fus = pd.read_csv(path, sep="\t")
    fus["INDEX"] = fus["#FusionName"] + ":" + fus["BC"]
    fus = fus.drop_duplicates(subset="INDEX", keep="last")
    return [(str(n), str(b)) for n, b in zip(fus["#FusionName"], fus["BC"])]


def matrix_columns(barcodes: Sequence[str], fusions: Sequence[Tuple[str, str]], n_sites: int):
    """The matrices' columns: the distinct CB of the long table (every barcode, if there is a site) and of the fusion rows, in pandas'
    sorted order.  Returns (column names, col_src: the barcode's index or -1 for a barcode of the fusion file alone, float_cells:
    whether some (row, column) pair is absent — the pivot then holds NaN and the integer matrices print as floats)."""
    index_of = {b: i for i, b in enumerate(barcodes)} if n_sites else {}
    names = sorted(set(index_of) | {b for _, b in fusions})
    col_src = [index_of.get(n, -1) for n in names]
    pairs = set(fusions)
    gaps = (n_sites > 0 and -1 in col_src) or any((f, n) not in pairs for f in {f for f, _ in fusions} for n in names)
    return names, col_src, bool(gaps)


def fusion_rows(fusions: Sequence[Tuple[str, str]], columns: Sequence[str], float_cells: bool, vaf_as_float: bool = False) -> Dict[str, List[Tuple[str, str]]]:
    """The fusion rows of the four matrices as text (:337: Dp = ALT = VAF = BinMutationStatus = 1, INDEX 'zzz:' + name): per matrix a list
    of (INDEX, line).  A cell is 1 where the file names (fusion, barcode) and empty elsewhere; the integer matrices print it as pandas
    prints the float column around it, the VAF matrix (a column of strings) as the integer it is — unless every cell of the sample is
    covered, no '.' makes the column text, and it is a float column too (vaf_as_float)."""
    pairs = set(fusions)
    names = []
    for f, _ in fusions:
        if f not in names:
            names.append(f)
    out: Dict[str, List[Tuple[str, str]]] = {m: [] for m in MATRICES}
    for m in MATRICES:
        one = "1.0" if (vaf_as_float if m == "VAF" else float_cells) else "1"
        for f in names:
            out[m].append(("zzz:" + f, "\t".join([matrix_label("zzz:" + f)] + [one if (f, c) in pairs else "" for c in columns]) + "\n"))
    return out


def plan_sites(variant_file: str, contig_names: Sequence[str], window: int, chrm_contaminant: str):
    """The target sites as the device wants them (keys ascending, expected alt symbol, pileup windows, the chrM flag) and as the tables
    print them (heads, INDEX, the long table's site order).  The twin step (reanno.single_cell_genotype) states the reference's rules:
    windows by floor(POS / window) in file order, a site's last line wins, Python's set order inside a window, windows written by
    (chromosome text, smallest position)."""
    tid_of = {n: i for i, n in enumerate(contig_names)}
    blocks = []
    for lines in reanno.read_target_windows(variant_file, window).values():
        chrom = lines[0][0]
        sites: Dict[int, tuple] = {}
        for el in lines:
            sites[int(el[1]) - 1] = (el[3], el[4].split(",")[0], el[6], el[13])      # :98-109 (ALT up to its first comma)
        blocks.append((chrom, min(sites), list(set(sites.keys())), sites))              # CELLS is built by iterating this very set (:112,130)
    if not blocks:
        return None
    key_of = {}
    for chrom, _, order, _ in blocks:
        if chrom not in tid_of:
            raise ValueError("contig %r of %s is not in the BAM header" % (chrom, variant_file))
        for p in order:
            key_of[(chrom, p)] = (tid_of[chrom] << 32) | p
    uniq = sorted(set(key_of.values()))
    row_of = {k: i for i, k in enumerate(uniq)}
    n = len(uniq)
    alt_sym = np.full(n, 255, np.uint8); is_chrm = np.zeros(n, np.uint8)
    heads, indexes = [""] * n, [""] * n
    for chrom, _, order, sites in blocks:
        for p in order:
            i = row_of[key_of[(chrom, p)]]
            ref_e, alt_e, ct_e, nc_e = sites[p]
            alt_sym[i] = reanno.SYM_OF_BASE.get(alt_e, 255)
            is_chrm[i] = 1 if (chrm_contaminant == "True" and chrom == "chrM") else 0   # :197
            heads[i] = "\t".join([chrom, str(p + 1), str(p + 1), ref_e, alt_e, ct_e, nc_e])
            indexes[i] = chrom + ":" + str(p + 1) + ":" + alt_e.split(",")[0]             # :221
    keys = np.asarray(uniq, np.int64)
    code = (keys >> 32) * (1 << 40) + ((keys & 0xFFFFFFFF) + 1) // int(window)
    group_off = np.concatenate([[0], np.nonzero(np.diff(code))[0] + 1, [n]]).astype(np.int64)
    by_chrom: Dict[str, Dict[int, tuple]] = {}
    for b in blocks:
        by_chrom.setdefault(b[0], {})[b[1]] = b                                          # a later window with the same (chrom, start) replaces (:296-300)
    long_order = [row_of[key_of[(chrom, p)]] for chrom in sorted(by_chrom) for start in sorted(by_chrom[chrom]) for p in by_chrom[chrom][start][2]]
    return keys, alt_sym, is_chrm, group_off, heads, indexes, long_order


def cell_genotype_matrices(engine, variant_file: str, table, contig_names: Sequence[str], out_prefix: str, fusion_file: Optional[str] = None, *,
                           alt_flag: str = "All", window: int = 50000, min_bq: int = 30, min_mq: int = 255, alpha2: float = 0.2474528917555431,
                           beta2: float = 162.03696139428595, pvalue: float = 0.01, chrm_contaminant: str = "True", max_depth: int = 200000,
                           stats: Optional[dict] = None, bnpc_prefix: Optional[str] = None, bnpc_barcodes: Optional[str] = None, min_cells_per_mut: int = 5,
                           min_pos_cov: int = 3) -> int:
    """The reads, contigs and `table` (hostio.BarcodeTable) must be resident in `engine`.  Writes <out_prefix>.SingleCellGenotype.tsv and
    the four <out_prefix>.{Dp,Alt,VAF,Binary}Matrix.tsv; returns the rows of the long table.  stats (a dict, filled in): per barcode the
    sites with coverage ("covered") and with MutationStatus PASS ("mutated"), as the twin step counts them.  bnpc_prefix: also write
    BnpC's input (format_bnpc_input: rule FormatInputBnpC with bnpc_barcodes as its --barcodes) from the cells while they are resident."""
    from ._lib import GenotypeParams
    plan = plan_sites(variant_file, contig_names, window, chrm_contaminant)
    if plan is None:
        print("No temporary files found")                                               # :323; the reference then dies reading the table it never wrote (:353)
        raise NoTargets("%s names no target site: no %s.SingleCellGenotype.tsv to pivot (the reference stops here too, in read_csv)" % (variant_file, out_prefix))
    keys, alt_sym, is_chrm, group_off, heads, indexes, long_order = plan
    # the CB tag is cleaned before the lookup (:164-169): a "-1" suffix does not hide a read (strict_cb = 0)
    params = GenotypeParams.longsom_defaults(min_bq=int(min_bq), min_mq=int(min_mq), alt_only=1 if alt_flag == "Alt" else 0, strict_cb=0)
    engine.cellgeno_count(keys, alt_sym, is_chrm, group_off, params, max_depth, alpha2, beta2, pvalue)
    tally = engine.cellgeno_fetch(cells=False)
    barcodes = list(table.barcodes)
    n_cb = len(barcodes)
    fusions = read_fusions(fusion_file)
    # rows of the long table the pivot sees: a window replaced by a later one of the same start is not in the file
    listed = sorted(set(long_order))
    columns, col_src, float_cells = matrix_columns(barcodes, fusions, len(listed))
    all_index = [indexes[i] for i in listed] + ["zzz:" + f for f in dict.fromkeys(f for f, _ in fusions)]
    order = matrix_row_order(all_index)
    mat_order = [listed[i] for i in order if i < len(listed)]
    celltypes = [table.celltype_names[int(c)] for c in table.celltype_of]
    engine.cellgeno_set_text(heads, indexes, [matrix_label(s) for s in indexes], barcodes, celltypes, long_order, mat_order, col_src, float_cells)
    long_path = out_prefix + ".SingleCellGenotype.tsv"
    with open(long_path, "w") as f:
        f.write("\t".join(LONG_HEADER) + "\n")
    engine.format_table(engine.TABLE_CELL_LONG)
    engine.append_table(engine.TABLE_CELL_LONG, long_path)
    engine.free_table(engine.TABLE_CELL_LONG)
    all_covered = int(tally["n_covered"].sum()) == len(keys) * n_cb                      # no "." in the VAF column: pandas reads it as floats
    frows = fusion_rows(fusions, columns, float_cells, vaf_as_float=all_covered)
    slots = {"Dp": engine.TABLE_CELL_DP, "Alt": engine.TABLE_CELL_ALT, "VAF": engine.TABLE_CELL_VAF, "Binary": engine.TABLE_CELL_BIN}
    # where the fusion rows fall among the rows the device prints: after all of them (their 'zzz:' sorts last) unless a contig's name says otherwise
    after = [sum(1 for j in order[:k] if j < len(listed)) for k, i in enumerate(order) if i >= len(listed)]
    by_index = {m: dict(frows[m]) for m in MATRICES}
    for m in MATRICES:
        path = out_prefix + "." + m + "Matrix.tsv"
        lines = [by_index[m][all_index[i]] for i in order if i >= len(listed)]
        with open(path, "w") as f:
            f.write("\t".join([""] + columns) + "\n")                                    # (the index has lost its name in sort_chr_index)
        n_bytes = engine.format_table(slots[m])
        if all(a == len(mat_order) for a in after):
            engine.append_table(slots[m], path)
            with open(path, "a") as f:
                f.write("".join(lines))
        else:
            rows = engine.table_bytes(slots[m], n_bytes).decode().splitlines(True)
            for a, line in sorted(zip(after, lines), key=lambda t: -t[0]):
                rows.insert(a, line)
            with open(path, "a") as f:
                f.write("".join(rows))
        engine.free_table(slots[m])
    if bnpc_prefix:
        fusion_order = [matrix_label(all_index[i]) for i in order if i >= len(listed)]
        if any("--" not in f for f in fusion_order) or any("--" in matrix_label(indexes[i]) for i in mat_order):
            # FormatInputBnpC.py:11 tells a fusion row by the "--" in its label: where that is not the fusion file's rows, the files decide
            format_bnpc_input_host(out_prefix + ".BinaryMatrix.tsv", out_prefix + ".VAFMatrix.tsv", bnpc_barcodes, bnpc_prefix, min_cells_per_mut, min_pos_cov)
        else:
            format_bnpc_input(engine, columns, fusions, bnpc_barcodes, bnpc_prefix, min_cells_per_mut, min_pos_cov, float_cells=float_cells, fusion_order=fusion_order)
    if stats is not None:
        stats["covered"] = {bc: int(v) for bc, v in zip(barcodes, tally["n_covered"]) if v}
        stats["mutated"] = {bc: int(v) for bc, v in zip(barcodes, tally["n_pass"]) if v}
    return len(long_order) * n_cb


# ---- BnpC's input: scripts/CellClustering/FormatInputBnpC.py:6-35 (rule FormatInputBnpC, rules/CellClustering.smk:105-133) ----------------
# The script reads BinaryMatrix and VAFMatrix back with 3 and "." as NA (:7-8), sets the fusion rows (labels with "--") aside (:11-13),
# keeps the SNV rows more than min_cells_per_mut cells carry as 1 (:16), then the columns covered at more than min_pos_cov of those rows
# (:19), and prints the kept SNV rows, then all fusion rows, over the kept columns (:21-34) with the listed barcodes' table (:26,30,35).
# The two filters, the compaction and the SNV rows' text are the device's (csrc/cellgeno.hip: lsg_cellgeno_filter, tables
# LSG_TABLE_BNPC_*); the fusion rows, the header and Barcodes.tsv are written here.
BNPC_OUTPUTS = ("BinaryMatrix", "VAFMatrix", "Barcodes")
_BIN_CODE = {"0": 0, "1": 1, "3": 3, "0.0": 0, "1.0": 1, "3.0": 3, "": 3}                   # what :7 reads a Binary cell as (3 = NA)
_BIN_INT_TEXT = ("0", "1")                                                                  # ... and the texts that leave a column int64


class HandBack(Exception):
    """a matrix file holds something the device form does not state: the host twin takes the step"""


def write_bnpc_barcodes(barcodes_file: str, kept_columns: Sequence[str], out_path: str) -> int:
    """:9,26,30,35 - the rows of --barcodes whose Index is a kept column, in that file's order, with the re-annotation's colour"""
    import pandas as pd
    bc = pd.read_csv(barcodes_file, sep="\t")
    bc = bc[bc["Index"].isin(list(kept_columns))].copy()
    bc["Cell_Reanno_Colors"] = ["#94C773" if x == "Non-Cancer" else "#8F79A1" for x in bc["Reannotated_cell_type"]]
    bc.to_csv(out_path, sep="\t", index=False)
    return len(bc)


def format_bnpc_input_host(bin_path: str, vaf_path: str, barcodes_path: str, out_prefix: str, min_cells_per_mut: int = 5, min_pos_cov: int = 3):
    """The whole step in pandas, restated from the rules above: the twin the device forms are tested against, and the path a matrix file
    the device form does not state is handed back to.  Returns (rows written, columns kept)."""
    import pandas as pd
    na = [3, "."]
    b = pd.read_csv(bin_path, sep="\t", index_col=0, na_values=na)                        # :7
    v = pd.read_csv(vaf_path, sep="\t", index_col=0, na_values=na)                        # :8
    fusion = np.array(["--" in str(i) for i in b.index], bool)                             # :11
    snv = b[~fusion]
    snv = snv[(snv.notna() & (snv != 0)).sum(axis=1) > min_cells_per_mut]                  # :16 (NA and 0 are not counted)
    snv = snv.loc[:, snv.notna().sum(axis=0) > min_pos_cov]                                # :19 (over the kept SNV rows alone)
    rows = list(snv.index) + list(b.index[fusion])                                         # :21
    pd.concat([snv, b.loc[fusion, snv.columns]]).to_csv(out_prefix + ".BinaryMatrix.tsv", sep="\t")      # :27,33
    v.loc[rows, snv.columns].to_csv(out_prefix + ".VAFMatrix.tsv", sep="\t")               # :25,34
    write_bnpc_barcodes(barcodes_path, [str(c) for c in snv.columns], out_prefix + ".Barcodes.tsv")
    return len(rows), len(snv.columns)


def bnpc_col_int_ok(columns: Sequence[str], fusions: Sequence[Tuple[str, str]], float_cells: bool) -> List[int]:
    """The host's half of a Binary column's dtype in the fused form: pandas reads a column of <id>.BinaryMatrix.tsv as int64 iff no cell
    of it is empty or float text, over all rows.  SingleCellGenotype.py prints every cell as a float when its pivot had a gap
    (float_cells), and a fusion row is empty wherever the barcode does not carry the fusion.  (Coverage at every site is the device's half.)"""
    pairs = set(fusions)
    names = list(dict.fromkeys(f for f, _ in fusions))
    return [int(not float_cells and all((f, c) in pairs for f in names)) for c in columns]


def _vaf_code(text: str, cache: dict) -> int:
    """a VAF cell as the device states it: -1 for NA, else k with text == repr(k / 1e4) (or the integers 0 and 1)"""
    k = cache.get(text)
    if k is None:
        if text in ("", "."):
            k = -1
        else:
            try:
                k = int(round(float(text) * 10000))
            except (ValueError, OverflowError):                                         # ("inf" parses and cannot be rounded)
                raise HandBack("VAF cell %r" % text)
            if not (0 <= k <= 10000 and (repr(k / 10000.0) == text or text in ("0", "1"))):
                raise HandBack("VAF cell %r is not a 4-decimal repr" % text)
        cache[text] = k
    return k


def read_bnpc_matrices(bin_path: str, vaf_path: str):
    """The two matrix files as the device takes them.  Returns (columns, SNV labels, bin [n_snv, n_cols] uint8, vaf4 int32, fusion labels,
    their bin and vaf4 rows, col_int_ok).  Raises HandBack for whatever lsg_cellgeno_load_cells cannot state as pandas would read it:
    quoting, blank or ragged lines, duplicate labels or columns, VAF rows or columns other than Binary's, a Binary value outside
    {0, 1, 3, empty and their .0 forms}, a VAF text that is not repr(k / 1e4), a VAF column that pandas would read as integers."""
    def table(path):
        import gzip
        with (gzip.open(path, "rt", newline="") if path.endswith(".gz") else open(path, newline="")) as f:
            text = f.read()
        if '"' in text or "\r" in text or not text.endswith("\n"):
            raise HandBack("%s: quoting, carriage returns or no final newline" % path)
        lines = text[:-1].split("\n")
        head = lines[0].split("\t")
        rows = [l.split("\t") for l in lines[1:]]
        if head[0] != "" or len(set(head[1:])) != len(head) - 1 or any(len(r) != len(head) or r[0] == "" for r in rows) or not rows:
            raise HandBack("%s: not a labelled matrix with unique columns" % path)
        return head[1:], rows
    columns, brows = table(bin_path)
    vcolumns, vrows = table(vaf_path)
    labels = [r[0] for r in brows]
    if not columns or vcolumns != columns or [r[0] for r in vrows] != labels or len(set(labels)) != len(labels):
        raise HandBack("the matrices differ in rows or columns, or a label repeats")
    n, m = len(labels), len(columns)
    bin_ = np.zeros((n, m), np.uint8); vaf4 = np.zeros((n, m), np.int32)
    int_ok = np.ones(m, bool); vaf_float = np.zeros(m, bool)
    cache: dict = {}
    try:
        for i, (br, vr) in enumerate(zip(brows, vrows)):
            bin_[i] = [_BIN_CODE[t] for t in br[1:]]
            int_ok &= [t in _BIN_INT_TEXT for t in br[1:]]
            vaf4[i] = [_vaf_code(t, cache) for t in vr[1:]]
            vaf_float |= [t not in _BIN_INT_TEXT for t in vr[1:]]
    except KeyError as e:
        raise HandBack("Binary cell %s" % e)
    if not vaf_float.all():
        raise HandBack("a VAF column of integers")
    fusion = np.array(["--" in l for l in labels], bool)
    pick = lambda flag: [l for l, f in zip(labels, fusion) if f == flag]
    return columns, pick(False), bin_[~fusion], vaf4[~fusion], pick(True), bin_[fusion], vaf4[fusion], int_ok.astype(np.uint8)


def _write_bnpc(engine, columns, col_int_ok, fusion_labels, fusion_bin, fusion_vaf4, barcodes_file, out_prefix, min_cells_per_mut, min_pos_cov):
    """filter on the device, then the three files: header, the device's rows, the fusion rows (:27: by the column's dtype in Binary, floats in VAF)"""
    n_rows, n_cols = engine.cellgeno_filter(min_cells_per_mut, min_pos_cov, col_int_ok)
    f = engine.cellgeno_filter_fetch()
    kept = np.nonzero(f["col_keep"])[0]
    assert len(kept) == n_cols and int(f["row_keep"].sum()) == n_rows
    names = [columns[i] for i in kept]
    header = "\t".join([""] + names) if names else '""'                                # (to_csv quotes the lone empty field of a frame without columns)
    for name, slot in (("BinaryMatrix", engine.TABLE_BNPC_BIN), ("VAFMatrix", engine.TABLE_BNPC_VAF)):
        path = out_prefix + "." + name + ".tsv"
        with open(path, "w") as out:
            out.write(header + "\n")
        engine.format_table(slot)
        engine.append_table(slot, path)
        engine.free_table(slot)
        with open(path, "a") as out:
            for label, b, v in zip(fusion_labels, fusion_bin, fusion_vaf4):
                if name == "BinaryMatrix":
                    cells = ["" if b[i] == 3 else str(int(b[i])) + ("" if f["col_int"][i] else ".0") for i in kept]
                else:
                    cells = ["" if v[i] < 0 else repr(int(v[i]) / 10000.0) for i in kept]
                out.write("\t".join([label] + cells) + "\n")
    write_bnpc_barcodes(barcodes_file, names, out_prefix + ".Barcodes.tsv")
    return n_rows + len(fusion_labels), n_cols


def format_bnpc_input(engine, columns: Sequence[str], fusions: Sequence[Tuple[str, str]], barcodes_file: str, out_prefix: str,
                      min_cells_per_mut: int = 5, min_pos_cov: int = 3, *, float_cells: bool = False, fusion_order: Optional[Sequence[str]] = None):
    """BnpC's input from the state cell_genotype_matrices leaves resident (cells, mat_order, col_src): <out_prefix>.BinaryMatrix.tsv,
    .VAFMatrix.tsv and .Barcodes.tsv as FormatInputBnpC.py writes them from that run's matrices, without reading those back.  columns,
    fusions, float_cells: as cell_genotype_matrices made them; fusion_order: the fusion names in the matrices' row order (default: the
    pairs' order).  Returns (rows written, columns kept)."""
    pairs = set(fusions)
    names = list(fusion_order) if fusion_order is not None else list(dict.fromkeys(f for f, _ in fusions))
    carried = np.array([[1 if (f, c) in pairs else 3 for c in columns] for f in names], np.uint8).reshape(len(names), len(columns))
    return _write_bnpc(engine, list(columns), bnpc_col_int_ok(columns, fusions, float_cells), names, carried, np.where(carried == 1, 10000, -1),
                       barcodes_file, out_prefix, min_cells_per_mut, min_pos_cov)


def format_bnpc_input_files(engine, bin_path: str, vaf_path: str, barcodes_path: str, out_prefix: str, min_cells_per_mut: int = 5, min_pos_cov: int = 3):
    """The file-in form: the two matrices parsed, their SNV rows made resident (cellgeno_load_cells + cellgeno_set_text), then as above.
    A file the device form does not state goes to format_bnpc_input_host.  Returns (rows written, columns kept, "device" or "host")."""
    try:
        columns, labels, bin_, vaf4, f_labels, f_bin, f_vaf4, int_ok = read_bnpc_matrices(bin_path, vaf_path)
    except HandBack:
        return format_bnpc_input_host(bin_path, vaf_path, barcodes_path, out_prefix, min_cells_per_mut, min_pos_cov) + ("host",)
    n, m = len(labels), len(columns)
    engine.cellgeno_load_cells(bin_.reshape(n, m), vaf4.reshape(n, m))
    engine.cellgeno_set_text([""] * n, [""] * n, labels, columns, [""] * m, [], list(range(n)), list(range(m)), False)
    return _write_bnpc(engine, columns, int_ok, f_labels, f_bin, f_vaf4, barcodes_path, out_prefix, min_cells_per_mut, min_pos_cov) + ("device",)
