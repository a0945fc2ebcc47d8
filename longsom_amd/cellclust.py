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
                           stats: Optional[dict] = None) -> int:
    """The reads, contigs and `table` (hostio.BarcodeTable) must be resident in `engine`.  Writes <out_prefix>.SingleCellGenotype.tsv and
    the four <out_prefix>.{Dp,Alt,VAF,Binary}Matrix.tsv; returns the rows of the long table.  stats (a dict, filled in): per barcode the
    sites with coverage ("covered") and with MutationStatus PASS ("mutated"), as the twin step counts them."""
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
    if stats is not None:
        stats["covered"] = {bc: int(v) for bc, v in zip(barcodes, tally["n_covered"]) if v}
        stats["mutated"] = {bc: int(v) for bc, v in zip(barcodes, tally["n_pass"]) if v}
    return len(long_order) * n_cb
