#!/usr/bin/env python3
"""FormatInputBnpC goldens: RUN the reference's own scripts/CellClustering/FormatInputBnpC.py (unmodified, imported from the reference
tree given by --reference, no bytecode written) on matrices that are goldens already and commit what it writes.  The script needs
pandas and numpy only; pandas is the installed one, so the float / integer / empty-cell rendering is pinned by this pandas and
everything else by the reference's code.

Writes under tests/golden/:
  bnpc.barcodes.tsv                  Index / Cell_type / Reannotated_cell_type of pileup.rand.barcodes.tsv's barcodes, in reversed order (not
                                     the columns'), every third cell re-annotated to the other type, plus one barcode no matrix has
  bnpc.small.in.BinaryMatrix.tsv, bnpc.small.in.VAFMatrix.tsv, bnpc.small.barcodes.tsv
                                     a matrix pair written here as data, in the integer form SingleCellGenotype.py prints when its pivot
                                     has no gap: two barcodes covered at every site (integer columns beside float ones), a row whose count
                                     of 1s equals min_cells_per_mut and one with one more, a column whose coverage over the kept rows
                                     equals min_pos_cov and one with one more, an all-3 column, a fusion row carried by every barcode
  bnpc.<case>.BinaryMatrix.tsv, .VAFMatrix.tsv, .Barcodes.tsv for the cases
      rand.fusions.c0p8   cellclust.rand.fusions, --min_cells_per_mut 0 --min_pos_cov 8: the fusion-only barcode dropped, fusion rows last
      rand.All.c0p8       cellclust.rand.All with the same thresholds
      rand.All.c1p3       one row and no column left: the header is '""'
      rand.All.c5p3       the script's defaults: no SNV row left
      small.c1p2          the pair above
"""
import argparse
import contextlib
import importlib.util
import io
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
OUTPUTS = ("BinaryMatrix", "VAFMatrix", "Barcodes")

SMALL_COLUMNS = ["B01", "B02", "B03", "B04", "B05", "B06", "B07"]
# (label, Binary cells, VAF cells): thresholds (1, 2)
SMALL_ROWS = [
    ("chr1:10:A", "1 1 0 3 3 0 3", "0.5 1.0 0.0 . . 0.0 ."),            # two 1s = min + 1: kept
    ("chr1:20:C", "1 3 0 3 0 3 3", "0.3333 . 0.0 . 0.0 . ."),          # one 1 = min: dropped
    ("chr1:30:G", "1 1 1 0 3 3 3", "0.25 0.6667 1.0 0.0 . . ."),
    ("chr2:5:T", "0 1 1 1 3 0 3", "0.0 0.125 0.0909 1.0 . 0.0 ."),
    ("chr2:9:A", "1 0 1 1 0 3 3", "0.8 0.0417 0.75 0.5 0.0 . ."),
    ("chrM:7:G", "0 0 0 0 3 3 3", "0.0 0.1 0.2857 0.0 . . ."),         # covered, never mutated: dropped
    ("G1--G2", "1 1 1 1 1 1 1", "1 1 1 1 1 1 1"),
]   # over the four kept rows: B04 is covered 3 times (min + 1: kept), B06 twice (min: dropped), B05 once, B07 never; B01 and B03 everywhere


def write_small():
    for name, pick in (("BinaryMatrix", 1), ("VAFMatrix", 2)):
        with open(os.path.join(OUT, "bnpc.small.in.%s.tsv" % name), "w") as f:
            f.write("\t".join([""] + SMALL_COLUMNS) + "\n")
            for row in SMALL_ROWS:
                f.write("\t".join([row[0]] + row[pick].split(" ")) + "\n")
    with open(os.path.join(OUT, "bnpc.small.barcodes.tsv"), "w") as f:
        f.write("Index\tCell_type\tReannotated_cell_type\n")
        for b, ct, re_ct in (("B06", "Cancer", "Cancer"), ("B03", "Non-Cancer", "Cancer"), ("B01", "Cancer", "Cancer"), ("B09", "Cancer", "Non-Cancer"),
                             ("B04", "Non-Cancer", "Non-Cancer"), ("B02", "Cancer", "Non-Cancer"), ("B07", "Non-Cancer", "Non-Cancer"), ("B05", "Cancer", "Cancer")):
            f.write("%s\t%s\t%s\n" % (b, ct, re_ct))


def write_barcodes():
    rows = [l.split("\t") for l in open(os.path.join(OUT, "pileup.rand.barcodes.tsv")).read().split("\n")[1:] if l]
    other = {"Cancer": "Non-Cancer", "Non-Cancer": "Cancer"}
    with open(os.path.join(OUT, "bnpc.barcodes.tsv"), "w") as f:
        f.write("Index\tCell_type\tReannotated_cell_type\n")
        for i, (b, ct) in enumerate(reversed(rows)):
            if i == 7:
                f.write("CCCC0000AA\tCancer\tCancer\n")                             # in no matrix
            f.write("%s\t%s\t%s\n" % (b, ct, other.get(ct, ct) if i % 3 == 0 else ct))


def cases():
    def m(run, name):
        p = os.path.join(OUT, "cellclust.%s.%s.tsv" % (run, name))
        return p if os.path.exists(p) else p + ".gz"                                # (pandas reads the gzipped fixtures as they are)
    rand = os.path.join(OUT, "bnpc.barcodes.tsv")
    return [("rand.fusions.c0p8", m("rand.fusions", "BinaryMatrix"), m("rand.fusions", "VAFMatrix"), rand, 0, 8),
            ("rand.All.c0p8", m("rand.All", "BinaryMatrix"), m("rand.All", "VAFMatrix"), rand, 0, 8),
            ("rand.All.c1p3", m("rand.All", "BinaryMatrix"), m("rand.All", "VAFMatrix"), rand, 1, 3),
            ("rand.All.c5p3", m("rand.All", "BinaryMatrix"), m("rand.All", "VAFMatrix"), rand, 5, 3),
            ("small.c1p2", os.path.join(OUT, "bnpc.small.in.BinaryMatrix.tsv"), os.path.join(OUT, "bnpc.small.in.VAFMatrix.tsv"),
             os.path.join(OUT, "bnpc.small.barcodes.tsv"), 1, 2)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a LongSom checkout (the directory that holds workflow/)")
    a = ap.parse_args()
    script = os.path.join(a.reference, "workflow", "scripts", "CellClustering", "FormatInputBnpC.py")
    spec = importlib.util.spec_from_file_location("ref_formatinputbnpc", script)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    write_small()
    write_barcodes()
    import pandas
    print("pandas", pandas.__version__)
    work = tempfile.mkdtemp(prefix="bnpc_gold_")
    try:
        for name, bin_path, vaf_path, barcodes, c, p in cases():
            prefix = os.path.join(work, name)
            old = sys.argv
            sys.argv = ["FormatInputBnpC.py", "--bin", bin_path, "--vaf", vaf_path, "--barcodes", barcodes, "--min_pos_cov", str(p), "--min_cells_per_mut", str(c),
                        "--outfile", prefix]
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    ref.main()
            finally:
                sys.argv = old
            for o in OUTPUTS:
                shutil.copy(prefix + "." + o + ".tsv", os.path.join(OUT, "bnpc.%s.%s.tsv" % (name, o)))
            lines = open(prefix + ".BinaryMatrix.tsv").read().split("\n")
            print(name, len(lines) - 2, "rows,", len(lines[0].split("\t")) - 1 if "\t" in lines[0] else 0, "columns,", len(open(prefix + ".Barcodes.tsv").read().split("\n")) - 2, "barcodes")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
