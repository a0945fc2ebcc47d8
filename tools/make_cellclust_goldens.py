#!/usr/bin/env python3
"""SingleCellGenotype goldens: RUN the reference's own scripts/CellClustering/SingleCellGenotype.py (unmodified, imported from
/root/reference, no bytecode written) on the committed random BAMs and commit what it writes.  Runs only in the build container.

pysam is tools/minipysam.py's column-replay stand-in (see its header, and tools/make_pileup_goldens.py).  natsort is not installed either:
unless the real module imports, a stand-in is registered under its name — a key of alternating (text, unsigned integer) pieces with an
empty text in front of a leading number, written here on its own (longsom_amd/cellclust.py has the product's).  pandas is the installed
one.  So the matrices' row order and their float / empty-cell rendering are pinned by this restatement and this pandas, everything else
by the reference's code.

Writes under tests/golden/:
  cellclust.targets.tsv          about 60 target lines in pileup.rand.HCCV.tsv's layout, taken from it: the 49999 / 50000 / 50001 trio,
                                 chrM rows, I / D / N alts, alts with ",X", and one position named twice in its window (the last line wins)
  cellclust.fusions.tsv          #FusionName / BC pairs: a duplicated pair, a barcode of the sample, a barcode absent from it
  cellclust.<run>.SingleCellGenotype.tsv, .DpMatrix.tsv, .AltMatrix.tsv, .VAFMatrix.tsv, .BinaryMatrix.tsv for the runs
      rand.All   rand.Alt (--alt_flag Alt)   randsfx.All ("-1"-suffixed barcodes)   rand.p002 (--pvalue 0.002: BetaBin_problem rows)
      rand.fusions (--fusions cellclust.fusions.tsv; its long table is rand.All's and is not written twice)
  The matrices of rand.fusions are committed as text, to be read (floats, empty cells, fusion rows); the long tables (1 475 rows each) and
  the other runs' matrices as .tsv.gz (gzip level 9, no name, time stamp 0: the same bytes every time the tool runs).
"""
import contextlib
import gzip
import importlib.util
import io
import os
import re
import shutil
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference/workflow/scripts"
OUT = os.path.join(ROOT, "tests", "golden")
OUTPUTS = ("SingleCellGenotype", "DpMatrix", "AltMatrix", "VAFMatrix", "BinaryMatrix")

import minipysam  # noqa: E402


def natsorted_stand_in(seq):
    def key(s):
        k = [int(t) if t[0].isdigit() else t for t in re.findall(r"[0-9]+|[^0-9]+", s)]
        return ([""] + k) if k and isinstance(k[0], int) else k
    return sorted(seq, key=key)


def install_natsort():
    try:
        import natsort  # noqa: F401
        return "natsort %s" % natsort.__version__
    except ImportError:
        mod = types.ModuleType("natsort")
        mod.natsorted = natsorted_stand_in
        sys.modules["natsort"] = mod
        return "the stand-in of tools/make_cellclust_goldens.py"


def write_targets(path):
    src = [l for l in open(os.path.join(OUT, "pileup.rand.HCCV.tsv")).read().split("\n") if l]
    head, rows = [l for l in src if l.startswith("#")], [l.split("\t") for l in src if not l.startswith("#")]
    # sites at which some cell of the twin fixture (pileup.rand.genotype.All.tsv, the same BAM and lines) carries the expected alt
    hit = {(l.split("\t")[0], l.split("\t")[1]) for l in open(os.path.join(OUT, "pileup.rand.genotype.All.tsv")).read().split("\n")[1:] if l and l.split("\t")[10] != "0"}
    trio = [r for r in rows if r[0] == "chr1" and r[1] in ("49999", "50000", "50001")]
    with_alt = [r for r in rows if (r[0], r[1]) in hit and r not in trio]
    pick = trio + [r for r in with_alt if r[0] != "chrM"] + [r for r in with_alt if r[0] == "chrM"][:14]
    rest = [r for r in rows if r not in pick]
    pick += [r for r in rest if r[4][0] in "IDN"][::2][:12]
    pick += [r for r in rows if r not in pick and "," in r[4]][:6]
    pick += [r for r in rows if r not in pick and r[0] != "chrM"][:max(0, 59 - len(pick))]
    pick.sort(key=lambda r: rows.index(r))
    twice = next(r for r in pick if r[0] == "chr2")                                     # named again at the end of the file with another ALT
    again = list(twice); again[4] = "G" if twice[4][0] != "G" else "T"; again[13] = "7"
    with open(path, "w") as f:
        f.write("\n".join(head) + "\n" + "".join("\t".join(r) + "\n" for r in pick + [again]))
    return len(pick) + 1


def write_fusions(path, barcodes):
    rows = [("GENEA--GENEB", barcodes[3]), ("ABC1--DEF10", barcodes[0]), ("GENEA--GENEB", barcodes[3]), ("ABC1--DEF2", "GGGG9999TT"),
            ("ABC1--DEF10", barcodes[17]), ("GENEA--GENEB", barcodes[20])]
    with open(path, "w") as f:
        f.write("#FusionName\tBC\tLeftBreakpoint\n" + "".join("%s\t%s\tchr1:%d\n" % (n, b, 3 + i) for i, (n, b) in enumerate(rows)))


def main():
    minipysam.install()
    how = install_natsort()
    spec = importlib.util.spec_from_file_location("ref_cellgenotype", os.path.join(REF, "CellClustering", "SingleCellGenotype.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    targets = os.path.join(OUT, "cellclust.targets.tsv")
    n = write_targets(targets)
    cells = [l.split("\t")[0] for l in open(os.path.join(OUT, "pileup.rand.barcodes.tsv")).read().split("\n")[1:] if l]
    fusions = os.path.join(OUT, "cellclust.fusions.tsv")
    write_fusions(fusions, cells)
    import pandas
    print("%d target lines; natural sort: %s; pandas %s" % (n, how, pandas.__version__))
    work = tempfile.mkdtemp(prefix="cellclust_gold_")
    runs = [("rand.All", "rand", ["--alt_flag", "All"], None), ("rand.Alt", "rand", ["--alt_flag", "Alt"], None), ("randsfx.All", "randsfx", ["--alt_flag", "All"], None),
            ("rand.p002", "rand", ["--pvalue", "0.002"], None), ("rand.fusions", "rand", ["--alt_flag", "All"], fusions)]
    try:
        for name, bam, extra, fus in runs:
            prefix = os.path.join(work, name)
            old = sys.argv
            sys.argv = ["SingleCellGenotype.py", "--bam", os.path.join(OUT, "pileup.%s.bam" % bam), "--infile", targets, "--ref", os.path.join(OUT, "pileup.rand.fa"),
                        "--meta", os.path.join(OUT, "pileup.%s.barcodes.tsv" % bam), "--outfile", prefix, "--nprocs", "1", "--min_mq", "60",
                        "--tmp_dir", os.path.join(work, "tmp_" + name), "--chrM_contaminant", "True", "--fusions"] + ([fus] if fus else []) + extra
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    ref.main()
            finally:
                sys.argv = old
            for o in OUTPUTS:
                if fus and o == "SingleCellGenotype":
                    assert open(prefix + "." + o + ".tsv", "rb").read() == gzip.open(os.path.join(OUT, "cellclust.rand.All.SingleCellGenotype.tsv.gz")).read()
                    continue
                dst = os.path.join(OUT, "cellclust.%s.%s.tsv" % (name, o))
                if o != "SingleCellGenotype" and name == "rand.fusions":
                    shutil.copy(prefix + "." + o + ".tsv", dst)
                else:
                    with open(dst + ".gz", "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as z:
                        z.write(open(prefix + "." + o + ".tsv", "rb").read())
            text = open(prefix + ".SingleCellGenotype.tsv").read().split("\n")[1:]
            print(name, len([l for l in text if l]), "rows;", {s: sum(1 for l in text if l and l.split("\t")[13] == s) for s in
                                                                ("PASS", "BetaBin_problem", "LowVAFChrM", "NoAltReads", "NoCoverage")})
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
