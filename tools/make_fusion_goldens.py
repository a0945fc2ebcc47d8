#!/usr/bin/env python3
"""Fusion-branch goldens: RUN the reference's own FusionCalling/BamToFastq.py and FusionCalling/FusionCalling.py (unmodified, loaded from
the reference tree given with --reference, no bytecode written) on small inputs and commit what they write under tests/golden/fusion/.

  plain.bam, plain.fastq             a hand-authored BAM (tests/support/fastq_cases.py: the edge cases without the 70 000-base read, plus
                                     the routed cases that carry a CB) and what bam_to_fastq wrote for it
  routed.bam, routed.meta.tsv,       the routed-mode BAM, its barcode table, and the reference chain's FASTQ: hostio.split_bam's per-cell-type
  routed.fastq, routed.nM2.fastq     BAMs (checked against the reference's split_bam elsewhere) -> bam_to_fastq each -> concatenated in
                                     cell-type order (rules BamToFastq + ConcatFastq); .nM2: the same under --max_nM 2
  predictions.tsv, barcodes.tsv      a ctat-LR-fusion predictions table that reaches every filter outcome, a duplicated fusion name and a
                                     non-ONLY_REF_SPLICE row, and its barcode table
  fusionsunfiltered.Fusions.tsv, fusions.Fusions.tsv, fusions.Fusions.SingleCellGenotype.tsv
                                     what fusion_report wrote for them with --outdir .../fusions (3, 2, 0.1, 0.3: the config's values)

pysam is not installed, so BamToFastq.py runs over a stand-in (below) that provides what the script touches - AlignmentFile iteration
with check_sq=False, read.to_dict(), has_tag, get_tag - written from the SAM specification (sections 1.4, 4.2) and pysam's documented
behaviour: to_dict() renders the record's SAM fields as strings, has_tag / get_tag follow htslib's bam_aux_get (the FIRST field of that
name), get_tag(tag, with_value_type=True) returns (value, type code).  That pins the script's own name / CB / UMI logic; the SEQ / QUAL
rendering rests on the specification, which is why tests/support/fastq_cases.py also states every case's text by hand.
FusionCalling.py needs only pandas and runs as it is."""
import argparse
import importlib.util
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tools.minipysam import read_bgzf  # noqa: E402

_NT16 = "=ACMGRSVTWYHKDBN"


class Segment:
    """One BAM record with the three calls BamToFastq.py makes"""

    def __init__(self, raw):
        self.raw = raw
        (self.tid, self.pos, l_name, self.mapq, _bin, n_cigar, self.flag, l_seq, _mt, _mp, _tl) = struct.unpack_from("<iiBBHHHIiii", raw, 0)
        p = 32
        self.query_name = raw[p:p + l_name].split(b"\0")[0].decode(); p += l_name + 4 * n_cigar
        packed = raw[p:p + (l_seq + 1) // 2]; p += (l_seq + 1) // 2
        self._seq = "".join(_NT16[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
        self._qual = raw[p:p + l_seq]; p += l_seq
        self._aux = []                     # (tag, type code, value) in record order
        while p + 3 <= len(raw):
            tag, ty = raw[p:p + 2].decode(), chr(raw[p + 2]); p += 3
            if ty == "A":
                v = chr(raw[p]); p += 1
            elif ty in "cC":
                v = struct.unpack_from("<b" if ty == "c" else "<B", raw, p)[0]; p += 1
            elif ty in "sS":
                v = struct.unpack_from("<h" if ty == "s" else "<H", raw, p)[0]; p += 2
            elif ty in "iI":
                v = struct.unpack_from("<i" if ty == "i" else "<I", raw, p)[0]; p += 4
            elif ty == "f":
                v = struct.unpack_from("<f", raw, p)[0]; p += 4
            elif ty in "ZH":
                e = raw.index(b"\0", p); v = raw[p:e].decode(); p = e + 1
            elif ty == "B":
                st, cnt = chr(raw[p]), struct.unpack_from("<I", raw, p + 1)[0]
                size = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[st]
                v = raw[p + 5:p + 5 + cnt * size]; p += 5 + cnt * size
            else:
                raise ValueError("aux type %r" % ty)
            self._aux.append((tag, ty, v))

    def to_dict(self):
        """the SAM line's fields as strings (SEQ '*' without bases; QUAL '*' without bases or with 0xFF qualities, else Phred + 33)"""
        qual = "*" if not self._seq or self._qual[0] == 0xFF else "".join(chr(q + 33) for q in self._qual)
        return {"name": self.query_name, "flag": str(self.flag), "seq": self._seq or "*", "qual": qual}

    def has_tag(self, tag):
        return any(t == tag for t, _, _ in self._aux)

    def get_tag(self, tag, with_value_type=False):
        for t, ty, v in self._aux:
            if t == tag:
                return (v, ty) if with_value_type else v
        raise KeyError("tag '%s' not present" % tag)


class AlignmentFile:
    def __init__(self, path, mode="rb", check_sq=True, **kw):
        d = read_bgzf(path)
        assert d[:4] == b"BAM\1", path
        p = 8 + struct.unpack_from("<I", d, 4)[0]
        n_ref = struct.unpack_from("<I", d, p)[0]; p += 4
        for _ in range(n_ref):
            p += 4 + struct.unpack_from("<I", d, p)[0] + 4
        self._reads = []
        while p + 4 <= len(d):
            bs = struct.unpack_from("<I", d, p)[0]
            self._reads.append(d[p + 4:p + 4 + bs]); p += 4 + bs

    def __iter__(self):                    # every record of the file, unmapped ones too
        return (Segment(r) for r in self._reads)


def load_reference_script(path):
    pysam = types.ModuleType("pysam")
    pysam.AlignmentFile = AlignmentFile
    sys.modules["pysam"] = pysam
    spec = importlib.util.spec_from_file_location("ref_bam_to_fastq", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PREDICTIONS_HEADER = ["#FusionName", "num_LR", "LeftGene", "LeftLocalBreakpoint", "LeftBreakpoint", "RightGene", "RightLocalBreakpoint", "RightBreakpoint", "SpliceType",
                      "LR_accessions"]


def predictions_rows():
    """30 cancer cells C00..C29, 20 non-cancer cells N00..N19 (barcodes_rows).  One row per filter outcome:"""
    acc = lambda items: ",".join("%s^%s^read%d" % (bc, umi, i) for i, (bc, umi) in enumerate(items))
    many_c = [("C%02d" % i, "U%02d" % i) for i in range(12)]                                    # 12 cancer cells: MCF 0.4
    return [
        ["A--B", 12, "A", 100, "chr1:1000:+", "B", 200, "chr2:2000:-", "ONLY_REF_SPLICE", acc(many_c)],                               # PASS, no non-cancer
        ["A--B", 2, "A", 101, "chr1:1001:+", "B", 201, "chr2:2001:-", "ONLY_REF_SPLICE", acc([("C00", "U1"), ("C01", "U2")])],         # duplicated name: A--B2, 2 UMIs -> Low_Cancer_UMI
        ["C--D", 3, "C", 300, "chr3:3000:+", "D", 400, "chr4:4000:+", "ONLY_REF_SPLICE", acc([("C00", "U1"), ("C00", "U2"), ("C00", "U3")])],      # 3 UMIs, 1 cell -> Low_Cancer_BC
        ["E--F", 6, "E", 500, "chr5:5000:+", "F", 600, "chr6:6000:-", "ONLY_REF_SPLICE",
         acc([("C00", "U1"), ("C01", "U2"), ("C02", "U3"), ("N00", "U4"), ("N01", "U5"), ("XX", "U6")])],                            # MCF 0.1 - 0.1 < 0.3 -> Low_delta_MCF
        ["G--H", 20, "G", 700, "chr7:7000:+", "H", 800, "chr8:8000:-", "ONLY_REF_SPLICE",
         acc([("C%02d" % i, "U%02d" % i) for i in range(18)] + [("N%02d" % i, "V%02d" % i) for i in range(3)])],                      # 0.6 - 0.15 >= 0.3, 0.15 > 0.1 -> High_Non-Cancer_MCF
        ["I--J", 14, "I", 900, "chr9:9000:+", "J", 950, "chr10:9500:-", "ONLY_REF_SPLICE", acc(many_c + [("N05", "W1")])],             # 0.4 - 0.05, 0.05 <= 0.1 -> PASS with non-cancer
        ["K--L", 9, "K", 10, "chr11:10:+", "L", 20, "chr12:20:-", "INCL_NON_REF_SPLICE", acc(many_c)],                                # dropped: not ONLY_REF_SPLICE
        ["I--J", 12, "I", 901, "chr9:9001:+", "J", 951, "chr10:9501:-", "ONLY_REF_SPLICE", acc(many_c)],                              # I--J2: PASS
    ]


def barcodes_rows():
    return [("C%02d" % i, "Cancer") for i in range(30)] + [("N%02d" % i, "Non-Cancer") for i in range(20)] + [("XX", "Unknown")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("LONGSOM_REFERENCE", ""), help="root of the LongSom tree (holds workflow/scripts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fusion"))
    a = ap.parse_args()
    scripts = os.path.join(a.reference, "workflow", "scripts", "FusionCalling")
    if not os.path.exists(os.path.join(scripts, "BamToFastq.py")):
        sys.exit("give the LongSom tree with --reference (or LONGSOM_REFERENCE)")
    from longsom_amd import hostio
    from tests.support import fastq_cases as fc
    os.makedirs(a.out, exist_ok=True)
    ref = load_reference_script(os.path.join(scripts, "BamToFastq.py"))

    # ---- plain mode
    edge, _ = fc.edge_records()
    plain = [r for r in edge if len(r["seq"]) < 10000] + [r for r in fc.routed_records() if "CB" in r["tags"]]
    fc.write(os.path.join(a.out, "plain.bam"), plain)
    ref.bam_to_fastq(os.path.join(a.out, "plain.bam"), os.path.join(a.out, "plain.fastq"))

    # ---- the routed chain: split BAMs -> bam_to_fastq each -> cat in cell-type order
    fc.write(os.path.join(a.out, "routed.bam"), fc.routed_records())
    with open(os.path.join(a.out, "routed.meta.tsv"), "w") as f:
        f.write(fc.ROUTED_META)
    table = hostio.read_barcodes(os.path.join(a.out, "routed.meta.tsv"))
    for out_name, filters in (("routed.fastq", None), ("routed.nM2.fastq", hostio.SplitFilters(max_nM=2))):
        with tempfile.TemporaryDirectory() as tmp:
            bams = [os.path.join(tmp, ct + ".bam") for ct in table.celltype_names]
            hostio.split_bam(os.path.join(a.out, "routed.bam"), table, bams, 30, filters)
            with open(os.path.join(a.out, out_name), "wb") as cat:
                for b in bams:
                    ref.bam_to_fastq(b, b + ".fastq")
                    with open(b + ".fastq", "rb") as g:
                        shutil.copyfileobj(g, cat)

    # ---- SomaticFusions
    with open(os.path.join(a.out, "predictions.tsv"), "w") as f:
        f.write("\t".join(PREDICTIONS_HEADER) + "\n")
        for row in predictions_rows():
            f.write("\t".join(str(x) for x in row) + "\n")
    with open(os.path.join(a.out, "barcodes.tsv"), "w") as f:
        f.write("Index\tCell_type\n" + "".join("%s\t%s\n" % r for r in barcodes_rows()))
    subprocess.check_call([sys.executable, "-B", os.path.join(scripts, "FusionCalling.py"), "--fusions", os.path.join(a.out, "predictions.tsv"),
                           "--barcodes", os.path.join(a.out, "barcodes.tsv"), "--min_ac_reads", "3", "--min_ac_cells", "2", "--max_MCF_noncancer", "0.1",
                           "--deltaMCF", "0.3", "--outdir", os.path.join(a.out, "fusions")])
    for n in sorted(os.listdir(a.out)):
        print("%8d  %s" % (os.path.getsize(os.path.join(a.out, n)), n))


if __name__ == "__main__":
    main()
