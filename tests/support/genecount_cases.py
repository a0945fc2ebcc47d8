"""Hand-stated cases of the cell-by-gene read count (longsom_amd/genecounts.py, csrc/genecounts.hip): annotations as GTF text, reads as
blocks, and the matrix, tallies and file text they must give, written out by hand - nothing here is computed by the code under test.

A read is a dict: tid, cb (index into the case's barcodes, -1 = no listed barcode), blocks [(start0, len), ...], flag, mapq.  The same
reads come out as a ReadRecords (records) and as a BAM (write_bam), so that every way of loading them can be held to the same answer."""
import os
from typing import Dict, List

import numpy as np

from longsom_amd.engine import ReadRecords
from tests.support import bamwrite


def read(tid, cb, blocks, flag=0, mapq=60):
    return {"tid": tid, "cb": cb, "blocks": list(blocks), "flag": flag, "mapq": mapq}


def records(reads: List[dict]) -> ReadRecords:
    """coordinate-sorted ReadRecords; every event is 0 ('NA'): the gene count reads no event"""
    reads = sorted(reads, key=lambda r: (r["tid"], r["blocks"][0][0]))
    seg_read = [i for i, r in enumerate(reads) for _ in r["blocks"]]
    seg_start = [b[0] for r in reads for b in r["blocks"]]
    seg_len = np.asarray([b[1] for r in reads for b in r["blocks"]], np.int64)
    off = np.concatenate([[0], np.cumsum(seg_len)[:-1]]) if len(seg_len) else np.zeros(0, np.int64)
    return ReadRecords([r["tid"] for r in reads], [r["blocks"][0][0] for r in reads], [r["flag"] for r in reads], [r["mapq"] for r in reads],
                       [r["cb"] for r in reads], seg_read, seg_start, seg_len, off, np.zeros(int(seg_len.sum()), np.uint16))


def write_bam(path: str, contigs, reads: List[dict], barcodes: List[str]) -> None:
    """the same reads as a coordinate-sorted BAM: blocks -> M runs with N between them, CB = the barcode (an unlisted one for cb -1)"""
    import struct
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs)
    parts = [b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(contigs))]
    parts += [struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", ln) for n, ln in contigs]
    made = {}                                              # equal reads are encoded once (the wide case repeats one read 100 000 times)
    for r in sorted(reads, key=lambda r: (r["tid"], r["blocks"][0][0])):
        key = (r["tid"], r["cb"], r["flag"], r["mapq"], tuple(r["blocks"]))
        if key not in made:
            cigar, n, end = "", 0, None
            for s, l in r["blocks"]:
                if end is not None:
                    cigar += "%dN" % (s - end)
                cigar += "%dM" % l; n += l; end = s + l
            made[key] = bamwrite.encode_record(r["tid"], r["blocks"][0][0], "r", r["flag"], r["mapq"], cigar, "A" * n, [30] * n,
                                               {"CB": barcodes[r["cb"]] if r["cb"] >= 0 else "NOTLISTED"})
        parts.append(made[key])
    out = b"".join(parts)
    with open(path, "wb") as f:
        for i in range(0, len(out), 0xFF00):
            f.write(bamwrite._bgzf_block(out[i:i + 0xFF00]))
        f.write(bamwrite._bgzf_block(b""))


def write_meta(path: str, barcodes: List[str]) -> None:
    """the barcode table (Index, Cell_type) in the case's barcode order; alternating cell types"""
    with open(path, "w") as f:
        f.write("Index\tCell_type\n")
        for i, b in enumerate(barcodes):
            f.write("%s\t%s\n" % (b, "Cancer" if i % 2 else "Non-Cancer"))


def write_gtf(path: str, text: str) -> None:
    with open(path, "w") as f:
        f.write(text)


def _gene(contig, gid, attrs):
    return "%s\thand\tgene\t1\t2\t.\t+\t.\tgene_id \"%s\"; %s\n" % (contig, gid, attrs)


def _exon(contig, gid, start, end, strand="+"):
    return "%s\thand\texon\t%d\t%d\t.\t%s\t.\tgene_id \"%s\"; transcript_id \"%s.1\";\n" % (contig, start, end, strand, gid, gid)


# ---- the main case -----------------------------------------------------------------------------------------------------------------
# BAM contigs: chr1 (1000), chr2 (500), chr3 (300, no gene).  The GTF also has chrX, which the BAM lacks: its one exon is dropped.
# Exons, 1-based inclusive as the GTF states them -> [start0, end0):
#   GF "First"  chr1 [1,10]     -> [0,10)        the first interval of the table
#   GA "Alpha"  chr1 [101,200]  -> [100,200)     chr1 [301,400] -> [300,400)       (an earlier gene line names it "Old": the later one wins)
#   GB "Beta"   chr1 [151,250]  -> [150,250)     shares [150,200) with GA: that interval is ambiguous
#   GC "Gamma"  chr1 [501,520] [511,530] [521,540] [531,560]   -> elementary [500,510) [510,520) [520,530) [530,540) [540,560): five of one gene
#   GD (no gene line: no name)  chr1 [601,650] -> [600,650)
#   GE1, GE2 both "Dup"         chr1 [701,720] -> [700,720), [741,760] -> [740,760)
#   GH "Hotel"  chr2 [1,20]     -> [0,20)        the next contig's first exon at position 0
#   GL "Last"   chr2 [401,450]  -> [400,450)     the last interval of the table
#   GX "Xray"   chrX [1,100]    dropped (a row of zeros: the gene id is known)
# Under --gene_names gene_name GF is "Foxtrot" (its third attribute, what the default rule takes, says "First").
MAIN_CONTIGS = [("chr1", 1000), ("chr2", 500), ("chr3", 300)]
MAIN_GTF = (
    "##description: hand-made\n##provider: tests\n##contact: nobody\n##format: gtf\n##date: today\n"
    + _gene("chr1", "GA", 'gene_type "pc"; gene_name "Old";')
    + _gene("chr1", "GF", 'gene_type "pc"; transcript_name "First"; gene_name "Foxtrot";')
    + _exon("chr1", "GF", 1, 10)
    + _gene("chr1", "GA", 'gene_type "pc"; gene_name "Alpha";')
    + _exon("chr1", "GA", 101, 200) + _exon("chr1", "GA", 301, 400, "-")
    + _gene("chr1", "GB", 'gene_type "pc"; gene_name "Beta";')
    + _exon("chr1", "GB", 151, 250, "-")
    + _gene("chr1", "GC", 'gene_type "lncRNA"; gene_name "Gamma";')
    + _exon("chr1", "GC", 501, 520) + _exon("chr1", "GC", 511, 530) + _exon("chr1", "GC", 521, 540) + _exon("chr1", "GC", 531, 560)
    + _exon("chr1", "GD", 601, 650)
    + _gene("chr1", "GE1", 'gene_type "pc"; gene_name "Dup";') + _gene("chr1", "GE2", 'gene_type "pc"; gene_name "Dup";')
    + _exon("chr1", "GE1", 701, 720) + _exon("chr1", "GE2", 741, 760)
    + "chr1\thand\ttranscript\t701\t760\t.\t+\t.\tgene_id \"GE1\";\n"
    + _gene("chr2", "GH", 'gene_type "pc"; gene_name "Hotel";') + _exon("chr2", "GH", 1, 20)
    + _gene("chr2", "GL", 'gene_type "pc"; gene_name "Last";') + _exon("chr2", "GL", 401, 450)
    + _gene("chrX", "GX", 'gene_type "pc"; gene_name "Xray";') + _exon("chrX", "GX", 1, 100)
)
MAIN_GENE_IDS = ["GF", "GA", "GB", "GC", "GD", "GE1", "GE2", "GH", "GL", "GX"]      # order of first appearance among the exon lines
# the flattening, by hand: (tid, start0, len, gene id or "*" for ambiguous)
MAIN_INTERVALS = [(0, 0, 10, "GF"), (0, 100, 50, "GA"), (0, 150, 50, "*"), (0, 200, 50, "GB"), (0, 300, 100, "GA"),
                  (0, 500, 10, "GC"), (0, 510, 10, "GC"), (0, 520, 10, "GC"), (0, 530, 10, "GC"), (0, 540, 20, "GC"),
                  (0, 600, 50, "GD"), (0, 700, 20, "GE1"), (0, 740, 20, "GE2"), (1, 0, 20, "GH"), (1, 400, 50, "GL")]
MAIN_BARCODES = ["TTTT", "AAAC", "CCCC", "GGGG"]          # ids 0..3; the columns are AAAC, CCCC, GGGG, TTTT; GGGG has no read
MAIN_READS = [
    # barcode 0 (TTTT)
    read(0, 0, [(290, 11)]),                  # touches GA's second exon by its first base (300) alone          Assigned Alpha
    read(0, 0, [(399, 11)]),                  # ... by its last base (399) alone                                 Assigned Alpha
    read(0, 0, [(290, 10)]),                  # ends at 299: misses it by one                                    NoFeatures
    read(0, 0, [(400, 10)]),                  # starts at 400: misses it by one                                  NoFeatures
    read(0, 0, [(260, 30)]),                  # inside GA's intron, past GB's end                                NoFeatures
    read(0, 0, [(495, 70)]),                  # spans the five elementary intervals of GC                        Assigned Gamma
    read(0, 0, [(100, 20), (210, 20)]),       # one block in GA, one in GB                                       Ambiguity
    read(0, 0, [(160, 10)]),                  # inside the interval GA and GB share                              Ambiguity
    # barcode 1 (AAAC)
    read(0, 1, [(610, 10)]),                  # GD alone: assigned, and in no row of the file                    Assigned (GD)
    read(0, 1, [(305, 5), (610, 10)]),        # GA and the unnamed GD                                            Ambiguity
    read(0, 1, [(705, 5)]),                   # GE1                                                              Assigned Dup
    read(0, 1, [(745, 5)]),                   # GE2: the same row                                                Assigned Dup
    read(0, 1, [(0, 5)]),                     # the first interval of the table                                  Assigned First
    read(1, 1, [(440, 20)]),                  # the last interval of the table                                   Assigned Last
    read(0, 1, [(990, 10)]),                  # ends at chr1's last base; chr2's first exon starts at 0          NoFeatures
    read(1, 1, [(0, 10)]),                    # that exon                                                        Assigned Hotel
    read(2, 1, [(10, 40)]),                   # a contig without a gene                                          NoFeatures
    # barcode 2 (CCCC)
    read(0, 2, [(300 + 2 * i, 2) for i in range(70)]),      # 70 segments, [300, 440): GA or nothing              Assigned Alpha
    read(0, 2, [(310, 10)], mapq=5),          # MAPQ 5                                                           Assigned Alpha / Filtered under --min_MQ 10
    read(0, 2, [(320, 10)], flag=0x100),      # secondary                                                        Assigned Alpha / Filtered under --primary_only
    read(0, 2, [(220, 10)], flag=0x810),      # supplementary, reverse strand                                    Assigned Beta / Filtered under --primary_only
    # no listed barcode
    read(0, -1, [(310, 10)]),                 # counted nowhere
]
MAIN_ROWS = ["Alpha", "Beta", "Dup", "First", "Gamma", "Hotel", "Last", "Xray"]
MAIN_TEXT = (b"Geneid,AAAC,CCCC,GGGG,TTTT\n"
             b"Alpha,0,3,0,2\n"
             b"Beta,0,1,0,0\n"
             b"Dup,2,0,0,0\n"
             b"First,1,0,0,0\n"
             b"Gamma,0,0,0,1\n"
             b"Hotel,1,0,0,0\n"
             b"Last,1,0,0,0\n"
             b"Xray,0,0,0,0\n")
# tallies per barcode id (TTTT, AAAC, CCCC, GGGG): Assigned, NoFeatures, Ambiguity, Filtered
MAIN_TALLIES = [[3, 3, 2, 0], [6, 2, 1, 0], [4, 0, 0, 0], [0, 0, 0, 0]]
MAIN_SUMMARY = (b"Status\tAAAC\tCCCC\tGGGG\tTTTT\n"
                b"Assigned\t6\t4\t0\t3\n"
                b"NoFeatures\t2\t0\t0\t3\n"
                b"Ambiguity\t1\t0\t0\t2\n"
                b"Filtered\t0\t0\t0\t0\n")


def _case(name, contigs, gtf, barcodes, reads, rows, text, tallies, min_mapq=0, primary_only=False, gene_names="third", tsv=False, n_dropped_exons=0):
    return dict(name=name, contigs=contigs, gtf=gtf, barcodes=barcodes, reads=reads, rows=rows, text=text, tallies=np.asarray(tallies, np.int64),
                min_mapq=min_mapq, primary_only=primary_only, flag_exclude=0x904 if primary_only else 0x4, gene_names=gene_names, tsv=tsv,
                n_dropped_exons=n_dropped_exons)


def _main(name, text=MAIN_TEXT, tallies=MAIN_TALLIES, rows=MAIN_ROWS, **kw):
    return _case(name, MAIN_CONTIGS, MAIN_GTF, MAIN_BARCODES, MAIN_READS, rows, text, tallies, n_dropped_exons=1, **kw)


# ---- 130 barcodes, one row, every digit width --------------------------------------------------------------------------------------
# One gene "Solo" (chr1 [1,100] -> [0,100)); barcode id i is "BC%03d" % (129 - i), so the columns are the ids backwards.  130 columns:
# the last wave of the row holds two.  Counts of 0, 9, 10, 99 and 100 000 stand side by side.
WIDE_BARCODES = ["BC%03d" % (129 - i) for i in range(130)]
WIDE_COUNTS: Dict[str, int] = {"BC001": 9, "BC002": 10, "BC003": 99, "BC004": 100000, "BC063": 7, "BC064": 1234, "BC128": 12, "BC129": 1}
WIDE_GTF = _gene("chr1", "G1", 'gene_type "pc"; gene_name "Solo";') + _exon("chr1", "G1", 1, 100)
WIDE_READS = [read(0, 129 - int(b[2:]), [(10, 10)]) for b, n in sorted(WIDE_COUNTS.items()) for _ in range(n)]
_wide_names = ["BC%03d" % i for i in range(130)]
WIDE_TEXT = (",".join(["Geneid"] + _wide_names) + "\n" + ",".join(["Solo"] + [str(WIDE_COUNTS.get(b, 0)) for b in _wide_names]) + "\n").encode()
assert WIDE_TEXT.startswith(b"Geneid,BC000,BC001,BC002,BC003,BC004,BC005,") and b"\nSolo,0,9,10,99,100000,0," in WIDE_TEXT and WIDE_TEXT.endswith(b",12,1\n")
WIDE_TALLIES = [[WIDE_COUNTS.get(b, 0), 0, 0, 0] for b in WIDE_BARCODES]


HAND_CASES = [
    _main("main"),
    _main("main_min_mq_10", min_mapq=10,
          text=MAIN_TEXT.replace(b"Alpha,0,3,0,2", b"Alpha,0,2,0,2"), tallies=[[3, 3, 2, 0], [6, 2, 1, 0], [3, 0, 0, 1], [0, 0, 0, 0]]),
    _main("main_primary_only", primary_only=True,
          text=MAIN_TEXT.replace(b"Alpha,0,3,0,2", b"Alpha,0,2,0,2").replace(b"Beta,0,1,0,0", b"Beta,0,0,0,0"), tallies=[[3, 3, 2, 0], [6, 2, 1, 0], [2, 0, 0, 2], [0, 0, 0, 0]]),
    _main("main_tsv", tsv=True, text=MAIN_TEXT.replace(b",", b"\t")),
    _main("main_gene_name", gene_names="gene_name", rows=["Alpha", "Beta", "Dup", "Foxtrot", "Gamma", "Hotel", "Last", "Xray"], text=MAIN_TEXT.replace(b"First", b"Foxtrot")),
    _main("main_ids", gene_names="none", rows=["GA", "GB", "GC", "GD", "GE1", "GE2", "GF", "GH", "GL", "GX"],
          text=(b"Geneid,AAAC,CCCC,GGGG,TTTT\nGA,0,3,0,2\nGB,0,1,0,0\nGC,0,0,0,1\nGD,1,0,0,0\nGE1,1,0,0,0\nGE2,1,0,0,0\nGF,1,0,0,0\nGH,1,0,0,0\nGL,1,0,0,0\nGX,0,0,0,0\n")),
    _case("wide_one_row", [("chr1", 1000)], WIDE_GTF, WIDE_BARCODES, WIDE_READS, ["Solo"], WIDE_TEXT, WIDE_TALLIES),
]


# ---- the seeded fuzz case ------------------------------------------------------------------------------------------------------------
FUZZ_CONTIGS = [("c1", 200000), ("c2", 150000), ("c3", 100000)]
FUZZ_MIN_MAPQ, FUZZ_FLAG_EXCLUDE = 10, 0x904


def fuzz_case(seed: int = 20260101):
    """20 000 reads of 1 to 12 segments, 300 genes on 3 contigs with overlapping genes, 130 barcodes; reads below the MAPQ limit, secondary
    records and reads without a listed barcode among them.  Returns dict(contigs, gtf, exons [(gene index, tid, start0, end0)], n_genes,
    gene_ids, barcodes, reads)."""
    rng = np.random.default_rng(seed)
    exons, lines, gene_ids = [], [], []
    for g in range(300):
        tid = g % 3
        gid = "ENSG%05d" % g
        gene_ids.append(gid)
        at = int(rng.integers(0, FUZZ_CONTIGS[tid][1] - 6000))
        lines.append(_gene(FUZZ_CONTIGS[tid][0], gid, 'gene_type "pc"; gene_name "N%d";' % (g // 2 if g % 7 == 0 else g)) if g % 11 else "")      # every 11th: no name; some share one
        for _ in range(int(rng.integers(1, 5))):
            ln = int(rng.integers(50, 400))
            exons.append((g, tid, at, at + ln)); lines.append(_exon(FUZZ_CONTIGS[tid][0], gid, at + 1, at + ln))
            at += ln + int(rng.integers(-100, 1000))           # (a negative gap: exons of one gene may overlap each other)
            at = max(at, 0)
    barcodes = ["CB%04d" % int(v) for v in rng.permutation(130)]
    reads = []
    for _ in range(20000):
        tid = int(rng.integers(0, 3))
        at = int(rng.integers(0, FUZZ_CONTIGS[tid][1] - 12 * 800))
        blocks = []
        for _ in range(int(rng.integers(1, 13))):
            ln = int(rng.integers(20, 200)); blocks.append((at, ln)); at += ln + int(rng.integers(50, 600))
        u = rng.random()
        reads.append(read(tid, -1 if rng.random() < 0.04 else int(rng.integers(0, 130)), blocks, flag=0x100 if u < 0.03 else 0x800 if u < 0.05 else 16 if u < 0.5 else 0,
                          mapq=int(rng.integers(0, 10)) if rng.random() < 0.04 else 60))
    return dict(contigs=FUZZ_CONTIGS, gtf="".join(lines), exons=exons, n_genes=300, gene_ids=gene_ids, barcodes=barcodes, reads=reads)


def paths(tmp, case_name):
    d = os.path.join(str(tmp), case_name)
    os.makedirs(d, exist_ok=True)
    return {k: os.path.join(d, k2) for k, k2 in (("bam", "reads.bam"), ("meta", "barcodes.tsv"), ("gtf", "anno.gtf"), ("out", "out"))}
