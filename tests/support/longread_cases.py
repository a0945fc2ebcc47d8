"""One BAM of long-read-shaped records (PacBio / ONT: what the product is for), seeded, written once per test session.

80 records: four families of 20 copies, over 20 barcodes of alternating cell types.
  max_cigar    65 535 CIGAR operations (n_cigar at its 16-bit maximum): M / = / X of 1-3 between I or D of 1-2, now and then P before I,
               D then I, and 1D2D.  The record is 400 KB: with bamwrite's cut at 0xFF00 it spans 7-8 BGZF members, the middle ones
               holding no record start.  Its reference span is 97 kb (match blocks of 1-3 between 32 767 separators give no more).
  long_match   30000S 120000M 5S: a segment of 1 876 tiles with two or three window edges strictly inside it.  The pileup windows are
               [1 + k W, 1 + (k + 1) W) in 0-based columns, W = 50 000 (store.hip win_edge_after, plp_oracle.c).  Copy 4 starts on a
               window's first column (50 001), copy 1 ends on a window's last (200 000: pos 80 001); copy 0 starts at 50 000, the last
               column of window 0 - one column in that window, three edges inside; the others start at even and odd offsets, the last
               four late enough to reach into the window behind 200 000, where max_cigar's columns are its own.
  many_exons   400 match blocks of 20-199 between N of 50-2 999 (neighbouring segments share a tile), one intron of 600 000 behind the
               fifteenth block; copies 2, 9 and 16 carry N followed by I at seven introns.
  long_indels  chrM from position 0 to its last base: 50M 10000D 40M 5000I 5910M.
Per family: odd copies are reverse strand, copy 3 is supplementary (0x800), copy 6 secondary (0x100), copy 11 has MAPQ 20, copy 14 has
no CB: eight countable reads per family and cell type.  Copies c and c + 2 of a group of four start on the same position (and, by the
barcode rule, in the same cell type): htslib's depth cap only ever drops a read that is not the first of its start position.

Where the families lie.  In file order: long_match (chr1 50 000-206 000), max_cigar (from 155 000), many_exons (from 225 000 to the
contig's last 100 kb), long_indels (chrM).  Each overlaps the next, so a depth cap of 8 meets up to seventeen reads of a cell type
in one window's pileup (tests/test_longread_cpu.py looks at each family where its columns are its own: `alone`); and no read
that starts early reaches far: a read of 1.2 Mb at the head of the file would pin the .bai's linear index to its own offset in every
window it spans, and regions.BaiPlan could then cut chr1 nowhere.  As laid out, a cut by compressed bytes falls on the first 16 kb window
that max_cigar no longer reaches - inside many_exons' long intron (tests/test_longread_cpu.py asserts it), so the slice's guessed end
stops short and regions.ingest_slice guesses again.  (What runs again is its check of the guess on the host, _last_key_of_block; the
repeat of the device ingest behind it - info["last_key"] short of the region's end after a load - is reached by no file here.)
Qualities: 90 % in 30-60, the rest in 2-29.  Bases: the reference with 2 % random mismatches, a few N and IUPAC letters."""
import os
from typing import Dict, List, Tuple

import numpy as np

from tests.support import bamwrite

SEED = 20261021
CONTIGS = [("chr1", 1_600_000), ("chrM", 16_000)]
N_COPIES = 20
BARCODES = ["LRCELL%04dGT" % i for i in range(20)]
CELLTYPE_OF = (np.arange(20) % 2).astype(np.uint8)
FAMILIES = ("max_cigar", "long_match", "many_exons", "long_indels")
WINDOW = 50_000
MAX_CIGAR_OPS = 65_535
LONG_INTRON = 600_000
LONG_INTRON_AFTER = 14                                        # the block (0-based) the long intron follows
LONG_INDELS_CIGAR = [("M", 50), ("D", 10_000), ("M", 40), ("I", 5_000), ("M", 5_910)]
_OPS = "MIDNSHP=X"
_REF_OPS = np.array([c in "MDN=X" for c in _OPS])
_QRY_OPS = np.array([c in "MIS=X" for c in _OPS])
_ALN_OPS = np.array([c in "M=X" for c in _OPS])
_NT = np.frombuffer(b"ACGT", np.uint8)


def reference(rng, length: int) -> np.ndarray:
    """upper-case ACGT with a few short runs of N"""
    s = _NT[rng.integers(0, 4, length)].copy()
    for p in rng.integers(0, length - 4, length // 3000):
        s[int(p):int(p) + int(rng.integers(1, 4))] = ord("N")
    return s


def max_cigar_ops(rng) -> List[Tuple[str, int]]:
    """exactly 65 535 operations, a match block first and last"""
    ops: List[Tuple[str, int]] = []
    while True:
        ops.append(("M" if rng.random() < 0.8 else ("=" if rng.random() < 0.5 else "X"), min(3, int(rng.integers(1, 5)))))      # 1, 2, 3, 3
        left = MAX_CIGAR_OPS - len(ops)
        if left == 0:
            return ops
        # a separator of one or two operations; what is left after it must end on a match block: never exactly two before one
        r = rng.random()
        two = left == 3 or (left > 4 and r < 0.12)
        if two:
            ops += ([("P", 1), ("I", int(rng.integers(1, 3)))] if r < 0.04 else [("D", int(rng.integers(1, 3))), ("I", 1)] if r < 0.08 else [("D", 1), ("D", 2)])
        else:
            ops.append(("I" if r < 0.56 else "D", int(rng.integers(1, 3))))


def many_exons_ops(rng) -> List[Tuple[str, int]]:
    ops: List[Tuple[str, int]] = []
    for b in range(400):
        ops.append(("M", int(rng.integers(20, 200))))
        if b < 399:
            ops.append(("N", LONG_INTRON if b == LONG_INTRON_AFTER else int(rng.integers(50, 3000))))
    return ops


def ref_len(ops) -> int:
    return sum(l for op, l in ops if op in "MDN=X")


def make_read(rng, ref: np.ndarray, tid: int, pos: int, ops, flag: int, mapq: int, cb, name: str) -> dict:
    """the record as bamwrite.write_bam takes it; the sequence is drawn for all bases at once (a 150 000-base read is one numpy pass)"""
    code = np.array([_OPS.index(op) for op, _ in ops]); ln = np.array([l for _, l in ops], np.int64)
    r_at = np.cumsum(np.where(_REF_OPS[code], ln, 0)) - np.where(_REF_OPS[code], ln, 0)        # reference offset at which an operation begins
    q = np.flatnonzero(_QRY_OPS[code])
    op_of = np.repeat(q, ln[q])                                                                  # per query base: its operation
    within = np.arange(len(op_of)) - np.repeat(np.cumsum(ln[q]) - ln[q], ln[q])
    aligned = _ALN_OPS[code[op_of]]
    seq = _NT[rng.integers(0, 4, len(op_of))].copy()
    seq[aligned] = ref[pos + r_at[op_of[aligned]] + within[aligned]]
    u = rng.random(len(seq))
    seq = np.where(u < 0.02, _NT[rng.integers(0, 4, len(seq))], seq)
    seq = np.where((u >= 0.02) & (u < 0.023), ord("N"), seq)
    seq = np.where((u >= 0.023) & (u < 0.025), np.frombuffer(b"RYKM", np.uint8)[rng.integers(0, 4, len(seq))], seq).astype(np.uint8)
    qual = np.where(rng.random(len(seq)) < 0.9, rng.integers(30, 61, len(seq)), rng.integers(2, 30, len(seq))).astype(np.uint8)
    return dict(tid=tid, pos=pos, cigar="".join("%d%s" % (l, op) for op, l in ops), seq=seq.tobytes().decode(), qual=qual, flag=flag, mapq=mapq,
                tags={} if cb is None else {"CB": cb}, name=name, ref_len=int(np.where(_REF_OPS[code], ln, 0).sum()))


class LongReadCase:
    """contigs, lens, refs (uint8 per contig), barcodes, celltype_of, reads (sorted, as written), by_family {name: [read, ...] in copy order},
    spans {name: (tid, first column, last column + 1) over the family's copies}"""

    def __init__(self, seed: int = SEED):
        rng = np.random.default_rng(seed)
        self.contigs = CONTIGS
        self.lens = [l for _, l in CONTIGS]
        self.refs = [reference(rng, l) for l in self.lens]
        self.barcodes, self.celltype_of = BARCODES, CELLTYPE_OF
        cig = {"max_cigar": max_cigar_ops(rng), "long_match": [("S", 30_000), ("M", 120_000), ("S", 5)],
               "many_exons": many_exons_ops(rng), "long_indels": LONG_INDELS_CIGAR}
        exons_i = list(cig["many_exons"])
        for k in range(len(exons_i) - 1, -1, -1):                                                # the same blocks, N followed by I at seven introns
            if exons_i[k][0] == "N" and (k // 2) % 57 == 5:
                exons_i.insert(k + 1, ("I", 3))
        self.cigars = dict(cig, many_exons_n_then_i=exons_i)
        self.by_family: Dict[str, List[dict]] = {}
        for f, fam in enumerate(FAMILIES):
            out = []
            for c in range(N_COPIES):
                ops = cig[fam]
                step = c // 4 * 2 + c % 2                                                        # copies c and c + 2 of a group of four share a start
                if fam == "max_cigar":
                    pos = 155_000 + 197 * step
                elif fam == "long_match":
                    pos = 50_000 if c in (0, 2) else 4 * WINDOW + 1 - 120_000 if c in (1, 3) else WINDOW + 1 if c in (4, 6) else 50_000 + 4_000 * step + step % 2
                elif fam == "many_exons":
                    pos = 225_000 + 3 * step
                    if c in (2, 9, 16):
                        ops = exons_i
                else:
                    pos = 0
                flag = (0x10 if c % 2 else 0) | (0x800 if c == 3 else 0) | (0x100 if c == 6 else 0)
                tid = 1 if fam == "long_indels" else 0
                assert pos + ref_len(ops) <= self.lens[tid], fam
                out.append(make_read(rng, self.refs[tid], tid, pos, ops, flag, 20 if c == 11 else 60,
                                     None if c == 14 else BARCODES[(c + 5 * f) % 20], "%s.%02d" % (fam, c)))
                out[-1]["family"] = fam
            self.by_family[fam] = out
        self.reads = sorted((r for fam in FAMILIES for r in self.by_family[fam]), key=lambda r: (r["tid"], r["pos"]))
        self.spans = {fam: (rs[0]["tid"], min(r["pos"] for r in rs), max(r["pos"] + r["ref_len"] for r in rs)) for fam, rs in self.by_family.items()}
        # where only one family has columns: long_match before max_cigar begins, max_cigar between long_match's end and many_exons' start,
        # many_exons behind max_cigar's end (its last 1.5 kb before the long intron, and everything behind it)
        sp = self.spans
        self.alone = {"long_match": (0, sp["long_match"][1], sp["max_cigar"][1]), "max_cigar": (0, sp["long_match"][2], sp["many_exons"][1]),
                      "many_exons": (0, sp["max_cigar"][2], sp["many_exons"][2]), "long_indels": sp["long_indels"]}
        # ... and where two overlap (the only places a cap of 8 can bite: eight countable reads per family and cell type)
        self.shared = {"long_match+max_cigar": (0, sp["max_cigar"][1], sp["long_match"][2]), "max_cigar+many_exons": (0, sp["many_exons"][1], sp["max_cigar"][2])}
        self.bam = None

    def long_introns(self) -> List[Tuple[int, int]]:
        """[first column, last column + 1) of the 600 000-base intron of every many_exons copy"""
        before = 0
        for op, l in self.cigars["many_exons"]:
            if (op, l) == ("N", LONG_INTRON):
                break
            before += l
        return [(r["pos"] + before, r["pos"] + before + LONG_INTRON) for r in self.by_family["many_exons"]]

    def write(self, directory: str) -> str:
        self.bam = os.path.join(str(directory), "longread.bam")
        bamwrite.write_bam(self.bam, self.contigs, self.reads)
        return self.bam

    def decoded(self, min_mapq: int = 60):
        """the host decoder's record arrays (hostio.decode_bam): with lens, refs, celltype_of what tests/test_count_gpu.run_both takes"""
        from longsom_amd import hostio
        return hostio.decode_bam(self.bam, self.barcodes, min_mapq=min_mapq)

    @staticmethod
    def inside(keys: np.ndarray, stretch) -> np.ndarray:
        """mask of the row keys (tid << 32 | pos0) inside stretch = (tid, first column, last column + 1)"""
        tid, a, b = stretch
        return (keys >= ((tid << 32) | a)) & (keys < ((tid << 32) | b))


_MADE: Dict[int, LongReadCase] = {}


def written(tmp_path_factory, seed: int = SEED) -> LongReadCase:
    """the case with its BAM on disk: generated and written once a process (the Python writer is the slow part), whichever module asks first"""
    case = _MADE.get(seed)
    if case is None or not os.path.exists(case.bam):
        case = LongReadCase(seed)
        case.write(tmp_path_factory.mktemp("longread"))
        _MADE[seed] = case
    return case
