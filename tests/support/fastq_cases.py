"""Hand-authored BAMs for the FASTQ printer (csrc/fastq.hip, hostio lsio_bam_fastq) and the text they must print.

Every case names its record's fields in plain text (name, bases, qualities, tags) and, written by hand beside them, the header line
`CB^UMI^name` BamToFastq.py:24-37 gives it; the SEQ and QUAL lines are the case's own bases and qualities + 33 (the SAM text of the
record, SAM spec 1.4 / 4.2.3-4.2.4), never anything read back from a BAM.  tests/support/bamwrite.py packs the records."""
import random
from typing import List, Optional, Tuple

from tests.support import bamwrite

NT16 = "=ACMGRSVTWYHKDBN"
CONTIGS = [("chr1", 400000), ("chr2", 90000)]


def bases(n: int, shift: int = 0) -> str:
    """n bases cycling through all 16 codes"""
    return "".join(NT16[(i + shift) % 16] for i in range(n))


def quals(n: int, shift: int = 0) -> List[int]:
    """n qualities cycling through 0, 93 and values between"""
    cyc = [0, 93, 1, 40, 92, 2, 60, 13, 33]
    return [cyc[(i + shift) % len(cyc)] for i in range(n)]


def two_fields(first: str, tag: str, second: str) -> str:
    """a Z value that makes bamwrite emit TWO aux fields: `first`, then a field `tag`:Z:`second` (its NUL and tag bytes ride in the value)"""
    return first + "\0" + tag + "Z" + second


# (name, number of bases, has qualities, tags, mapped, the header line written by hand)
EDGE = [
    ("r", 0, True, {"CB": "AAAC-1", "UB": "UMI0", "nM": 0}, True, "AAAC^UMI0^r"),                         # no SEQ: '*' and '*'
    ("ab", 1, True, {"CB": "AAAC-2", "nM": 5}, True, "AAAC-2^NA^ab"),                                      # "-2" stays; no dot, no UB: NA
    ("a.b", 2, True, {"CB": "AAAC-1-1"}, True, "AAAC-1^^a.b"),                                    # one "-1" goes; field 'a' shorter than 3: empty
    ("abcd", 7, True, {"CB": "-1"}, True, "^NA^abcd"),                                            # "-1" alone: empty barcode
    ("abc.d", 8, True, {"nM": 2, "CB": "GGGT-1"}, True, "GGGT^^abc.d"),                                    # field 'abc' exactly 3: empty
    ("abcdef", 9, True, {"CB": "GGGT-1", "UB": "TTTT"}, True, "GGGT^TTTT^abcdef"),
    ("abcdefg", 63, True, {"CB": two_fields("FIRST-1", "CB", "SECOND-1"), "nM": 1}, True, "FIRST^NA^abcdefg"),      # two CB fields: the first
    ("x.abcd.z", 64, True, {"CB": "GGGT-1"}, True, "GGGT^a^x.abcd.z"),                            # second-to-last field 'abcd' minus 3
    ("abcdefghi", 65, False, {"CB": "GGGT-1", "UB": ""}, True, "GGGT^^abcdefghi"),                # 0xFF qualities: '*'; an empty UB is a UMI
    ("mol.ACGTACGTxyz.1", 513, True, {"CB": "CCCA-1"}, True, "CCCA^ACGTACGT^mol.ACGTACGTxyz.1"),
    ("long.read", 70000, True, {"xx": 7, "CB": "CCCA-1", "UB": two_fields("U1", "UB", "U2"), "nM": 1}, True, "CCCA^U1^long.read"),      # longer than a BGZF block
    ("un.mapped.q", 33, True, {"CB": "TTTG-1"}, False, "TTTG^map^un.mapped.q"),                   # tid -1: printed in plain mode
]


# Routed mode over the edge cases: the cleaned LAST CB:Z routes (the load's rule), the FIRST CB prints.  "" is what "-1" cleans to and
# SECOND is the second CB field of 'abcdefg'.  Cell type 0: GGGT, CCCA (the 70 000-base read) and ""; cell type 1: AAAC, TTTG, SECOND.
# Some records carry nM (0, 5, 2, 1, 1), the others none: under --max_nM 2 'r' and 'abcdefg' (type 1), 'abc.d' and 'long.read' (type 0) stay.
EDGE_BARCODES = ["AAAC", "GGGT", "CCCA", "TTTG", "SECOND", ""]
EDGE_CELLTYPE_OF = [1, 0, 0, 1, 1, 0]
EDGE_ROUTED = {None: (["abcd", "abc.d", "abcdef", "x.abcd.z", "abcdefghi", "mol.ACGTACGTxyz.1", "long.read"], ["r", "ab", "a.b", "abcdefg"]),
               2: (["abc.d", "long.read"], ["r", "abcdefg"])}      # max_nM -> the names printed per cell type, in file order; 'un.mapped.q' never


def record(name: str, n: int, has_qual: bool, tags: dict, mapped: bool, pos: int, shift: int = 0, mapq: int = 60) -> dict:
    return {"tid": 0 if mapped else -1, "pos": pos if mapped else -1, "name": name, "flag": 0 if mapped else 4, "mapq": mapq,
            "cigar": "%dM" % n if mapped and n else "*", "seq": bases(n, shift) if n else "*", "qual": quals(n, shift) if has_qual else [], "tags": tags}


def text_of(header: str, n: int, has_qual: bool, shift: int = 0) -> str:
    seq = bases(n, shift) if n else "*"
    qual = "".join(chr(q + 33) for q in quals(n, shift)) if n and has_qual else "*"
    return "@%s\n%s\n+\n%s\n" % (header, seq, qual)


def edge_records() -> Tuple[List[dict], str]:
    """the edge-case BAM's records and its FASTQ text"""
    recs, text = [], ""
    for k, (name, n, hq, tags, mapped, header) in enumerate(EDGE):
        recs.append(record(name, n, hq, tags, mapped, 100 + 10 * k, shift=k))
        text += text_of(header, n, hq, shift=k)
    return recs, text


def edge_routed_text(max_nm: Optional[int]) -> Tuple[str, List[int]]:
    """routed mode over the edge-case BAM with EDGE_BARCODES under --max_nM: the text (cell type 0's records, then cell type 1's) and the
    records printed per cell type, from EDGE_ROUTED's hand-written lists"""
    by_name = {c[0]: (k, c) for k, c in enumerate(EDGE)}
    text = ""
    for names in EDGE_ROUTED[max_nm]:
        for nm in names:
            k, (_, n, hq, _tags, _mapped, header) = by_name[nm]
            text += text_of(header, n, hq, shift=k)
    return text, [len(names) for names in EDGE_ROUTED[max_nm]]


def bad_records(kind: str) -> Tuple[List[dict], int]:
    """a BAM the printers must refuse, and the ordinal they must name: 'no_cb' = good records, a record without CB at ordinal 3, a CB:i
    record behind it; 'cb_type' = a CB:i record at ordinal 5, a record without CB behind it; 'ub_type' = a UB:i record at ordinal 2; 'nm_type' / 'nh_type' (routed mode
    over EDGE_BARCODES with that limit set) = a listed read with nM:Z / NH:Z at ordinal 4 behind an unlisted one with the same tag"""
    good, _ = edge_records()
    no_cb = record("nocb", 5, True, {"UB": "U"}, True, 90)
    cb_i = record("cbint", 5, True, {"CB": 12}, True, 95)
    ub_i = record("ubint", 5, True, {"CB": "AAAC-1", "UB": 3}, True, 97)
    if kind in ("nm_type", "nh_type"):      # routed mode under --max_nM / --max_NH: a listed read whose tag is a string, at ordinal 4; its low
        tag = "nM" if kind == "nm_type" else "NH"      # MAPQ does not hide it (the reference compares the tag before it tests MAPQ)
        bad = record("tagstr", 5, True, {"CB": "GGGT-1", tag: "two"}, True, 96, mapq=0)
        unlisted = record("elsewhere", 5, True, {"CB": "ZZZZ-1", tag: "two"}, True, 94)      # routed nowhere: not an error
        return good[:3] + [unlisted, bad] + good[3:], 4
    if kind == "no_cb":
        return good[:3] + [no_cb] + good[3:6] + [cb_i] + good[6:], 3
    if kind == "cb_type":
        return good[:5] + [cb_i] + good[5:7] + [no_cb] + good[7:], 5
    return good[:2] + [ub_i] + good[2:], 2


def write(path: str, records: List[dict]) -> None:
    bamwrite.write_bam(path, CONTIGS, records)


# ---- routed mode: two cell types, an unlisted barcode, a read below min_MQ, a read without CB, an unmapped read, nM tags ------------------
ROUTED_META = "Index\tCell_type\nAAAC-1\tNon-Cancer\nGGGT-1\tCancer\nCCCA-1\tCancer\nTTTG-1\tNon-Cancer\n"


def routed_records() -> List[dict]:
    spec = [("n1.AAAAxyz.1", 40, {"CB": "AAAC-1", "nM": 0}, True, 60), ("c1", 70, {"CB": "GGGT-1", "UB": "U1", "nM": 3}, True, 60),
            ("c2.lowq", 30, {"CB": "CCCA-1", "nM": 0}, True, 10), ("unlisted", 30, {"CB": "ZZZZ-1", "nM": 0}, True, 60),
            ("nocb", 30, {"nM": 0}, True, 60), ("c3", 17, {"CB": "CCCA-1", "nM": 1}, True, 60), ("n2", 16, {"CB": "TTTG-1"}, True, 60),
            ("c4.TTTTTabc.9", 1500, {"CB": "GGGT-1", "nM": 0}, True, 60), ("n3", 0, {"CB": "AAAC-1", "nM": 0}, True, 60),
            ("un", 20, {"CB": "GGGT-1", "nM": 0}, False, 60)]
    return [record(name, n, True, tags, mapped, 500 + 7 * k, shift=k, mapq=mq) for k, (name, n, tags, mapped, mq) in enumerate(spec)]


# ---- a seeded fuzz: random lengths, names, tags; bamwrite cuts blocks at 0xFF00, so records straddle blocks ---------------------------------
FUZZ_BARCODES = ["AAAC", "GGGT", "CCCA", "TTTG", "ACAC", "GTGT"]
FUZZ_CELLTYPE_OF = [0, 1, 1, 0, 1, 0]


def fuzz_records(n_records: int = 3000, max_len: int = 5000, seed: int = 20261019) -> List[dict]:
    rng = random.Random(seed)
    alphabet = "abcXYZ019._:-"
    out = []
    for k in range(n_records):
        n = rng.choice([0, 1, 15, 16, 17, 31]) if rng.random() < 0.1 else rng.randint(0, max_len)
        name = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 40)))
        tags = {}
        if rng.random() < 0.3:
            tags["xx"] = rng.randint(-5, 5)
        cb = rng.choice(FUZZ_BARCODES + ["NNNN"]) + rng.choice(["", "-1", "-2", "-1-1"])
        tags["CB"] = cb if rng.random() < 0.9 else two_fields(cb, "CB", "OTHER-1")
        if rng.random() < 0.5:
            tags["UB"] = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 12)))
        if rng.random() < 0.7:
            tags["nM"] = rng.randint(0, 4)
        mapped = rng.random() < 0.9
        out.append(record(name, n, rng.random() < 0.9, tags, mapped, 10 * k, shift=rng.randint(0, 100), mapq=rng.choice([0, 10, 60, 255])))
    return out
