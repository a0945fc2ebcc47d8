"""The BAMs the index tests share (tests/test_bai_cpu.py, tests/test_bai_gpu.py): the smallest shapes at which a .bai builder can go wrong.
Every case is a BAM file's bytes; records carry no sequence (l_seq = 0) unless a case is about their size, so the files stay small."""
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests.support import bamwrite, bgzf, longread_cases

BIG = 1 << 29
BARCODES = ["AAAC", "CCCA", "GGGT"]
CELLTYPE_OF = [0, 1, 0]
CELLTYPES = ["Cancer", "Non-Cancer"]


def rec(tid: int, pos: int, cigar: str = "10M", flag: int = 0, name: str = "r", k: int = 0, seq: str = "*") -> dict:
    """k picks the barcode (and with it the cell type a split sends the record to)"""
    return dict(tid=tid, pos=pos, cigar=cigar, flag=flag, name=name, seq=seq, qual=[30] * (0 if seq == "*" else len(seq)), mapq=60, tags={"CB": BARCODES[k % 3] + "-1"})


def stream_of(contigs: Sequence[Tuple[str, int]], records: Sequence[dict], text_pad: int = 0) -> bytes:
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs) + "".join("@CO\t%s\n" % ("x" * 100) for _ in range(text_pad))
    parts = [b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(contigs))]
    for name, ln in contigs:
        parts.append(struct.pack("<I", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", ln))
    for r in records:
        parts.append(bamwrite.encode_record(r["tid"], r["pos"], r["name"], r["flag"], r["mapq"], r["cigar"], r["seq"], r["qual"], r["tags"]))
    return b"".join(parts)


def on_records(stream: bytes, target: int = 0xFF00, extra_cuts: Sequence[int] = ()) -> bytes:
    """members that start on record boundaries, as htslib writes them (a header longer than a member is cut by size first)"""
    offs = bgzf.record_offsets(stream)
    head = list(range(target, offs[0], target)) + ([offs[0]] if len(offs) > 1 and offs[0] > target else [])
    cuts = sorted(set(head + bgzf.cuts_on_records(offs, target, head[-1] if head else 0) + list(extra_cuts)))
    return bgzf.reblock(stream, [c for c in cuts if 0 < c < len(stream)], lambda i: bgzf.level1)


def every(stream: bytes, size: int) -> bytes:
    """members of `size` bytes wherever the records are (a record longer than a member spans several)"""
    return bgzf.reblock(stream, bgzf.cuts_every(len(stream), size), lambda i: bgzf.level1)


def record_cut(stream: bytes, k: int) -> int:
    """the stream offset of record k: a member boundary to ask for"""
    return bgzf.record_offsets(stream)[k]


C1 = [("chr1", 1_000_000)]


def levels_records() -> List[dict]:
    """one read per bin level, the edges of §1 of the contract"""
    r = [rec(0, 0, "10M", name="pos0"), rec(0, 100, "5S3I5S", name="rlen0"), rec(0, 3 * 16384 - 10, "10M", name="ends_on_edge"),
         rec(0, 5 * 16384 - 5, "10M", name="x16k", k=1), rec(0, (1 << 17) * 3 - 5, "10M", name="x128k", k=1), rec(0, (1 << 20) * 2 - 5, "10M", name="x1M", k=2),
         rec(0, (1 << 23) - 5, "10M", name="x8M"), rec(0, (1 << 26) - 5, "10M", name="x64M", k=1), rec(0, BIG - 10, "10M", name="ends_at_2^29")]
    return sorted(r, key=lambda x: x["pos"])


def max_cigar_string() -> str:
    ops = longread_cases.max_cigar_ops(np.random.default_rng(5))
    assert len(ops) == 65535
    return "".join("%d%s" % (l, op) for op, l in ops)


def build_all() -> Dict[str, bytes]:
    """name -> the BAM file's bytes, every accepted case"""
    out: Dict[str, bytes] = {}
    three = [("chr1", 100_000), ("chr2", 50_000), ("chr3", 200_000)]
    unplaced = [rec(-1, -1, "*", 4, "u%d" % i, i) for i in range(5)]
    out["empty"] = on_records(stream_of(C1, []))
    out["all_unplaced"] = on_records(stream_of(C1, unplaced))
    out["middle_empty"] = on_records(stream_of(three, [rec(0, 10, k=0), rec(0, 10, "*", 4, "placed_unmapped", 1), rec(0, 20_000, "30M", k=2), rec(0, 20_005, "*", 4, "pu2", 0),
                                                       rec(2, 5, k=1), rec(2, 150_000, "100M2000N100M", k=0), rec(2, 150_000, "*", 0x4, "pu3", 2)] + unplaced))
    out["levels"] = on_records(stream_of([("big", BIG)], levels_records()))
    back = [rec(0, 100, name="a"), rec(0, 200, "20000M", name="wide", k=1), rec(0, 300, name="b")]
    s = stream_of(C1, back)
    out["bin_back_one_block"] = on_records(s)
    out["bin_back_two_blocks"] = on_records(s, extra_cuts=[record_cut(s, 2)])
    # 769 records in 513 runs over 513 bins and windows: 3 x 256 + 1 and 2 x 256 + 1, a second wave with one live lane in every kernel
    many = []
    for w in range(513):
        many.append(rec(0, w * 16384 + 7, "50M", name="m%d" % w, k=w))
        if w % 2 == 1:
            many.append(rec(0, w * 16384 + 9, "50M", flag=16, name="n%d" % w, k=w + 1))
    assert len(many) == 769
    out["many_bins"] = on_records(stream_of([("chr1", 513 * 16384 + 100)], many), target=3000)
    out["deep_window"] = on_records(stream_of(C1, [rec(0, 5000 + i, "50M", flag=(16 if i % 3 == 0 else 0) | (4 if i % 100 == 0 else 0), name="d%d" % i, k=i) for i in range(3000)]))
    longc = [rec(0, 1000 + 10 * i, name="s%d" % i, k=i) for i in range(70)]
    longc.insert(35, rec(0, 1345, max_cigar_string(), name="max_cigar", k=1))
    longc += [rec(0, 10 * 16384 - 50, "100M1200000N100M", name="spliced", k=2), rec(0, 10 * 16384 + 5, name="after", k=0)]
    s = stream_of([("chr1", 2_000_000)], longc)
    out["long_cigar"] = every(s, 0xFF00)                       # the 262 KB record spans five members, three of them without a record start
    big = [rec(0, 40 + 900 * i, "100M", name="q%d" % i, k=i, seq="ACGT" * 25) for i in range(12)]
    big.insert(6, rec(0, 40 + 900 * 5 + 1, "25S69950M25S", name="long.read", k=1, seq="ACGT" * 17500))
    out["oversize"] = every(stream_of(C1, big), 0xFF00)
    holes = [rec(0, 100 * i, name="h%d" % i, k=i) for i in range(40)]
    s = stream_of(C1, holes, text_pad=700)                     # a header of 70 KB: longer than a member
    assert bgzf.record_offsets(s)[0] > 65536
    c = [record_cut(s, 10), record_cut(s, 10), record_cut(s, 20), record_cut(s, 20), record_cut(s, 20), record_cut(s, 30)]     # empty members in mid-file
    offs0 = bgzf.record_offsets(s)[0]
    out["empty_members"] = bgzf.reblock(s, sorted([0xFF00, offs0] + c), lambda i: bgzf.level1)
    return out


def refused() -> Dict[str, Tuple[bytes, int, int]]:
    """name -> (the BAM file's bytes, the ordinal refused, the kind: 1 unsorted, 2 negative position, 3 beyond 2^29)"""
    two = [("chr1", 100_000), ("chr2", 100_000)]
    base = [rec(0, 100 * i, name="o%d" % i, k=i) for i in range(300)]                # (more than a wave and a workgroup before the bad record)
    out = {}
    out["pos_steps_back"] = (on_records(stream_of(two, base + [rec(0, 29_000, name="back"), rec(1, 5)])), 300, 1)
    out["ref_steps_back"] = (on_records(stream_of(two, base + [rec(1, 5), rec(0, 50_000, name="back")])), 301, 1)
    out["unplaced_first"] = (on_records(stream_of(two, base + [rec(-1, -1, "*", 4, "u"), rec(1, 5, name="late")])), 301, 1)
    out["negative_pos"] = (on_records(stream_of(two, base[:3] + [rec(1, -1, name="neg"), rec(1, 7)])), 3, 2)
    out["negative_pos_no_cigar"] = (on_records(stream_of(two, base[:3] + [rec(1, -1, "*", 4, "neg"), rec(1, 7)])), 3, 2)      # (one a split routes: no alignment to validate)
    out["beyond_2^29"] = (on_records(stream_of([("big", BIG + 1000)], levels_records() + [rec(0, BIG - 9, "10M", name="ends_at_2^29+1")])), 9, 3)
    return out


def split_table():
    from longsom_amd import hostio
    return hostio.BarcodeTable(list(BARCODES), np.asarray(CELLTYPE_OF, np.uint8), list(CELLTYPES))


_BUILT: Optional[Dict[str, bytes]] = None


def cases() -> Dict[str, bytes]:
    global _BUILT
    if _BUILT is None:
        _BUILT = build_all()
    return _BUILT


NAMES = ("empty", "all_unplaced", "middle_empty", "levels", "bin_back_one_block", "bin_back_two_blocks", "many_bins", "deep_window", "long_cigar", "oversize", "empty_members")
REFUSED_NAMES = ("pos_steps_back", "ref_steps_back", "unplaced_first", "negative_pos", "negative_pos_no_cigar", "beyond_2^29")
# the refused inputs a split routes into cell type 0's file (barcodes k % 3 in {0, 2}), where the index of that file refuses them:
# name -> (ordinal in that file, kind).  pos_steps_back: 200 of the 300 sorted records go there, then `back`.  ref_steps_back: the 200, the
# record on chr2, then `back`.  negative_pos_no_cigar: o0, o2, then `neg`.  beyond_2^29: pos0, rlen0, ends_on_edge, x1M, x8M, ends_at_2^29,
# then the read that ends at 2^29 + 1.  (unplaced_first: a split routes no unplaced record; negative_pos: lsg_split_bam's own validation
# refuses an aligned read at a negative position before any index is made)
SPLIT_REFUSED = {"pos_steps_back": (200, 1), "ref_steps_back": (201, 1), "negative_pos_no_cigar": (2, 2), "beyond_2^29": (6, 3)}
REFUSED_TEXT = {1: "not coordinate-sorted", 2: "negative position", 3: "beyond 2^29"}
