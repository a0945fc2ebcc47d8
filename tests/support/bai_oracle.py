"""The project's canonical .bai (SAM specification §5.2) restated in plain Python, sharing no code with
longsom_amd/csrc/bamindex_core.h: blocks inflated with zlib, records walked with struct, bins as a dict of lists, the merge a literal loop.
Also the brute-force answer to a region query, which the index's chunk lists must cover."""
import struct
import zlib
from typing import Dict, List, Optional, Tuple

UNSORTED, NEG_POS, TOO_FAR = 1, 2, 3


class Refused(Exception):
    def __init__(self, ordinal: int, kind: int):
        super().__init__("record %d refused (%d)" % (ordinal, kind))
        self.ordinal, self.kind = ordinal, kind


def _members(raw: bytes) -> List[Tuple[int, int, bytes]]:
    """(file offset, size in the file, uncompressed bytes) of every BGZF member"""
    out, off = [], 0
    while off < len(raw):
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        bsize, q = None, off + 12
        while q + 4 <= off + 12 + xlen:
            slen = struct.unpack_from("<H", raw, q + 2)[0]
            if raw[q:q + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", raw, q + 4)[0] + 1
            q += 4 + slen
        data = zlib.decompress(raw[off + 12 + xlen:off + bsize - 8], -15)
        assert len(data) == struct.unpack_from("<I", raw, off + bsize - 4)[0]
        out.append((off, bsize, data))
        off += bsize
    return out


class Records:
    """every record of a BAM: (tid, pos, end, unmapped, start virtual offset, end virtual offset); n_ref"""

    def __init__(self, raw: bytes):
        mem = [m for m in _members(raw) if m[2]]                       # an empty member is never pointed at
        stream = b"".join(m[2] for m in mem)
        ustart, u = [], 0
        for _, _, d in mem:
            ustart.append(u); u += len(d)

        def voff(g: int) -> int:
            k = max(i for i in range(len(ustart)) if ustart[i] <= g)
            return (mem[k][0] << 16) | (g - ustart[k])
        assert stream[:4] == b"BAM\x01"
        p = 8 + struct.unpack_from("<I", stream, 4)[0]
        self.n_ref = struct.unpack_from("<I", stream, p)[0]; p += 4
        for _ in range(self.n_ref):
            p += 8 + struct.unpack_from("<I", stream, p)[0]
        starts, facts = [], []
        while p < len(stream):
            bs = struct.unpack_from("<I", stream, p)[0]
            tid, pos, l_name, _mapq, _bin, n_cigar, flag = struct.unpack_from("<iiBBHHH", stream, p + 4)
            cig = struct.unpack_from("<%dI" % n_cigar, stream, p + 4 + 32 + l_name)
            rlen = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))
            starts.append(voff(p)); facts.append((tid, pos, pos + max(rlen, 1), bool(flag & 4)))
            p += 4 + bs
        eof = (mem[-1][0] + mem[-1][1]) << 16
        ends = starts[1:] + [eof]
        self.recs = [f + (s, e) for f, s, e in zip(facts, starts, ends)]

    def overlapping(self, tid: int, beg: int, end: int) -> List[int]:
        """ordinals of the records of tid whose interval meets [beg, end): brute force"""
        return [i for i, r in enumerate(self.recs) if r[0] == tid and r[1] < end and r[2] > beg]


def _bin_of(beg: int, end: int) -> int:
    last = end - 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == last >> shift:
            return first + (beg >> shift)
    return 0


def check(recs: Records) -> None:
    """raises Refused for the first record the contract refuses; of several reasons at one record the smallest kind"""
    prev = None
    for i, (tid, pos, end, _u, _s, _e) in enumerate(recs.recs):
        key = (1 << 62, 0) if tid < 0 else (tid, pos)
        if prev is not None and key < prev:
            raise Refused(i, UNSORTED)
        if tid >= 0 and pos < 0:
            raise Refused(i, NEG_POS)
        if tid >= 0 and end > (1 << 29):
            raise Refused(i, TOO_FAR)
        prev = key


def build(raw: bytes) -> bytes:
    """the .bai of a BAM file's bytes"""
    recs = Records(raw)
    check(recs)
    out = [b"BAI\x01", struct.pack("<i", recs.n_ref)]
    for r in range(recs.n_ref):
        mine = [x for x in recs.recs if x[0] == r]
        bins: Dict[int, List[List[int]]] = {}
        last_bin: Optional[int] = None
        for tid, pos, end, _u, s, e in mine:                          # runs: file-consecutive records of one bin
            b = _bin_of(pos, end)
            if b == last_bin:
                bins[b][-1][1] = e
            else:
                bins.setdefault(b, []).append([s, e])
            last_bin = b
        for b in bins:                                                 # the merge: a chunk that starts in the block where its neighbour ends
            merged: List[List[int]] = []
            for c in bins[b]:
                if merged and (merged[-1][1] >> 16) >= (c[0] >> 16):
                    merged[-1][1] = c[1]
                else:
                    merged.append(list(c))
            bins[b] = merged
        out.append(struct.pack("<i", len(bins) + (1 if mine else 0)))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])))
            for c in bins[b]:
                out.append(struct.pack("<QQ", c[0], c[1]))
        if mine:
            n_unm = sum(1 for x in mine if x[3])
            out.append(struct.pack("<IiQQQQ", 37450, 2, mine[0][4], mine[-1][5], len(mine) - n_unm, n_unm))
        n_intv = max(((x[2] - 1) >> 14) + 1 for x in mine) if mine else 0
        lin = [None] * n_intv
        for w in range(n_intv):
            over = [x[4] for x in mine if x[1] < ((w + 1) << 14) and x[2] > (w << 14)]
            lin[w] = min(over) if over else None
        first = next((v for v in lin if v is not None), None)
        for w in range(n_intv):
            if lin[w] is None:
                lin[w] = lin[w - 1] if w else first
        out.append(struct.pack("<i", n_intv))
        out.append(struct.pack("<%dQ" % n_intv, *lin))
    out.append(struct.pack("<Q", sum(1 for x in recs.recs if x[0] < 0)))
    return b"".join(out)
