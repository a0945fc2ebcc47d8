"""A BGZF re-blocker for tests: reads a BAM, and writes the SAME uncompressed stream again cut into other members, every member deflated
the way a plan says - stored, fixed or dynamic codes, Z_RLE / Z_HUFFMAN_ONLY streams, several DEFLATE blocks of different types in one
member, members of 0, 1 or 65 536 bytes, foreign extra subfields beside BC.  htslib with libdeflate, `samtools view -u` / `-1` and
`bgzip -@` write such shapes; the project's own two writers (tests/support/bamwrite.py, lsio_synth_bam) write none of them.
Pure Python + zlib: what it writes is checked against gzip and the host decoder by tests/test_bgzf_shapes_cpu.py."""
import bisect
import gzip
import struct
import zlib
from typing import Callable, List, Optional, Sequence, Tuple

Piece = Tuple[bytes, int, int]                    # (bytes, zlib level, zlib strategy): one raw-deflate stream of a member
DEFAULT, FIXED, HUFFMAN_ONLY, RLE = zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE
MAX_MEMBER = 65536                                # BSIZE is 16 bits (minus one), ISIZE of a BGZF member at most 2^16

# foreign subfields (RFC 1952 §2.3.1.1).  The first one's payload reads like a BC subfield: a reader has to WALK the subfields by their
# lengths (as htslib does), not search the extra field for "BC"
FOREIGN_BEFORE = b"LS" + struct.pack("<H", 6) + b"BC\x02\x00\xff\xff"
FOREIGN_AFTER = b"ZZ" + struct.pack("<H", 0) + b"Qx" + struct.pack("<H", 3) + b"\x00\x01\x02"


def read_stream(path: str) -> bytes:
    """the uncompressed stream of a BGZF file (gzip reads concatenated members)"""
    with open(path, "rb") as f:
        return gzip.decompress(f.read())


def record_offsets(stream: bytes) -> List[int]:
    """offsets of every BAM record in the uncompressed stream, walked by block_size from the first one, and the stream's end last"""
    assert stream[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<I", stream, 4)[0]
    n_ref = struct.unpack_from("<I", stream, p)[0]; p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<I", stream, p)[0]
    offs = []
    while p < len(stream):
        offs.append(p)
        p += 4 + struct.unpack_from("<I", stream, p)[0]
    assert p == len(stream), "the last record is cut"
    offs.append(p)
    return offs


def cuts_on_records(offs: Sequence[int], target: int, start: int = 0) -> List[int]:
    """cut offsets behind `start`, each on a record boundary (offs: record_offsets), members of at most `target` bytes where a record
    boundary allows it and of one record (or what is left of one) where none does"""
    cuts, pos, total = [], start, offs[-1]
    while True:
        k = bisect.bisect_right(offs, pos + target) - 1
        if k < 0 or offs[k] <= pos:
            k = bisect.bisect_right(offs, pos)
        if offs[k] >= total:
            return cuts
        cuts.append(offs[k]); pos = offs[k]


def cuts_every(total: int, size: int, start: int = 0) -> List[int]:
    return list(range(start + size, total, size))


def cuts_of_sizes(sizes: Sequence[int], start: int = 0) -> List[int]:
    cuts, pos = [], start
    for s in sizes:
        pos += s; cuts.append(pos)
    return cuts


def deflate_pieces(pieces: Sequence[Piece]) -> bytes:
    """the pieces as ONE raw DEFLATE stream: every piece a stream of its own, all but the last ended with a full flush (which leaves an
    empty stored block, not final, on a byte boundary), the last with a plain flush (its final block)"""
    out = []
    for i, (data, level, strategy) in enumerate(pieces):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        out.append(co.compress(data))
        if i + 1 < len(pieces):
            out.append(co.flush(zlib.Z_FULL_FLUSH))
        else:
            out.append(co.flush())
    return b"".join(out)


def member(payload: bytes, data: bytes, before: bytes = b"", after: bytes = b"") -> bytes:
    """one BGZF member around a raw-deflate payload of `data`"""
    xlen = len(before) + 6 + len(after)
    bsize = 12 + xlen + len(payload) + 8
    assert len(data) <= MAX_MEMBER and bsize <= 65536, "a BGZF member of %d bytes (%d uncompressed)" % (bsize, len(data))
    return (struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + before + b"BC" + struct.pack("<HH", 2, bsize - 1) + after + payload +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


EOF = member(b"\x03\x00", b"")                   # htslib's 28-byte end-of-file marker: an empty member


# ---- member shapes: data -> pieces
def stored(d: bytes) -> List[Piece]: return [(d, 0, DEFAULT)]
def fixed(d: bytes) -> List[Piece]: return [(d, 6, FIXED)]
def level1(d: bytes) -> List[Piece]: return [(d, 1, DEFAULT)]
def level6(d: bytes) -> List[Piece]: return [(d, 6, DEFAULT)]
def level9(d: bytes) -> List[Piece]: return [(d, 9, DEFAULT)]
def huffman_only(d: bytes) -> List[Piece]: return [(d, 6, HUFFMAN_ONLY)]
def rle(d: bytes) -> List[Piece]: return [(d, 6, RLE)]


def mixed(d: bytes) -> List[Piece]:
    """four DEFLATE block types in one member: dynamic codes, stored, fixed codes, an RLE stream"""
    q = len(d) // 4
    return [(d[:q], 6, DEFAULT), (d[q:2 * q], 0, DEFAULT), (d[2 * q:3 * q], 6, FIXED), (d[3 * q:], 6, RLE)]


PATCHWORK = (stored, fixed, level1, level9, huffman_only, rle, mixed)
Shape = Callable[[bytes], List[Piece]]


def reblock(stream: bytes, cuts: Sequence[int], shape_of: Callable[[int], Shape], extra_of: Optional[Callable[[int], Tuple[bytes, bytes]]] = None) -> bytes:
    """the stream as BGZF members [0, cuts[0]), [cuts[0], cuts[1]), ... and the empty EOF member; member i deflated as shape_of(i) says,
    with the foreign subfields extra_of(i) = (before BC, after BC)"""
    edges = [0] + list(cuts) + [len(stream)]
    assert all(a <= b for a, b in zip(edges, edges[1:])), "cuts out of order"
    out = []
    for i, (a, b) in enumerate(zip(edges, edges[1:])):
        data = stream[a:b]
        before, after = extra_of(i) if extra_of else (b"", b"")
        out.append(member(deflate_pieces(shape_of(i)(data)), data, before, after))
    out.append(EOF)
    return b"".join(out)


def members(raw: bytes) -> List[Tuple[int, int, int, int]]:
    """(offset, bsize, xlen, isize) of every member of a BGZF file, subfields walked by their lengths"""
    out, off = [], 0
    while off < len(raw):
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        bsize, q = None, off + 12
        while q + 4 <= off + 12 + xlen:
            slen = struct.unpack_from("<H", raw, q + 2)[0]
            if raw[q:q + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", raw, q + 4)[0] + 1
            q += 4 + slen
        assert bsize is not None
        out.append((off, bsize, xlen, struct.unpack_from("<I", raw, off + bsize - 4)[0]))
        off += bsize
    return out


# ---- the plans the shape tests share (tests/test_bgzf_shapes_cpu.py pins them on the host, tests/test_bgzf_shapes_gpu.py runs them)
EDGE_SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 1, 1023, 1024, 1025, 5, 2047, 2049, 0, 11, 4095, 4097, 13, 16383, 16385)
UNIFORM = {"stored": stored, "fixed": fixed, "huffman_only": huffman_only, "rle": rle}


def patchwork_extra(i: int) -> Tuple[bytes, bytes]:
    return (FOREIGN_BEFORE if i % 2 else b"", FOREIGN_AFTER if i % 3 == 0 else b"")


def plan(name: str, stream: bytes) -> bytes:
    """the re-blocked file of a named plan"""
    offs = record_offsets(stream)
    if name == "patchwork":          # >= 150 record-aligned members, neighbours of different DEFLATE types, foreign subfields
        return reblock(stream, cuts_on_records(offs, 1500), lambda i: PATCHWORK[i % 7], patchwork_extra)
    if name == "full64k":            # members of exactly 2^16 bytes, wherever the records are
        return reblock(stream, cuts_every(len(stream), 65536), lambda i: level9)
    if name == "edges":              # tiny members, every edge of the CRC's 1 KB chunks, an empty member in mid-file
        head = cuts_of_sizes(EDGE_SIZES)
        return reblock(stream, head + cuts_on_records(offs, 20000, head[-1]), lambda i: (level6, stored, fixed, rle)[i % 4])
    if name == "unaligned4k":        # every member boundary inside a record
        return reblock(stream, cuts_every(len(stream), 4096), lambda i: level6)
    if name in UNIFORM:
        return reblock(stream, cuts_on_records(offs, 60000), lambda i: UNIFORM[name])
    raise KeyError(name)


def _stored_member(data: bytes) -> bytes:
    """a member of one final stored block, without a compressobj (the queue plan writes tens of thousands)"""
    return member(b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data, data)


def one_record_per_member(stream: bytes, cycle: str = "sfsl") -> bytes:
    """the header, then every record in a member of its own; member types cycle through `cycle` (s: stored, f: fixed, l: level 1)"""
    offs = record_offsets(stream)
    edges = [0] + offs
    out = []
    n = len(cycle)
    for i, (a, b) in enumerate(zip(edges, edges[1:])):
        data = stream[a:b]
        kind = cycle[i % n]
        if kind == "s":
            out.append(_stored_member(data))
        else:
            co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, DEFAULT) if kind == "l" else zlib.compressobj(6, zlib.DEFLATED, -15, 8, FIXED)
            out.append(member(co.compress(data) + co.flush(), data))
    out.append(EOF)
    return b"".join(out)


# ---- damaged members (refusals both decoders are written to make)
def damaged(raw: bytes, index: int, how: str) -> bytes:
    """member `index` of a BGZF file with one thing wrong: "nlen" (its stored block's NLEN is not ~LEN), "isize-1" / "isize+1" (the
    trailer's ISIZE off by one), "type3" (the reserved block type), "crc" (another CRC32 in the trailer)"""
    off, bsize, xlen, isize = members(raw)[index]
    m = bytearray(raw[off:off + bsize])
    if how in ("isize-1", "isize+1"):
        m[-4:] = struct.pack("<I", isize + (1 if how == "isize+1" else -1))
    elif how == "crc":
        m[-8] ^= 0x10
    elif how == "nlen":
        assert m[12 + xlen] == 1 and struct.unpack_from("<H", m, 13 + xlen)[0] == isize, "not a member of one stored block"
        m[15 + xlen] ^= 0x01
    elif how == "type3":
        m[12 + xlen] = (m[12 + xlen] & 0xF8) | 0x07                                 # BFINAL = 1, BTYPE = 3
    else:
        raise KeyError(how)
    return raw[:off] + bytes(m) + raw[off + bsize:]
