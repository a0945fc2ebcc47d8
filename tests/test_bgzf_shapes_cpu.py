"""CPU: the BGZF re-blocker of the shape tests (tests/support/bgzf.py) and the host decoder on what it writes.  Every plan that
tests/test_bgzf_shapes_gpu.py puts through the device ingest is, here, (1) valid gzip that yields the source's uncompressed stream,
(2) decoded by hostio.decode_bam - zlib's inflate, the GPU tests' reference - to exactly what the source file decodes to, (3) indexable."""
import gzip
import os
import zlib

import numpy as np
import pytest

from longsom_amd import hostio, synth
from longsom_amd.engine import ReadRecords
from tests.support import bgzf

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_PLANS = ["patchwork", "full64k", "edges", "unaligned4k", "stored", "fixed", "huffman_only", "rle"]


def assert_same_decode(a, b):
    assert a.report == b.report and a.contig_names == b.contig_names
    np.testing.assert_array_equal(a.contig_len, b.contig_len)
    np.testing.assert_array_equal(a.cb_pass, b.cb_pass); np.testing.assert_array_equal(a.cb_low, b.cb_low)
    for name, _ in ReadRecords._SPEC:
        np.testing.assert_array_equal(getattr(a.records, name), getattr(b.records, name), err_msg=name)


@pytest.fixture(scope="module")
def golden():
    src = os.path.join(G, "pileup.rand.bam")
    bc = hostio.read_barcodes(os.path.join(G, "pileup.rand.barcodes.tsv"))
    return bgzf.read_stream(src), bc.barcodes, hostio.decode_bam(src, bc.barcodes, min_mapq=60)


@pytest.fixture(scope="module")
def c1(tmp_path_factory):
    m = synth.named("C1", n_reads=3000)
    src = str(tmp_path_factory.mktemp("c1") / "c1.bam")
    hostio.synth_bam(m, src)
    barcodes = hostio.synth_barcodes(m)
    return bgzf.read_stream(src), barcodes, hostio.decode_bam(src, barcodes, min_mapq=60)


def check(tmp_path, raw, source):
    stream, barcodes, want = source
    assert gzip.decompress(raw) == stream
    assert raw.endswith(bgzf.EOF) and len(bgzf.EOF) == 28, "no empty EOF member"
    p = str(tmp_path / "x.bam")
    with open(p, "wb") as f:
        f.write(raw)
    assert hostio.bam_header(p)[2] == bgzf.record_offsets(stream)[0]
    assert_same_decode(hostio.decode_bam(p, barcodes, min_mapq=60), want)
    assert len(hostio.read_bai(hostio.build_bai(p))) > 0


def test_the_golden_source_has_the_records_the_plans_are_sized_for(golden):
    stream = golden[0]
    offs = bgzf.record_offsets(stream)
    sizes = np.diff(offs)
    assert (len(stream), offs[0], len(offs) - 1, int(sizes.min()), int(sizes.max())) == (231853, 172, 1418, 57, 337)


@pytest.mark.parametrize("name", GOLDEN_PLANS)
def test_golden_plans(tmp_path, golden, name):
    raw = bgzf.plan(name, golden[0])
    mem = bgzf.members(raw)[:-1]
    isize = [m[3] for m in mem]
    assert sum(isize) == len(golden[0])
    if name == "patchwork":
        assert len(mem) >= 150
        assert {m[2] for m in mem} == {6, 6 + len(bgzf.FOREIGN_BEFORE), 6 + len(bgzf.FOREIGN_AFTER), 6 + len(bgzf.FOREIGN_BEFORE) + len(bgzf.FOREIGN_AFTER)}
    elif name == "full64k":
        assert isize.count(65536) >= 3
    elif name == "edges":
        assert tuple(isize[:len(bgzf.EDGE_SIZES)]) == bgzf.EDGE_SIZES and 0 in isize
    elif name == "unaligned4k":
        assert len(mem) == 57 and set(isize[:-1]) == {4096}
    check(tmp_path, raw, golden)


def _block_types(payload):
    """the BTYPE of every DEFLATE block of a raw stream whose blocks are stored (walked here) - enough for the stored plan"""
    types, p = [], 0
    while True:
        types.append((payload[p] >> 1) & 3)
        if types[-1] != 0:
            return types
        n = int.from_bytes(payload[p + 1:p + 3], "little")
        last = payload[p] & 1
        p += 5 + n
        if last:
            return types


def test_the_plans_hold_the_block_types_they_name(golden):
    """zlib is asked for a strategy; what the device decoder has to see is the DEFLATE block type in the stream"""
    stream = golden[0]
    for name, want in (("stored", 0), ("fixed", 1), ("huffman_only", 2), ("rle", 2)):
        raw = bgzf.plan(name, stream)
        for off, bsize, xlen, isize in bgzf.members(raw)[:-1]:
            payload = raw[off + 12 + xlen:off + bsize - 8]
            if want == 0:
                assert set(_block_types(payload)) == {0}
            else:
                assert (payload[0] >> 1) & 3 == want
    # a mixed member: its pieces start with a dynamic (or, for so few bytes, fixed), a stored, a fixed and again a dynamic (or fixed) block
    pieces = bgzf.mixed(stream[172:1672])
    starts = [(bgzf.deflate_pieces([p])[0] >> 1) & 3 for p in pieces]
    assert starts[0] in (1, 2) and starts[1:3] == [0, 1] and starts[3] in (1, 2), starts
    assert zlib.decompress(bgzf.deflate_pieces(pieces), -15) == stream[172:1672]


@pytest.mark.parametrize("name", sorted(bgzf.UNIFORM))
def test_uniform_plans_on_a_synthetic_bam(tmp_path, c1, name):
    check(tmp_path, bgzf.plan(name, c1[0]), c1)


def test_one_record_per_member(tmp_path, c1):
    """the shape of the GPU suite's queue test, at 3 000 records"""
    raw = bgzf.one_record_per_member(c1[0])
    assert len(bgzf.members(raw)) == 3000 + 2
    check(tmp_path, raw, c1)


@pytest.mark.parametrize("how", ["nlen", "isize-1", "isize+1", "type3", "crc"])
def test_the_host_decoder_refuses_a_damaged_member(tmp_path, golden, how):
    stream, barcodes, _ = golden
    raw = bgzf.plan("patchwork", stream)
    bad = bgzf.damaged(raw, 70, how)
    assert bad != raw and len(bad) == len(raw)
    p = str(tmp_path / "bad.bam")
    with open(p, "wb") as f:
        f.write(bad)
    with pytest.raises(Exception, match="CRC32" if how == "crc" else "inflate failed"):
        hostio.decode_bam(p, barcodes, min_mapq=60)
