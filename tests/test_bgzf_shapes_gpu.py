"""GPU: the device ingest (k_inflate, k_block_crc, k_chain / k_chain_fix of csrc/ingest.hip) on the BGZF shapes other writers leave and
the project's own two never do - stored and fixed-code blocks, Z_RLE and Z_HUFFMAN_ONLY streams, members of several DEFLATE blocks,
foreign extra subfields, members of 0, 1 .. 17 and 65 536 bytes, records that straddle every member, more members than the inflate
grid has lanes - and on damaged members.  Every file is the uncompressed stream of a committed golden or of a synthetic BAM, written
again by tests/support/bgzf.py (which tests/test_bgzf_shapes_cpu.py pins against gzip and the host decoder); every comparison is
equality: device arrays and count rows against the host decoder's (both_ways), and the host decoder's records for the re-blocked file
against those for the source."""
import os
import time

import numpy as np
import pytest

from longsom_amd import hostio, pipeline, synth, tsvio
from longsom_amd._lib import LsgError
from tests.support import bgzf
from tests.test_bgzf_shapes_cpu import assert_same_decode
from tests.test_ingest_gpu import both_ways, slices_add_up

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Source:
    """a BAM's uncompressed stream, what it takes to load it, the host decoder's answer for it - and its re-blocked files, each written once"""

    def __init__(self, folder, bam, barcodes, celltype_of, refs):
        self.folder, self.bam, self.barcodes, self.celltype_of, self.refs = folder, bam, barcodes, celltype_of, refs
        self.stream = bgzf.read_stream(bam)
        self.dec = hostio.decode_bam(bam, barcodes, min_mapq=60)
        _, self.lens, self.first = hostio.bam_header(bam)
        self._files = {}

    def write(self, name, raw):
        path = os.path.join(str(self.folder), name + ".bam")
        with open(path, "wb") as f:
            f.write(raw)
        self._files[name] = (path, raw)
        return path, raw

    def plan(self, name):
        """(path, bytes) of a named plan of tests/support/bgzf.py"""
        return self._files[name] if name in self._files else self.write(name, bgzf.plan(name, self.stream))

    def check(self, engine, path):
        """both_ways on `path`, and the host decoder's records for it == those for the source"""
        info, dec = both_ways(engine, path, self.barcodes, self.celltype_of, self.refs)
        assert_same_decode(dec, self.dec)
        assert info["n_ubytes"] == len(self.stream) and info["n_records"] == len(bgzf.record_offsets(self.stream)) - 1
        return info

    def load(self, engine, path):
        """a plain device load on the shared handle"""
        engine.set_contigs(self.lens); engine.set_barcodes(self.celltype_of, 2); engine.set_region()
        return engine.load_bam(path, self.barcodes, min_mapq=60, first_record_offset=self.first)[0]


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    bc = hostio.read_barcodes(os.path.join(G, "pileup.rand.barcodes.tsv"))
    _, seqs = tsvio.read_fasta(os.path.join(G, "pileup.rand.fa"))
    refs = [np.frombuffer(bytes(x), dtype=np.uint8) for x in seqs]
    return Source(tmp_path_factory.mktemp("golden"), os.path.join(G, "pileup.rand.bam"), bc.barcodes, bc.celltype_of, refs)


def synth_source(folder, n_reads):
    m = synth.named("C1", n_reads=n_reads)
    bam = os.path.join(str(folder), "src.bam")
    hostio.synth_bam(m, bam)
    refs = [hostio.ref_bases(m.seed, t, int(l)) for t, l in enumerate(m.contig_len)]
    return Source(folder, bam, hostio.synth_barcodes(m), m.celltype_of, refs)


@pytest.fixture(scope="module")
def c1(tmp_path_factory):
    return synth_source(tmp_path_factory.mktemp("c1"), 3000)


def test_patchwork(engine, golden):
    """150+ record-aligned members of ~1.5 KB, member i of shape i mod 7 (stored, fixed, level 1, level 9, Huffman only, RLE, four block
    types in one): the lanes of a wave decode different block types side by side; foreign subfields before and behind BC"""
    path, raw = golden.plan("patchwork")
    info = golden.check(engine, path)
    assert info["n_blocks"] == len(bgzf.members(raw)) >= 151 and info["chain_rounds"] <= 2


def test_full64k(engine, golden):
    """members of exactly 65 536 bytes: the only size with bit 16 of a length set (zero_ops[16], the last turn of crc_shift), all 64 lanes
    of the CRC wave with a full chunk"""
    path, raw = golden.plan("full64k")
    mem = bgzf.members(raw)
    info = golden.check(engine, path)
    assert info["n_blocks"] == len(mem) and sum(m[3] == 65536 for m in mem[:info["n_blocks"]]) >= 3


def test_edges(engine, golden):
    """members of 1 .. 17 bytes (the 8-byte stores' guards), of a CRC chunk and one byte less or more at odd offsets, an empty member in
    mid-file; the header and several records span members"""
    path, raw = golden.plan("edges")
    info = golden.check(engine, path)
    assert info["n_blocks"] == len(bgzf.members(raw))
    assert 2 <= info["chain_rounds"] <= info["n_blocks"] + 1


def test_unaligned4k(engine, golden, monkeypatch, tmp_path):
    """57 members of 4 096 bytes, every boundary inside a record: the chain settles a member a round; with fewer rounds allowed the device
    refuses (rc -4) and load_sample's auto mode hands the file to the host decoder"""
    path, raw = golden.plan("unaligned4k")
    info = golden.check(engine, path)
    assert info["n_blocks"] == len(bgzf.members(raw)) == 58
    assert 2 <= info["chain_rounds"] <= info["n_blocks"] + 1
    bct, fa = os.path.join(G, "pileup.rand.barcodes.tsv"), os.path.join(G, "pileup.rand.fa")

    def sample(ingest):
        res = pipeline.load_sample(path, bct, fa, engine, 60, ingest=ingest)
        return res, engine.pileup_count(), [engine.fetch_counts(ct) for ct in range(2)]
    res0, n0, rows0 = sample("auto")
    assert any(k.startswith("ingest_") for k in res0.seconds), "the device ingest did not take the file"
    monkeypatch.setenv("LSG_CHAIN_ROUNDS", "3")
    with pytest.raises(LsgError, match="straddle"):
        golden.load(engine, path)
    res1, n1, rows1 = sample("auto")
    assert not any(k.startswith("ingest_") for k in res1.seconds), "the device ingest took a file it had to refuse"
    assert res1.dec.report == res0.dec.report == golden.dec.report and n1 == n0
    np.testing.assert_array_equal(res1.dec.cb_pass, res0.dec.cb_pass); np.testing.assert_array_equal(res1.dec.cb_low, res0.dec.cb_low)
    for a, b in zip(rows0, rows1):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    with pytest.raises(LsgError, match="straddle"):
        pipeline.load_sample(path, bct, fa, engine, 60, ingest="device")
    monkeypatch.delenv("LSG_CHAIN_ROUNDS")
    golden.load(engine, golden.bam)                      # the handle is whole
    assert engine.reads_shape()[0] == 1333


@pytest.mark.parametrize("name", sorted(bgzf.UNIFORM))
@pytest.mark.parametrize("source", ["golden", "c1"])
def test_uniform(engine, request, source, name):
    """every member of one kind - stored blocks, fixed codes, Huffman only, RLE (matches at distance 1: the pattern path of the wide
    copy) - record-aligned at ~60 000 bytes"""
    src = request.getfixturevalue(source)
    path, raw = src.plan(name)
    info = src.check(engine, path)
    assert info["n_blocks"] == len(bgzf.members(raw)) and info["chain_rounds"] <= 2


def test_queue(engine, tmp_path):
    """more members than k_inflate's grid has lanes (64 lanes x 5 waves x CUs): the lanes take the rest off the block queue.  A record
    a member; stored, fixed and level-1 members in turn"""
    import torch
    lanes = 64 * 5 * torch.cuda.get_device_properties(0).multi_processor_count
    src = synth_source(tmp_path, lanes + 1500)
    t0 = time.time()
    path, raw = src.write("queue", bgzf.one_record_per_member(src.stream))
    print("queue: %d members written in %.1f s" % (lanes + 1502, time.time() - t0))
    info = src.check(engine, path)
    assert info["n_blocks"] == lanes + 1502 > lanes and info["chain_rounds"] <= 2


@pytest.mark.parametrize("name", ["patchwork", "edges"])
def test_slices(engine, golden, name):
    """the .bai's virtual offsets point into tiny, empty and foreign-subfield members: three slices add up to the whole"""
    path, _ = golden.plan(name)
    slices_add_up(engine, path, golden.barcodes, golden.celltype_of, golden.refs, 3)


@pytest.mark.parametrize("how", ["nlen", "isize-1", "isize+1", "type3", "crc"])
def test_refusals(engine, golden, how):
    """one member damaged: both decoders refuse the file, the device names the member, and the good file loads on the same handle"""
    if how == "crc":                                     # a wrong CRC32 behind a 65 536-byte member
        path, raw = golden.plan("full64k")
        index = [m[3] for m in bgzf.members(raw)].index(65536, 1)
        want = "CRC32 mismatch in BGZF block %d" % index
    else:                                                # member 70 of the patchwork: one stored block
        path, raw = golden.plan("patchwork")
        index, want = 70, "inflate failed in BGZF block 70"
    bad, _ = golden.write("bad_" + how, bgzf.damaged(raw, index, how))
    with pytest.raises(LsgError, match=want + r"\b"):
        golden.load(engine, bad)
    with pytest.raises(Exception, match="CRC32" if how == "crc" else "inflate failed"):
        hostio.decode_bam(bad, golden.barcodes, min_mapq=60)
    info = golden.load(engine, path)
    assert info["n_records"] == 1418 and engine.reads_shape()[0] == 1333
