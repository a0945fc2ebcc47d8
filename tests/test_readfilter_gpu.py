"""GPU: SplitBamCellTypes' read filters (--max_nM, --max_NH, --n_trim; SplitBamCellTypes.py:92-173) in the device ingest (ingest.hip
k_rec_info / k_rec_emit, lsg_set_split_filters) and through every ingest form of run_snv, against what the reference's own split_bam +
BaseCellCounter wrote for tests/golden/readfilter.bam (tools/make_readfilter_goldens.py).  The host side: tests/test_readfilter_cpu.py."""
import os
import shutil
import socket
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from longsom_amd import hostio, pipeline, synth, tsvio
from longsom_amd._lib import CountParams
from tests.util import assert_same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SETTINGS = {"nm": (5, None, 0), "nh": (None, 1, 0), "trim": (None, None, 5), "all": (5, 1, 5)}     # tools/make_readfilter_goldens.py
BAM, FA, BC = (os.path.join(G, "readfilter." + x) for x in ("bam", "fa", "barcodes.tsv"))


def golden_report(name):
    head, row = open(os.path.join(G, "readfilter.%s.report.txt" % name)).read().rstrip("\n").split("\n")
    return head, row


def golden_table(name, ct):
    p = os.path.join(G, "readfilter.%s.%s.tsv" % (name, ct))
    return open(p).read() if os.path.exists(p) else None


def no_date(text):
    return "".join(l for l in text.splitlines(True) if not l.startswith("##fileDate="))


def rows_text(text):
    return [l for l in text.splitlines(True) if l.strip() and not l.startswith("#")]


def check_outputs(out, name):
    """the report file (Total_time apart) and both count tables equal the reference's"""
    head, row = golden_report(name)
    h, r = open(out.report).read().rstrip("\n").split("\n")
    assert h.split("\t")[-1] == "Total_time"
    assert "\t".join(h.split("\t")[:-1]) == head and "\t".join(r.split("\t")[:-1]) == row
    for ct in ("Cancer", "Non-Cancer"):
        want, got = golden_table(name, ct), no_date(open(out.counts[ct]).read())
        if want is None:                                 # the reference writes no table for a cell type without a row
            assert not rows_text(got), ct
        else:
            assert got == want, ct


@pytest.mark.parametrize("ingest", ["device", "host"])
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_ingest_gives_the_reference_tables_and_report(engine, name, ingest):
    filt = hostio.SplitFilters(*SETTINGS[name])
    res = pipeline.load_sample(BAM, BC, FA, engine, 60, ingest=ingest, filters=filt)
    head, row = golden_report(name)
    assert list(res.dec.report) == head.split("\t") and [str(v) for v in res.dec.report.values()] == row.split("\t")
    engine.pileup_count(CountParams.longsom_defaults())
    for ct, cname in enumerate(res.table.celltype_names):
        k, r, c = engine.fetch_counts(ct)
        want = golden_table(name, cname)
        got = None if len(k) == 0 else no_date(tsvio.format_counts_tsv(k, r, c, res.contig_names, "s." + cname, "##fileDate=x\n"))
        assert got == want, cname
    assert engine.load_settings()["split_filters"] == (-1, -1, 0)      # load_sample puts the engine's filters back


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_run_snv_writes_the_reference_report_and_tables(tmp_path, name):
    out = pipeline.run_snv(BAM, BC, FA, str(tmp_path), "s", filters=hostio.SplitFilters(*SETTINGS[name]))
    check_outputs(out, name)


@pytest.mark.parametrize("index", [False, True])
def test_windowed_runs_write_the_reference_outputs(tmp_path, index):
    """--window_gb over the fixture: host-decoded batches (no index) or device-ingested slices (with one)"""
    bam = str(tmp_path / "s.bam")
    shutil.copy(BAM, bam)
    if index:
        hostio.build_bai(bam)
    out = pipeline.run_snv(bam, BC, FA, str(tmp_path / "out"), "s", filters=hostio.SplitFilters(5, 1, 5), window_bytes=20_000)
    check_outputs(out, "all")


@pytest.fixture(scope="module")
def tagged(tmp_path_factory):
    """a 60 k-read synthetic BAM (many BGZF blocks, htslib's block cuts) with random nM / NH tags, its .bai, and the whole-file run's report"""
    d = tmp_path_factory.mktemp("tagged")
    bam, fa, bct = str(d / "s.bam"), str(d / "ref.fa"), str(d / "bc.tsv")
    m = write_tagged_bam(d, 60_000, bam, fa, bct)
    hostio.build_bai(bam)
    whole = pipeline.run_snv(bam, bct, fa, str(d / "whole"), "s", filters=hostio.SplitFilters(5, 1, 3))
    return bam, fa, bct, open(whole.report).read().split("\n"), m


def same_report(path, want):
    got = open(path).read().split("\n")
    assert got[0] == want[0] and got[1].split("\t")[:-1] == want[1].split("\t")[:-1]
    assert len(got[0].split("\t")) > 12                  # (many reasons, their columns in first-seen order)


@pytest.mark.parametrize("index", [False, True])
def test_windows_of_a_tagged_bam_merge_to_the_whole_report(tagged, tmp_path, index):
    bam0, fa, bct, want, _ = tagged
    bam = str(tmp_path / "s.bam")
    shutil.copy(bam0, bam)
    if index:
        shutil.copy(bam0 + ".bai", bam + ".bai")
    out = pipeline.run_snv(bam, bct, fa, str(tmp_path / "out"), "s", filters=hostio.SplitFilters(5, 1, 3), window_bytes=2_000_000)
    assert out.timings["windows"] >= 2
    same_report(out.report, want)


def test_ranks_of_a_tagged_bam_merge_to_the_whole_report(tagged, tmp_path):
    bam, fa, bct, want, _ = tagged
    out_dir = str(tmp_path / "ranks")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, LSG_DIST_BACKEND="gloo", LSG_DIST_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "workflow", "scripts_gpu", "SNVCalling", "longsom_gpu_snv.py"), "--bam", bam, "--meta", bct, "--ref", fa, "--id", "s",
           "--outdir", out_dir, "--max_nM", "5", "--max_NH", "1", "--n_trim", "3"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert '"ranks": 2' in r.stdout and '"ingest_records_by_rank"' in r.stdout
    same_report(os.path.join(out_dir, "SplitBam", "s.report.txt"), want)


@pytest.mark.parametrize("index", [False, True])
def test_two_ranks_write_the_same_report(tmp_path, index):
    """2 ranks on one GPU over gloo: with an index every rank ingests its slice and the reasons are merged in (rank, ordinal) order;
    without one every rank ingests the whole file"""
    bam = str(tmp_path / "s.bam")
    shutil.copy(BAM, bam)
    if index:
        hostio.build_bai(bam)
    out_dir = str(tmp_path / "ranks")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, LSG_DIST_BACKEND="gloo", LSG_DIST_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "workflow", "scripts_gpu", "SNVCalling", "longsom_gpu_snv.py"), "--bam", bam, "--meta", BC, "--ref", FA, "--id", "s",
           "--outdir", out_dir, "--max_nM", "5", "--max_NH", "1", "--n_trim", "5"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert '"ranks": 2' in r.stdout
    out = pipeline.SnvOutputs(report=os.path.join(out_dir, "SplitBam", "s.report.txt"), counts={
        ct: os.path.join(out_dir, "BaseCellCounter", "s", "s.%s.tsv" % ct) for ct in ("Cancer", "Non-Cancer")}, merged="", step1="", step2="", step3="",
        step3_unfiltered="")
    check_outputs(out, "all")


def test_filters_off_outputs_are_byte_identical(tmp_path):
    """SplitFilters() (every filter off) is a run that never called the new entry points: every output file, byte for byte"""
    a = pipeline.run_snv(os.path.join(G, "pileup.rand.bam"), os.path.join(G, "pileup.rand.barcodes.tsv"), os.path.join(G, "pileup.rand.fa"), str(tmp_path / "a"), "s")
    b = pipeline.run_snv(os.path.join(G, "pileup.rand.bam"), os.path.join(G, "pileup.rand.barcodes.tsv"), os.path.join(G, "pileup.rand.fa"), str(tmp_path / "b"), "s",
                         filters=hostio.SplitFilters())
    for f in [*a.counts.values(), a.merged, a.step1, a.step2, a.step3]:
        g = f.replace(str(tmp_path / "a"), str(tmp_path / "b"))
        assert no_date(open(f).read()) == no_date(open(g).read()), f
    ra, rb = (open(x.report).read().split("\n") for x in (a, b))
    assert ra[0] == rb[0] and ra[1].split("\t")[:-1] == rb[1].split("\t")[:-1]


def _records(path):
    raw, d, off = open(path, "rb").read(), bytearray(), 0
    while off + 18 <= len(raw):
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        d += zlib.decompress(raw[off + 12 + xlen:off + bsize - 8], -15)
        off += bsize
    d = bytes(d)
    p = 8 + struct.unpack_from("<I", d, 4)[0]
    n_ref = struct.unpack_from("<I", d, p)[0]; p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<I", d, p)[0] + 4
    header, recs = d[:p], []
    while p + 4 <= len(d):
        bs = struct.unpack_from("<I", d, p)[0]
        recs.append(d[p + 4:p + 4 + bs]); p += 4 + bs
    return header, recs


def _bgzf(data):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    z = c.compress(data) + c.flush()
    return (struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, 6) + b"BC" + struct.pack("<HH", 2, len(z) + 25) + z +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_tagged_bam(d, n_reads, bam, fa, bct):
    """the synthetic model's reads with random nM / NH tags of every integer type (or none, or the tag twice), BGZF blocks cut as htslib cuts them"""
    m = synth.named("C1", n_reads=n_reads)
    src = str(d / "src.bam")
    hostio.synth_bam(m, src, fa)
    hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
    header, recs = _records(src)
    rng = np.random.default_rng(7)
    kinds = rng.integers(0, 8, size=(len(recs), 2)); vals = rng.integers(0, 4, size=(len(recs), 2)); nm_vals = rng.integers(0, 9, size=len(recs))
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
    out, block = [], bytearray(header)
    for i, rec in enumerate(recs):
        aux = b""
        for t, (name, v) in enumerate((("nM", int(nm_vals[i])), ("NH", int(vals[i, 1]) if vals[i, 1] else 1))):
            k = int(kinds[i, t])
            if k < 6:
                ty = "cCsSiI"[k]
                aux += name.encode() + ty.encode() + struct.pack(fmt[ty], v)
            elif k == 6:                                   # the tag twice: the first occurrence counts
                aux += name.encode() + b"C" + struct.pack("<B", v) + name.encode() + b"C" + struct.pack("<B", 9 - min(v, 9))
        l_name, n_cigar, l_seq = rec[8], struct.unpack_from("<H", rec, 12)[0], struct.unpack_from("<I", rec, 16)[0]
        at = 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
        rest = rec[at:]
        if rest.startswith(b"NHC\x01"):                  # (the generator's own NH:C:1 goes: the random tags replace it)
            rest = rest[4:]
        body = rec[:at] + aux + rest
        r = struct.pack("<I", len(body)) + body
        if len(block) + len(r) > 0xFF00:                   # htslib's cut: a record that does not fit the open block starts the next one
            out.append(_bgzf(bytes(block))); block = bytearray()
        block += r
    out.append(_bgzf(bytes(block))); out.append(_bgzf(b""))
    with open(bam, "wb") as f:
        f.write(b"".join(out))
    return m


def test_device_and_host_decoders_agree_at_scale(engine, tmp_path):
    """~200 k synthetic reads over many BGZF blocks, random nM / NH tags of every integer type (or none, or both twice): the device and
    the host decoder give the same read arrays, report and reason arrays under all three filters"""
    bam, fa, bct = (str(tmp_path / x) for x in ("s.bam", "ref.fa", "bc.tsv"))
    m = write_tagged_bam(tmp_path, 200_000, bam, fa, bct)
    barcodes = hostio.synth_barcodes(m)
    assert os.path.getsize(bam) > 100 * 65536 // 4
    filt = hostio.SplitFilters(5, 1, 3)
    names, lens, first = hostio.bam_header(bam)
    dec = hostio.decode_bam(bam, barcodes, min_mapq=60, filters=filt)
    nt, seqs = tsvio.read_fasta(fa)
    engine.set_contigs(lens)
    for t, s in enumerate(seqs):
        engine.load_reference(t, np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8))
    engine.set_barcodes(m.celltype_of, 2); engine.set_region()
    engine.set_keep_reads(True)
    engine.set_split_filters(filt)
    try:
        info, cb_pass, cb_low = engine.load_bam(bam, barcodes, min_mapq=60, first_record_offset=first)
        dev = engine.reads_to_host()
        n, f = engine.split_reasons()
    finally:
        engine.set_keep_reads(False)
        engine.set_split_filters(None)
    np.testing.assert_array_equal(n, dec.reasons[0]); np.testing.assert_array_equal(f, dec.reasons[1])
    assert hostio.split_report([info[k] for k in pipeline.REPORT_KEYS], [(n, f)]) == dec.report
    assert (n[2:] > 0).sum() >= 10 and n[0] == info["pass_reads"] and n[1] == info["mapq_filtered"]
    np.testing.assert_array_equal(cb_pass, dec.cb_pass); np.testing.assert_array_equal(cb_low, dec.cb_low)
    assert_same_records(dev, dec.records, phased_a=True)
