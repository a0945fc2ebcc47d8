#!/usr/bin/env python3
"""Read-filter goldens: RUN the reference's own SplitBamCellTypes.split_bam (with --max_nM / --max_NH / --n_trim) and
BaseCellCounter.py (unmodified, imported from the reference tree, no bytecode written) over one small BAM and commit what they
write.  Runs only in the build container, through tools/minipysam.py exactly as tools/make_pileup_goldens.py does (its
run_chain drives the two scripts; only split_bam's three filter arguments differ).

The BAM (tests/golden/readfilter.bam, .fa, .barcodes.tsv): the random reads of make_pileup_goldens.random_reads on one contig,
each with nM / NH tags of the integer types c C s S i I or without them, MAPQ failures combined with both, soft clips of
5 / 19 / 20 / 29 / 30 / 40 bases at either end, leading hard clips, single-operation CIGARs, reverse reads, deletions and insertion
anchors right at the trim boundary, and filtered reads whose report keys first appear out of reason-index order (NH before nM).
No read has a trim window longer than itself (the reference raises there).

Per setting S (SETTINGS below: each filter alone, all three together) under tests/golden/:
  readfilter.S.report.txt        the SplitBam report, Total_time dropped
  readfilter.S.<celltype>.tsv    BaseCellCounter's table of the cell type's split BAM, fileDate dropped
  readfilter.S.digests.json      per cell type, the first 12 hex digits of the SHA-1 of every record the split BAM holds, in order
"""
import contextlib
import hashlib
import io
import json
import os
import struct
import sys
import tempfile
import shutil
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_pileup_goldens as MPG  # noqa: E402
import minipysam  # noqa: E402
from tests.support import bamwrite  # noqa: E402

OUT = MPG.OUT
MIN_MQ = 60
SETTINGS = {            # name: (max_nM, max_NH, n_trim)
    "nm": (5, None, 0),
    "nh": (None, 1, 0),
    "trim": (None, None, 5),
    "all": (5, 1, 5),
}
MAX_TRIM = 5            # the largest n_trim of SETTINGS: no read of the file may be shorter than its window under it


def aux_int(tag, ty, v):
    return tag.encode() + ty.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty], v)


def trim_window(cigar, n_trim):
    """SplitBamCellTypes.py:129-158, restated to keep the file clear of reads the reference raises on"""
    ops = bamwrite.parse_cigar(cigar)

    def end(op, ln):
        return (30 + n_trim if 20 <= ln < 30 else ln + n_trim) if op == 4 else n_trim
    if len(ops) > 1:
        return end(*ops[0]), end(*ops[-1])
    return n_trim, n_trim


def add_clip(rng, r, at_start, length):
    ops = bamwrite.parse_cigar(r["cigar"])
    edge = ops[0] if at_start else ops[-1]
    if edge[0] in (4, 5):                              # the end already has a clip
        return r
    bases = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=length))
    qual = [int(x) for x in rng.integers(2, 41, size=length)]
    clip = "%dS" % length
    if at_start:
        return dict(r, cigar=clip + r["cigar"], seq=bases + r["seq"], qual=qual + r["qual"])
    return dict(r, cigar=r["cigar"] + clip, seq=r["seq"] + bases, qual=r["qual"] + qual)


def make_reads(rng, seqs, cells):
    contigs = [("chr1", len(seqs["chr1"]))]
    reads = MPG.random_reads(rng, contigs, seqs, cells, n_clusters=7, per_cluster=30)
    out = []
    for r in reads:
        u = rng.random()
        if u < 0.12:
            r = add_clip(rng, r, True, int(rng.choice([5, 19, 20, 29, 30, 40])))
        elif u < 0.24:
            r = add_clip(rng, r, False, int(rng.choice([5, 19, 20, 29, 30, 40])))
        elif u < 0.30:
            r = add_clip(rng, add_clip(rng, r, True, int(rng.choice([20, 29]))), False, int(rng.choice([19, 30])))
        out.append(r)
    # reads at the trim boundary (n_trim = 5): a deletion / insertion right after the trimmed bases at the start, right before them at the end
    ref = seqs["chr1"].upper().replace("N", "A")
    for i, (pos, cigar) in enumerate([(400, "5M2D30M"), (402, "4M2D30M"), (404, "5M1I30M"), (406, "4M1I30M"), (408, "30M2D4M"), (410, "30M2D5M"),
                                      (412, "29M1I5M"), (414, "3H36M"), (416, "2H5S31M"), (418, "40M"), (420, "36M1S"), (422, "20S30M")]):
        seq, x = [], pos
        for op, ln in bamwrite.parse_cigar(cigar):
            if op in (0, 7, 8):
                seq.append(ref[x:x + ln]); x += ln
            elif op in (2, 3):
                x += ln
            elif op in (1, 4):
                seq.append("".join("ACGT"[int(v)] for v in rng.integers(0, 4, size=ln)))
        seq = "".join(seq)
        out.append(dict(tid=0, pos=pos, cigar=cigar, seq=seq, qual=[int(v) for v in rng.integers(25, 41, size=len(seq))], flag=0x10 if i % 2 else 0,
                        mapq=60, tags={"CB": cells[i % len(cells)]}, name="b%d" % i))
    out = [r for r in out if max(trim_window(r["cigar"], MAX_TRIM)) <= len(r["seq"])]
    out.sort(key=lambda r: (r["tid"], r["pos"]))
    # the tags: the first reads of the file give NH before nM (the report's columns follow the file, not the reason index)
    forced = [("C", 1, "C", 3, 60), ("i", 2, None, None, 60), ("s", 9, "S", 1, 60), ("I", 0, "c", 1, 30), ("c", 7, None, None, 10)]
    for k, r in enumerate(out):
        if k < len(forced):
            nmt, nmv, nht, nhv, mq = forced[k]
            r["mapq"] = mq
        else:
            nmt = None if rng.random() < 0.12 else "cCsSiI"[int(rng.integers(0, 6))]
            nmv = int(rng.integers(0, 7))
            nht = None if rng.random() < 0.1 else "cCsSiI"[int(rng.integers(0, 6))]
            nhv = 1 if rng.random() < 0.85 else int(rng.integers(2, 4))
        aux = b""
        parts = []
        if nmt is not None:
            parts.append(aux_int("nM", nmt, nmv))
        if nht is not None:
            parts.append(aux_int("NH", nht, nhv))
        if rng.random() < 0.5:
            parts.reverse()
        r["aux"] = aux + b"".join(parts)
        if not r.get("name", "").startswith("b"):
            r["name"] = "q%d" % k
    return out


def write_bam(path, contigs, reads):
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs)
    out = b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(contigs))
    for name, ln in contigs:
        out += struct.pack("<I", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", ln)
    for r in reads:
        rec = bamwrite.encode_record(r["tid"], r["pos"], r["name"], r["flag"], r["mapq"], r["cigar"], r["seq"], r["qual"], r["tags"])
        body = rec[4:] + r["aux"]
        out += struct.pack("<I", len(body)) + body
    with open(path, "wb") as f:
        for i in range(0, len(out), 0xFF00):
            f.write(bamwrite._bgzf_block(out[i:i + 0xFF00]))
        f.write(bamwrite._bgzf_block(b""))


def record_digests(bam):
    d = minipysam.read_bgzf(bam)
    p = 8 + struct.unpack_from("<I", d, 4)[0]
    n_ref = struct.unpack_from("<I", d, p)[0]; p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<I", d, p)[0] + 4
    out = []
    while p + 4 <= len(d):
        bs = struct.unpack_from("<I", d, p)[0]
        out.append(hashlib.sha1(d[p + 4:p + 4 + bs]).hexdigest()[:12]); p += 4 + bs
    return out


def main():
    minipysam.install()
    split = MPG.load("PreProcessing/SplitBamCellTypes.py", "ref_splitbam")
    counter = MPG.load("SNVCalling/BaseCellCounter.py", "ref_counter")
    rng = np.random.default_rng(20261016)
    length = 3_000
    s = "".join(rng.choice(list("ACGT"), size=length))
    seqs = {"chr1": s}
    cells = ["ACGT%04dAA" % i for i in range(12)] + ["TGCA%04dTT" % i for i in range(10)]
    types_ = ["Cancer"] * 12 + ["Non-Cancer"] * 10
    reads = make_reads(rng, seqs, cells)
    bam, fa, bc = (os.path.join(OUT, "readfilter." + x) for x in ("bam", "fa", "barcodes.tsv"))
    write_bam(bam, [("chr1", length)], reads)
    MPG.write_fasta(fa, seqs)
    with open(bc, "w") as f:
        f.write("Index\tCell_type\n" + "".join("%s-1\t%s\n" % (c, t) for c, t in zip(cells, types_)))
    work = tempfile.mkdtemp(prefix="rfgold_")
    try:
        for name, (max_nm, max_nh, n_trim) in SETTINGS.items():
            # run_chain calls split_bam with the filters off: the same call with this setting's three arguments
            wrapped = types.SimpleNamespace(split_bam=lambda b, t, o, d, ti, _nm, _nh, mq, _tr: split.split_bam(b, t, o, d, ti, max_nm, max_nh, mq, n_trim))
            wdir = os.path.join(work, name)
            tables, report = MPG.run_chain(wrapped, counter, bam, bc, fa, "s", wdir, MIN_MQ)
            open(os.path.join(OUT, "readfilter.%s.report.txt" % name), "w").write(MPG.strip_report(report))
            for ct, t in tables.items():
                if t is not None:
                    open(os.path.join(OUT, "readfilter.%s.%s.tsv" % (name, ct)), "w").write(MPG.strip_date(t))
            dig = {ct: record_digests(os.path.join(wdir, "SplitBam", "s.%s.bam" % ct)) for ct in tables}
            json.dump(dig, open(os.path.join(OUT, "readfilter.%s.digests.json" % name), "w"), indent=0, sort_keys=True)
            print(name, MPG.strip_report(report).replace("\n", " | "), {ct: (t.count("\n") - 8 if t else None) for ct, t in tables.items()})
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    with contextlib.redirect_stderr(io.StringIO()) if os.environ.get("QUIET") else contextlib.nullcontext():
        main()
