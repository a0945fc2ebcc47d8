#!/usr/bin/env python3
"""Times the cell-by-gene read count (csrc/genecounts.hip) at the bench's shape: the synthetic 10 M-read load (synth.named("C1")) against
a generated annotation of GENCODE's size (about 60 k genes, about 600 k elementary intervals).  Reports the HIP-event times of the
segment kernel and the read kernel (lsg_gene_count_info), the print of the matrix, and - for scale - a device-to-device copy of the
per-segment bytes the segment kernel reads (12 bytes a segment).  Needs a GPU; prints one JSON line.  Nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from longsom_amd import genecounts, synth  # noqa: E402
from longsom_amd.engine import Engine  # noqa: E402


def annotation(contig_len, n_genes: int, seed: int = 7) -> genecounts.Annotation:
    """n_genes genes spread over the contigs in proportion to their lengths, about ten exons each, neighbours overlapping now and then"""
    rng = np.random.default_rng(seed)
    total = int(np.sum(contig_len))
    gene, contig, s0, e0 = [], [], [], []
    names = ["c%d" % t for t in range(len(contig_len))]
    for t, L in enumerate(contig_len):
        n = max(1, int(round(n_genes * int(L) / total)))
        starts = np.sort(rng.integers(0, max(1, int(L) - 400), n))
        for at in starts:
            g = len(set(gene)) if not gene else gene[-1] + 1
            at = int(at)
            for _ in range(int(rng.integers(4, 16))):
                ln = int(rng.integers(3, 7))       # (tiny exons: the table's SIZE is GENCODE's on a 5 Mb contig, so it is far denser than on a genome)
                gene.append(g); contig.append(names[t]); s0.append(at); e0.append(min(at + ln, int(L))); at += ln + int(rng.integers(2, 7))
    ids = ["G%d" % g for g in range(gene[-1] + 1)]
    return genecounts.flatten(genecounts.Exons(ids, np.asarray(gene, np.int64), contig, np.asarray(s0, np.int64), np.asarray(e0, np.int64)), names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    model = synth.named("C1", n_reads=a.reads)
    t0 = time.time()
    ann = annotation(model.contig_len, a.genes)
    t_flatten = time.time() - t0
    rows = ["G%d" % g for g in range(ann.n_genes)]
    barcodes = ["CB%06d" % i for i in range(len(model.celltype_of))]
    order = genecounts.column_order(barcodes)
    with Engine(a.device) as eng:
        eng.set_contigs(model.contig_len); eng.synth_reference(model.seed); eng.set_barcodes(model.celltype_of, 2)
        eng.synth_reads(model)
        R, S, _ = eng.reads_shape()
        eng.load_annotation(ann, np.arange(ann.n_genes, dtype=np.int32), ann.n_genes)
        runs = []
        for _ in range(a.repeats + 1):                       # the first run is the warm-up
            eng.gene_counts_reset(); eng.load_annotation(ann, np.arange(ann.n_genes, dtype=np.int32), ann.n_genes)
            runs.append(eng.gene_counts())
        eng.gene_counts_set_text(rows, order, barcodes, "\t")
        torch.cuda.synchronize(); t0 = time.time()
        n_text = eng.format_table(eng.TABLE_GENE_COUNTS)
        t_print = time.time() - t0
        info = runs[-1]
        # for scale: a device-to-device copy of the bytes per segment the segment kernel streams (seg_read, seg_start, seg_len)
        src = torch.empty(S * 12, dtype=torch.uint8, device="cuda:%d" % a.device); dst = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        copies = []
        for _ in range(a.repeats + 1):
            ev[0].record(); dst.copy_(src); ev[1].record(); torch.cuda.synchronize()
            copies.append(ev[0].elapsed_time(ev[1]))
    med = lambda k: float(np.median([r[k] for r in runs[1:]]))
    print(json.dumps({"reads": R, "segments": S, "genes": ann.n_genes, "intervals": ann.n_intervals, "barcodes": len(barcodes), "flatten_s": round(t_flatten, 2),
                      "ms_segments": round(med("ms_segments"), 3), "ms_reads": round(med("ms_reads"), 3), "ms_d2d_copy_of_segment_bytes": round(float(np.median(copies[1:])), 3),
                      "segment_bytes": S * 12, "print_s": round(t_print, 3), "text_bytes": n_text,
                      "outcomes": {k: info[k] for k in ("n_assigned", "n_no_features", "n_ambiguity", "n_filtered", "n_unlisted")}, "repeats": a.repeats}))


if __name__ == "__main__":
    main()
