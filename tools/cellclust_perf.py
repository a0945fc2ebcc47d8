"""Development aid / DESIGN.md numbers: the SingleCellGenotype step (per-cell verdicts, long table, four matrices) at n target sites x every
barcode over a resident synthetic load (C2), timed two ways from the same reads and targets:
  twin    reanno.single_cell_genotype - the device count, one tail round trip and the host's Python row builder: the only way to this
          text before csrc/cellgeno.hip (14 of the 16 columns, no matrices)
  device  cellclust.cell_genotype_matrices - count + classify + the five tables printed on the device and streamed to their files
usage: cellclust_perf.py [n_reads 2e6] [n_sites 2000] [n_cb 5000] [out_dir]"""
import os
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from longsom_amd import cellclust, hostio, reanno, synth
from longsom_amd.engine import Engine

n_reads = int(float(sys.argv[1])) if len(sys.argv) > 1 else 2_000_000
n_sites = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
n_cb = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
out_dir = sys.argv[4] if len(sys.argv) > 4 else tempfile.mkdtemp(prefix="cellclust_perf_")
os.makedirs(out_dir, exist_ok=True)
model = synth.named("C2", n_reads=n_reads, n_cb=n_cb)
eng = Engine(0, stream=torch.cuda.current_stream().cuda_stream)
eng.set_contigs(model.contig_len); eng.synth_reference(model.seed); eng.set_barcodes(model.celltype_of, 2)
eng.synth_reads(model)
rng = np.random.default_rng(3)
x = rng.choice(len(model.exon_start), size=n_sites, replace=True)
gene_of_exon = np.searchsorted(model.gene_exon_off, x, side="right") - 1
keys = np.unique((model.gene_tid[gene_of_exon].astype(np.int64) << 32) | (model.exon_start[x].astype(np.int64) + rng.integers(0, np.maximum(model.exon_len[x], 1))))
alt = rng.integers(0, 4, len(keys))
names = list(model.contig_names)
vf = os.path.join(out_dir, "targets.tsv")
with open(vf, "w") as f:
    f.write("#CHROM\tStart\n")
    for k, a in zip(keys.tolist(), alt.tolist()):
        p = (k & 0xFFFFFFFF) + 1
        f.write("\t".join([names[k >> 32], str(p), str(p), "N", "ACTG"[a], "PASS", "Cancer"] + ["."] * 6 + ["4", ".", "."]) + "\n")
table = hostio.BarcodeTable(hostio.synth_barcodes(model), np.asarray(model.celltype_of, np.uint8), ["Cancer", "Non-Cancer"])
kw = dict(min_bq=30, min_mq=60, alpha2=0.2474528917555431, beta2=162.03696139428595, pvalue=0.01, chrm_contaminant="True")
os.environ["LSG_TIMING"] = "1"                      # (the twin prints its own split: device, tails, table)
t0 = time.perf_counter()
rows = reanno.single_cell_genotype(eng, vf, table, names, os.path.join(out_dir, "twin.tsv"), strict_cb=False, **kw)
t_twin = time.perf_counter() - t0
best = 1e9
for _ in range(2):
    t0 = time.perf_counter()
    rows_dev = cellclust.cell_genotype_matrices(eng, vf, table, names, os.path.join(out_dir, "dev"), None, **kw)
    best = min(best, time.perf_counter() - t0)
assert rows == rows_dev
sizes = {o: os.path.getsize(os.path.join(out_dir, "dev." + o + ".tsv")) for o in ("SingleCellGenotype", "DpMatrix", "AltMatrix", "VAFMatrix", "BinaryMatrix")}
with open(os.path.join(out_dir, "twin.tsv")) as a, open(os.path.join(out_dir, "dev.SingleCellGenotype.tsv")) as b:
    same = all(x.rstrip("\n") == "\t".join(y.split("\t")[:14]) for x, y in zip(a, b))
print("sites %d x barcodes %d = %d rows: twin (14 columns, no matrices) %.2f s; device count + classify + five tables to files %.2f s (%.1fx); "
      "text %.0f MB long + %.0f MB matrices; first 14 columns equal the twin's: %s"
      % (len(keys), n_cb, rows, t_twin, best, t_twin / best, sizes["SingleCellGenotype"] / 1e6, sum(v for k, v in sizes.items() if k != "SingleCellGenotype") / 1e6, same))
