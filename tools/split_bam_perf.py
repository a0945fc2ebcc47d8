#!/usr/bin/env python3
"""Measurement aid for the device splitter (csrc/split.hip lsg_split_bam): the synthetic BAM of lsio_synth_bam (--config / --reads, the
one tools/fastq_perf.py uses) split over the model's barcodes and two cell types, or any BAM given with --bam and --meta.  Reports, as
one JSON line:

  ms_*              lsg_split_info's phase times, the median over --repeat calls after one warm-up call
  deflate_GBps      the uncompressed bytes over ms_deflate (k_sp_deflate alone);  file_bytes: the files' sizes
  copy_GBps         a device-to-device copy of the same uncompressed bytes, timed in the same session with device events
  device_wall_s     wall time BAM file -> BAM files: what cli.split_bam --device does (Engine.split_bam + one append_table a cell type, each
                    on its own thread)
  host_wall_s       the host twin (hostio.split_bam, one thread: the only path before) on the same file, same session
  size_ratio        device files' bytes / host files' bytes;  same_records: the files inflate to the same bytes (--verify)

Needs a GPU: there is no fall-back."""
import argparse
import gzip
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ("ms_h2d", "ms_inflate", "ms_chain", "ms_route", "ms_cut", "ms_gather", "ms_deflate", "ms_crc", "ms_pack", "ms_total")


def inflated_sha1(path):
    h = hashlib.sha1()
    with gzip.open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 24), b""):
            h.update(piece)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--bam", default="", help="a BAM to split (default: a synthetic one)"); ap.add_argument("--meta", default="", help="barcode table of --bam")
    ap.add_argument("--min_MQ", type=int, default=30)
    ap.add_argument("--config", default="C1"); ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3); ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--outdir", default=""); ap.add_argument("--no_host", action="store_true"); ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from longsom_amd import cli, hostio, synth
    from longsom_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("split_bam_perf: no GPU")
    if bool(a.bam) != bool(a.meta):
        sys.exit("split_bam_perf: --bam and --meta go together")
    tmp = tempfile.TemporaryDirectory(dir=a.outdir or None)
    if a.bam:
        bam, table = a.bam, hostio.read_barcodes(a.meta)
    else:
        bam = os.path.join(tmp.name, "synth.bam")
        model = synth.named(a.config, n_reads=a.reads)
        hostio.synth_bam(model, bam)
        table = hostio.BarcodeTable(hostio.synth_barcodes(model), np.asarray(model.celltype_of, np.uint8), ["Cancer", "Non-Cancer"])
    n_ct = len(table.celltype_names)
    res = {"bam": os.path.basename(bam), "bam_bytes": os.path.getsize(bam)}
    with Engine(a.device) as eng:
        eng.split_bam(bam, table.barcodes, table.celltype_of, n_ct, a.min_MQ)          # warm-up: code objects, the staging buffers' first use
        infos = [eng.split_bam(bam, table.barcodes, table.celltype_of, n_ct, a.min_MQ) for _ in range(a.repeat)]
        n_u = sum(infos[0]["n_ubytes"])
        res.update({k: round(statistics.median(i[k] for i in infos), 3) for k in PHASES})
        res.update(file_records=infos[0]["n_records"], records=infos[0]["n_written"][:n_ct], uncompressed_bytes=n_u, blocks=sum(infos[0]["n_blocks"]),
                   file_bytes=infos[0]["n_file_bytes"][:n_ct], deflate_GBps=round(n_u / (res["ms_deflate"] * 1e-3) / 1e9, 2))
        eng.free_table()
        src = torch.empty(n_u, dtype=torch.uint8, device="cuda:%d" % a.device).fill_(65)
        dst = torch.empty_like(src)
        dst.copy_(src); torch.cuda.synchronize()
        times = []
        for _ in range(max(a.repeat, 3)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        res["ms_copy"] = round(statistics.median(times), 3)
        res["copy_GBps"] = round(n_u / (res["ms_copy"] * 1e-3) / 1e9, 1)
        del src, dst
    dev_outs = [os.path.join(tmp.name, "device.%s.bam" % ct) for ct in table.celltype_names]
    t0 = time.perf_counter()
    rep_dev = cli._split_bam_device(bam, table, dev_outs, a.min_MQ, hostio.SplitFilters(), a.device)       # (its own Engine, as the CLI makes it)
    res["device_wall_s"] = round(time.perf_counter() - t0, 3)
    res["device_file_bytes"] = [os.path.getsize(p) for p in dev_outs]
    if not a.no_host:
        host_outs = [os.path.join(tmp.name, "host.%s.bam" % ct) for ct in table.celltype_names]
        t0 = time.perf_counter()
        rep_host = hostio.split_bam(bam, table, host_outs, a.min_MQ)
        res["host_wall_s"] = round(time.perf_counter() - t0, 3)
        res["host_file_bytes"] = [os.path.getsize(p) for p in host_outs]
        res["size_ratio"] = round(sum(res["device_file_bytes"]) / sum(res["host_file_bytes"]), 4)
        res["same_report"] = rep_dev == rep_host and list(rep_dev) == list(rep_host)
        if a.verify:
            res["same_records"] = all(inflated_sha1(d) == inflated_sha1(h) for d, h in zip(dev_outs, host_outs))
    print(json.dumps(res))
    tmp.cleanup()
    if not a.no_host and (not res["same_report"] or res.get("same_records") is False):
        sys.exit("split_bam_perf: the device's files differ from the host twin's")


if __name__ == "__main__":
    main()
