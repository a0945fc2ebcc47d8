#!/usr/bin/env python3
"""Measurement aid for the FASTQ printer (csrc/fastq.hip lsg_bam_fastq): a synthetic BAM from lsio_synth_bam (--config / --reads), or
any BAM given with --bam.  The synthetic BAM is printed in routed mode over the model's barcodes and two cell types (some of its reads
carry no CB tag, as in a real sample), a given BAM in plain mode or, with --meta, routed by that barcode table.  Reports, as one JSON line:

  ms_*              lsg_fastq_info's phase times, the median over --repeat calls after one warm-up call
  print_GBps        the text bytes over ms_print (k_fq_print alone: it reads 0.75 bytes and writes 1 byte per text byte of SEQ / QUAL)
  copy_GBps         a device-to-device copy of the same byte count timed in the same session with device events (torch's contiguous
                    copy_, a hipMemcpyAsync): the ceiling a pure writer of that many bytes can reach (it reads 1 and writes 1 per byte)
  device_wall_s     wall time BAM file -> FASTQ file: Engine.bam_fastq + append_table (lsg_append_table) into --outdir
  host_wall_s       the host twin (hostio.bam_fastq, one thread) on the same file; its output is compared with the device's

Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--bam", default="", help="a BAM to print (default: a synthetic one)")
    ap.add_argument("--meta", default="", help="barcode table of --bam: routed mode"); ap.add_argument("--min_MQ", type=int, default=30)
    ap.add_argument("--config", default="C1"); ap.add_argument("--reads", type=int, default=300_000)
    ap.add_argument("--repeat", type=int, default=5); ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--outdir", default=""); ap.add_argument("--no_host", action="store_true")
    a = ap.parse_args()
    import torch
    from longsom_amd import hostio, synth
    from longsom_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("fastq_perf: no GPU")
    tmp = tempfile.TemporaryDirectory(dir=a.outdir or None)
    bam, table = a.bam, hostio.read_barcodes(a.meta) if a.meta else None
    if not bam:
        import numpy as np
        bam = os.path.join(tmp.name, "synth.bam")
        model = synth.named(a.config, n_reads=a.reads)
        hostio.synth_bam(model, bam)
        table = hostio.BarcodeTable(hostio.synth_barcodes(model), np.asarray(model.celltype_of, np.uint8), ["Cancer", "Non-Cancer"])
    route = (None, None, 0, 0) if table is None else (table.barcodes, table.celltype_of, len(table.celltype_names), a.min_MQ)
    res = {"bam": os.path.basename(bam), "bam_bytes": os.path.getsize(bam)}
    with Engine(a.device) as eng:
        eng.bam_fastq(bam, *route)                                         # warm-up: code objects, the pinned staging buffers' first use
        infos = [eng.bam_fastq(bam, *route) for _ in range(a.repeat)]
        n_text = sum(infos[0]["n_bytes"])
        res.update(records=sum(infos[0]["n_printed"]), file_records=infos[0]["n_records"], text_bytes=n_text)
        for k in ("ms_h2d", "ms_inflate", "ms_chain", "ms_length", "ms_print", "ms_total"):
            res[k] = round(statistics.median(i[k] for i in infos), 3)
        res["print_GBps"] = round(n_text / (res["ms_print"] * 1e-3) / 1e9, 1)
        # the ceiling: a device-to-device copy of the same byte count, same session
        src = torch.empty(n_text, dtype=torch.uint8, device="cuda:%d" % a.device).fill_(65)
        dst = torch.empty_like(src)
        dst.copy_(src); torch.cuda.synchronize()
        times = []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        res["ms_copy"] = round(statistics.median(times), 3)
        res["copy_GBps"] = round(n_text / (res["ms_copy"] * 1e-3) / 1e9, 1)
        del src, dst
        # BAM file -> FASTQ file
        out = os.path.join(tmp.name, "device.fastq")
        t0 = time.perf_counter()
        eng.bam_fastq(bam, *route)
        open(out, "wb").close()
        eng.append_table(eng.TABLE_FASTQ, out)
        res["device_wall_s"] = round(time.perf_counter() - t0, 3)
    if not a.no_host:
        host_out = os.path.join(tmp.name, "host.fastq")
        t0 = time.perf_counter()
        hostio.bam_fastq(bam, host_out, table, a.min_MQ)
        res["host_wall_s"] = round(time.perf_counter() - t0, 3)
        same = os.path.getsize(out) == os.path.getsize(host_out)
        if same:
            with open(out, "rb") as f, open(host_out, "rb") as g:
                while same:
                    x, y = f.read(1 << 24), g.read(1 << 24)
                    same = x == y
                    if not x:
                        break
        res["device_equals_host"] = bool(same)
    print(json.dumps(res))
    tmp.cleanup()
    if not a.no_host and not res["device_equals_host"]:
        sys.exit("fastq_perf: the device's FASTQ differs from the host twin's")


if __name__ == "__main__":
    main()
