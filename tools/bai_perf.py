#!/usr/bin/env python3
"""Measurement aid for the device index builder (csrc/bamindex.hip), on the synthetic BAM of lsio_synth_bam that tools/split_bam_perf.py
uses (--config / --reads) or any coordinate-sorted BAM given with --bam and --meta.  Reports, as one JSON line:

  index             lsg_bam_index: lsg_bai_info's phase times and the whole call, the median over --repeat calls after one warm-up call;
                    the counts (records, runs, chunks, bins, windows, bytes)
  host_full_s       hostio.build_bai(full=True) - the host twin, one thread - on the same file, same session; same_bytes: the two files
                    are equal
  host_linear_s     the existing hostio.build_bai (linear index only) on the same file
  split_off / split_on   lsg_split_bam without and with lsg_set_split_index: per process the median ms_total of --repeat calls after
                    a warm-up call, processes of the two kinds alternating (--rounds of each); "median": over the processes,
                    "spread": the smallest and largest of them.  index_ms: the part of the call spent on the indexes (the sum of
                    the cell types' ms_total)
  parent_off        with --parent_lib (the library built from the parent commit): its lsg_split_bam, in processes alternating with
                    split_off's.  The condition to read: split_off's median is not above parent_off's beyond the two spreads

Every timed split runs in a child process of its own that loads one library with ctypes and nothing else of the package, so that a
parent commit's library - which lacks the newer entry points - is driven by the same code.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import mmap
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INDEX_PHASES = ("ms_h2d", "ms_inflate", "ms_chain", "ms_facts", "ms_runs", "ms_linear", "ms_print", "ms_total")


def child(a):
    """one process, one library: a warm-up call and --repeat timed calls of lsg_split_bam; prints {"ms_total": [...], "index_ms": [...]}"""
    import numpy as np
    from longsom_amd._lib import BaiInfo, SplitInfo            # (the structures only: no library is loaded by the import)
    lib = C.CDLL(a.lib)
    lib.lsg_create.restype = C.c_int; lib.lsg_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.lsg_destroy.argtypes = [C.c_void_p]
    lib.lsg_last_error.restype = C.c_char_p
    lib.lsg_split_bam.restype = C.c_int
    lib.lsg_split_bam.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SplitInfo)]
    with open(a.table) as f:
        t = json.load(f)
    ct = np.ascontiguousarray(t["celltype_of"], np.int32)
    h = C.c_void_p()
    if lib.lsg_create(a.device, C.byref(h)) != 0:
        sys.exit("lsg_create: " + lib.lsg_last_error().decode())
    if a.index:
        lib.lsg_set_split_index.argtypes = [C.c_void_p, C.c_int]
        lib.lsg_get_split_index_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(BaiInfo)]
        lib.lsg_set_split_index(h, 1)
    joined = "\n".join(t["barcodes"]).encode()
    ms, index_ms = [], []
    with open(a.bam, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            buf = np.frombuffer(mm, dtype=np.uint8)
            try:
                for k in range(a.repeat + 1):
                    info = SplitInfo()
                    if lib.lsg_split_bam(h, C.c_void_p(buf.ctypes.data), size, t["first"], joined, len(t["barcodes"]), ct.ctypes.data_as(C.c_void_p), t["n_ct"], a.min_MQ,
                                         C.byref(info)) != 0:
                        sys.exit("lsg_split_bam: " + lib.lsg_last_error().decode())
                    if k:
                        ms.append(info.ms_total)
                        if a.index:
                            tot = 0.0
                            for c in range(t["n_ct"]):
                                bi = BaiInfo(); lib.lsg_get_split_index_info(h, c, C.byref(bi)); tot += bi.ms_total
                            index_ms.append(tot)
            finally:
                del buf
    lib.lsg_destroy(h)
    print(json.dumps({"ms_total": ms, "index_ms": index_ms}))


def run_child(lib, bam, table, a, index):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--bam", bam, "--table", table, "--min_MQ", str(a.min_MQ), "--repeat", str(a.repeat),
                          "--device", str(a.device)] + (["--index"] if index else []), check=True, capture_output=True, text=True, timeout=600)
    return json.loads(out.stdout.strip().split("\n")[-1])


def summary(procs):
    med = [statistics.median(p["ms_total"]) for p in procs]
    d = {"median_ms": round(statistics.median(med), 2), "spread_ms": [round(min(med), 2), round(max(med), 2)], "per_process_ms": [round(m, 2) for m in med]}
    if procs and procs[0]["index_ms"]:
        d["index_ms"] = round(statistics.median(statistics.median(p["index_ms"]) for p in procs), 2)
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--bam", default=""); ap.add_argument("--meta", default=""); ap.add_argument("--min_MQ", type=int, default=30)
    ap.add_argument("--config", default="C1"); ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3); ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent_lib", default="", help="liblongsom_hip.so built from the parent commit")
    ap.add_argument("--outdir", default=""); ap.add_argument("--no_host", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS); ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--table", default="", help=argparse.SUPPRESS); ap.add_argument("--index", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    import torch
    from longsom_amd import _lib, hostio, synth
    from longsom_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("bai_perf: no GPU")
    if bool(a.bam) != bool(a.meta):
        sys.exit("bai_perf: --bam and --meta go together")
    tmp = tempfile.TemporaryDirectory(dir=a.outdir or None)
    if a.bam:
        bam, table = a.bam, hostio.read_barcodes(a.meta)
    else:
        bam = os.path.join(tmp.name, "synth.bam")
        model = synth.named(a.config, n_reads=a.reads)
        hostio.synth_bam(model, bam)
        table = hostio.BarcodeTable(hostio.synth_barcodes(model), np.asarray(model.celltype_of, np.uint8), ["Cancer", "Non-Cancer"])
    res = {"bam": os.path.basename(bam), "bam_bytes": os.path.getsize(bam), "repeat": a.repeat, "rounds": a.rounds}
    print("bai_perf: %s, %d bytes" % (bam, res["bam_bytes"]), file=sys.stderr, flush=True)
    # ---- (a) the index of the whole file: device, host twin, the linear-index builder
    with Engine(a.device) as eng:
        eng.bam_index(bam)
        infos = [eng.bam_index(bam) for _ in range(a.repeat)]
        res["index"] = {k: round(statistics.median(i[k] for i in infos), 3) for k in INDEX_PHASES}
        res["index"].update({k: infos[0][k] for k in ("n_records", "n_placed", "n_runs", "n_chunks", "n_bins", "n_windows", "n_bytes")})
        dev = eng.table_bytes(eng.TABLE_BAI, infos[0]["n_bytes"])
    print("bai_perf: index %s" % json.dumps(res["index"]), file=sys.stderr, flush=True)
    if not a.no_host:
        t0 = time.perf_counter(); full = hostio.build_bai(bam, os.path.join(tmp.name, "full.bai"), full=True); res["host_full_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter(); hostio.build_bai(bam, os.path.join(tmp.name, "lin.bai")); res["host_linear_s"] = round(time.perf_counter() - t0, 3)
        with open(full, "rb") as f:
            res["same_bytes"] = f.read() == dev
    # ---- (b), (c) the split: switch off / on / the parent's library, in alternating processes
    tab = os.path.join(tmp.name, "table.json")
    with open(tab, "w") as f:
        json.dump({"barcodes": list(table.barcodes), "celltype_of": [int(x) for x in table.celltype_of], "n_ct": len(table.celltype_names), "first": hostio.bam_header(bam)[2]}, f)
    kinds = [("split_off", _lib.LIB_PATH, False), ("split_on", _lib.LIB_PATH, True)] + ([("parent_off", a.parent_lib, False)] if a.parent_lib else [])
    procs = {k: [] for k, _, _ in kinds}
    for r in range(a.rounds):
        for k, lib, index in (kinds if r % 2 == 0 else kinds[::-1]):
            procs[k].append(run_child(lib, bam, tab, a, index))
            print("bai_perf: round %d %s %s" % (r, k, json.dumps(procs[k][-1])), file=sys.stderr, flush=True)
    for k in procs:
        res[k] = summary(procs[k])
    print(json.dumps(res))
    tmp.cleanup()
    if res.get("same_bytes") is False:
        sys.exit("bai_perf: the device's index differs from the host twin's")


if __name__ == "__main__":
    main()
