#!/usr/bin/env python3
"""Measurement aid for the beta-binomial fit (csrc/bbfit.hip): the bench's synthetic sample (C2's model, --reads of it, generated in
HBM, counted in the pass that loads it), then per cell type the pass over the resident count rows and, once, the solve.  Reports, as
one JSON line:

  rows, units         the cell types' count rows and the non-empty (tile, cell type) units the pass walks, a wave per unit
  accumulate_ms       per cell type, lsg_bbfit_accumulate's wall time (the call waits for its pass: the units' row offsets - a scan -,
                      the pass, and the counters' way back), the median over --repeat calls after one warm-up call
  read_bytes          per cell type, what the pass has to read of the rows: 64 of a row's 144 bytes (quads 0-3 of 9: DP, NC, CC, BC)
  accumulate_GBps     read_bytes over accumulate_ms
  copy_ms, copy_GBps  a device-to-device copy of read_bytes timed in the same session with device events (torch's contiguous copy_):
                      it reads and writes every byte once, so a pure reader of that many bytes can reach twice its rate
  loads_only_ms, lds_only_ms   the pass under LSG_BBFIT_PROBE=1 (it reads and filters, bins nothing) and =2 (it bins in LDS, the values
                      of 1024 and more nowhere): what the loads alone cost, and what the global atomics add
  seen, kept          rows the pass saw and kept (every site: no thinning)
  occupied            per histogram (Alt_CC, Ref_CC, NC, Alt_BC, Ref_BC, DP), the largest occupied value + 1: the solve's sums run that far
  solve_ms            lsg_bbfit_solve's wall time (both fits, one launch), median; iterations and status per fit (0 converged, 1 cap,
                      2 no rows, 3 no finite maximum)

  normal              what run_pon(fit=True) adds per normal, on a synthetic normal of --normal_reads reads written as a BAM: the fit's
                      first load + count and its pass, beside the load + count + call + tables every run makes (seconds, second round)

Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="C2"); ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=5); ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dump", default="", help="write the six histograms' occupied part to this .npz")
    ap.add_argument("--normal_reads", type=int, default=1_000_000, help="reads of the synthetic normal (a BAM file) the fused run's two loads are timed on; 0: skip")
    a = ap.parse_args()
    import numpy as np
    import torch
    from longsom_amd import bbfit, synth
    from longsom_amd._lib import CountParams
    from longsom_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("bbfit_perf: no GPU")
    model = synth.named(a.config, layout=1, n_reads=a.reads)
    cp = CountParams.longsom_defaults()
    res = {"config": a.config, "reads": a.reads}
    with Engine(a.device) as eng:
        eng.set_contigs(model.contig_len)
        eng.synth_reference(model.seed)
        eng.set_barcodes(model.celltype_of, 2)
        eng.set_load_filter(cp.min_mq, cp.flag_exclude, cp.ignore_orphans)
        eng.set_count_at_load(cp)
        eng.set_store_policy(eng.STORE_SKIP_WHEN_COUNTED)
        eng.synth_reads(model)
        rows, _ = eng.pileup_count(cp)
        stats = eng.count_stats()
        res.update(rows=rows, units=int(stats.n_units))
        cap = bbfit.capacity_for(cp.max_depth)
        acc_ms, seen, kept = [], [], []
        for ct in range(2):
            eng.bbfit_reset(cap)
            eng.bbfit_accumulate(ct, table=ct)                       # warm-up: the code object's first launch
            times = []
            for _ in range(a.repeat):
                eng.bbfit_reset(cap)
                t0 = time.perf_counter()
                s, k = eng.bbfit_accumulate(ct, table=ct)
                times.append((time.perf_counter() - t0) * 1e3)
            acc_ms.append(round(statistics.median(times), 3)); seen.append(s); kept.append(k)
        # where the pass's time goes: the same pass that bins nothing (loads and filter alone), and that bins in LDS alone (LSG_BBFIT_PROBE,
        # measurement only, the histograms are left incomplete and the library lets nothing read them)
        probes = {}
        for mode, name in ((1, "loads_only_ms"), (2, "lds_only_ms")):
            os.environ["LSG_BBFIT_PROBE"] = str(mode)
            probes[name] = []
            for ct in range(2):
                times = []
                for _ in range(a.repeat + 1):
                    eng.bbfit_reset(cap)
                    t0 = time.perf_counter()
                    eng.bbfit_accumulate(ct, table=ct)
                    times.append((time.perf_counter() - t0) * 1e3)
                probes[name].append(round(statistics.median(times[1:]), 3))
        del os.environ["LSG_BBFIT_PROBE"]
        res.update(probes)
        read_bytes = [64 * r for r in rows]
        res.update(accumulate_ms=acc_ms, read_bytes=read_bytes, seen=seen, kept=kept,
                   accumulate_GBps=[round(b / (ms * 1e-3) / 1e9, 1) for b, ms in zip(read_bytes, acc_ms)])
        copy_ms = []
        for b in read_bytes:
            src = torch.empty(max(b, 1), dtype=torch.uint8, device="cuda:%d" % a.device).fill_(1)
            dst = torch.empty_like(src)
            dst.copy_(src); torch.cuda.synchronize()
            times = []
            for _ in range(a.repeat):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            copy_ms.append(round(statistics.median(times), 3))
            del src, dst
        res.update(copy_ms=copy_ms, copy_GBps=[round(b / (ms * 1e-3) / 1e9, 1) for b, ms in zip(read_bytes, copy_ms)])
        # both cell types' rows in the histograms, then the solve
        eng.bbfit_reset(cap)
        for ct in range(2):
            eng.bbfit_accumulate(ct, table=ct)
        hist = eng.bbfit_fetch()
        res["occupied"] = [int(np.flatnonzero(h)[-1]) + 1 if h.any() else 0 for h in hist]
        if a.dump:
            np.savez_compressed(a.dump, hist=hist[:, :max(res["occupied"])])
        eng.bbfit_solve()
        times = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            est, infos = eng.bbfit_solve()
            times.append((time.perf_counter() - t0) * 1e3)
        res.update(solve_ms=round(statistics.median(times), 3), iterations=[i["iterations"] for i in infos], status=[i["status"] for i in infos], estimates=est)
    if a.normal_reads:
        res["normal"] = normal_twice(a)
    print(json.dumps(res))


def normal_twice(a):
    """what run_pon(fit=True) adds per normal: its first pass (load that makes the count and keeps no store, the fit's pass over every
    cell type) beside the pass every run makes (load, count, step-1 call, the per-normal tables), on one synthetic normal written as a BAM"""
    import tempfile
    from longsom_amd import bbfit, hostio, pipeline, synth
    from longsom_amd.engine import Engine
    m = synth.named("C2", n_reads=a.normal_reads)
    out = {"reads": a.normal_reads}
    with tempfile.TemporaryDirectory() as d, Engine(a.device) as eng:
        bam, fa, bct = os.path.join(d, "N.bam"), os.path.join(d, "ref.fa"), os.path.join(d, "barcodes.tsv")
        hostio.synth_bam(m, bam, fa)
        hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Epithelial", "Stromal"])
        out["bam_MB"] = round(os.path.getsize(bam) / 1e6, 1)
        p = pipeline.pon_params()
        for rep in range(2):                              # (the second round is the one reported: code objects and buffers are there)
            t0 = time.perf_counter()
            res = pipeline.load_sample(bam, bct, fa, eng, p.min_mapping_quality, count_params=p.count(), keep_store=False)
            eng.set_barcodes(res.table.celltype_of, 2)
            eng.pileup_count(p.count())
            eng.bbfit_reset(bbfit.capacity_for(p.max_depth))
            t1 = time.perf_counter()
            for ct in range(2):
                eng.bbfit_accumulate(ct, table=ct)
            t2 = time.perf_counter()
            res = pipeline.load_sample(bam, bct, fa, eng, p.min_mapping_quality)
            pipeline.chain_step1(res, res.table.celltype_of, res.table.celltype_names, res.dec.report, os.path.join(d, "out%d" % rep), "N", p, True)
            t3 = time.perf_counter()
            out.update(fit_load_count_s=round(t1 - t0, 3), fit_pass_s=round(t2 - t1, 4), run_load_count_call_tables_s=round(t3 - t2, 3))
    return out


if __name__ == "__main__":
    main()
