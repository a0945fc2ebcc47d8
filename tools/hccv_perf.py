"""Profile of reanno.hccv_filter on the step-2 table of a C2-shaped sample (the table is made by the fused SNV run first; needs the GPU),
then the same filter's whole call - decide, print, the three files written, the host's cluster step - in its four forms: the pandas form,
the host twin of the row code, the device over the uploaded file, the device over the resident step-2 text of a run; and the device's
kernels alone beside a device-to-device copy of the table's bytes.
usage: python tools/hccv_perf.py [n_reads] [--forms-only]      (--forms-only: without the row-wise run and the profile)"""
import cProfile, os, pstats, shutil, sys, tempfile, time
sys.path.insert(0, ".")
import torch
if not torch.cuda.is_available():                 # (torch's runtime first, as in the other tools that time a copy beside the library's kernels)
    sys.exit("hccv_perf: no GPU")
from longsom_amd import hostio, pipeline, reanno, synth
forms_only = "--forms-only" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "--forms-only"]
n_reads = int(float(argv[0])) if argv else 1_000_000
m = synth.named("C2", n_reads=n_reads)
d = tempfile.mkdtemp(prefix="lsg_hccv_")
bam, fa, bct = os.path.join(d, "S.bam"), os.path.join(d, "ref.fa"), os.path.join(d, "bc.tsv")
hostio.synth_bam(m, bam, fa)
hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
out = pipeline.run_snv(bam, bct, fa, os.path.join(d, "out"), "S")
print("step2: %.1f MB, %d rows" % (os.path.getsize(out.step2) / 1e6, sum(1 for l in open(out.step2) if not l.startswith("#"))))
for mode in (() if forms_only else ("1", "0")):
    os.environ["LONGSOM_HCCV_ROW_PATH"] = mode
    t0 = time.time(); o = reanno.hccv_filter(out.step2, os.path.join(d, "h" + mode), 50, 0.2, 0.25, 10000)
    print("row-wise" if mode == "1" else "column-wise", "%.2f s" % (time.time() - t0), [sum(1 for _ in open(o + s)) for s in ("", "2", "3")])
if not forms_only:
    cProfile.run("reanno.hccv_filter(out.step2, os.path.join(d, 'p'), 50, 0.2, 0.25, 10000)", os.path.join(d, "prof"))
    pstats.Stats(os.path.join(d, "prof")).sort_stats("cumulative").print_stats(22)
# ---- the four forms of the whole call, one session
import json
from longsom_amd.engine import Engine
ARGS = (50, 0.2, 0.25, 10000)
res = {"n_reads": n_reads, "step2_bytes": os.path.getsize(out.step2)}
os.environ["LONGSOM_HCCV_ROW_PATH"] = "0"


def best(fn, reps=3):
    ts = []
    for k in range(reps):
        t0 = time.time(); r = fn(k); ts.append(time.time() - t0)
    return min(ts), r


print("forms: pandas", flush=True)
res["pandas_s"], ref = best(lambda k: reanno.hccv_filter(out.step2, os.path.join(d, "w%d" % k), *ARGS), 2)
print("forms: native", flush=True)
rep = {}
res["native_s"], o = best(lambda k: reanno.hccv_filter_native(out.step2, os.path.join(d, "n%d" % k), *ARGS, report=rep))
print("forms:", json.dumps(res), flush=True)
res["native_path"] = rep.get("path"); res["native_same"] = all(open(o + x).read() == open(ref + x).read() for x in ("", "2", "3"))
print("forms: device", flush=True)
with Engine(0) as eng:
    rep = {}
    res["uploaded_s"], o = best(lambda k: reanno.hccv_filter_device(eng, out.step2, os.path.join(d, "u%d" % k), *ARGS, report=rep))
    res["uploaded_path"] = rep.get("path"); res["uploaded_ms_rows_decide_print"] = rep.get("ms"); res["rows"] = {k: rep.get(k) for k in ("rows_in", "rows_tsv2", "rows_tsv3", "rows_pass")}
    res["uploaded_same"] = all(open(o + x).read() == open(ref + x).read() for x in ("", "2", "3"))
    print("forms:", json.dumps(res), flush=True)
    # room for the resident runs' tables (gigabytes at 10 M reads): the first run's tables but its step-2 file, the other forms' outputs
    for root, _, files in os.walk(os.path.join(d, "out")):
        for x in files:
            if os.path.join(root, x) != out.step2:
                os.remove(os.path.join(root, x))
    for x in os.listdir(d):
        if x[:1] in ("n", "u"):
            os.remove(os.path.join(d, x))
    # the resident form: pass 1 of the re-annotation's chain with the filter made while the step-2 text is resident
    sp = pipeline.SnvParams()
    r = pipeline.load_sample(bam, bct, fa, eng, sp.min_mapping_quality, keep_unlisted=True)
    ts = []
    for k in range(3):
        p1 = pipeline.run_chain(r, r.table.celltype_of, r.table.celltype_names, r.dec.report, os.path.join(d, "res%d" % k), "S", sp, step3=False,
                                hccv=pipeline.HccvRequest(os.path.join(d, "res%d" % k, "HCCV", "S"), *ARGS))
        ts.append(p1.timings.get("hccv_device"))
        res["resident_path"] = (p1.hccv_report or {}).get("path"); res["resident_ms_rows_decide_print"] = (p1.hccv_report or {}).get("ms")
        res["resident_same"] = bool(p1.hccv) and all(open(p1.hccv + x).read() == open(ref + x).read() for x in ("", "2", "3"))
        shutil.rmtree(os.path.join(d, "res%d" % k), ignore_errors=True)      # (a run's tables are gigabytes at 10 M reads)
        print("forms: resident %d" % k, ts[-1], flush=True)
    res["resident_s"] = min(ts)
# the yardstick: a device-to-device copy of the table's bytes
n = res["step2_bytes"]
a = torch.empty(n, dtype=torch.uint8, device="cuda"); b = torch.empty_like(a)
b.copy_(a); torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ms = []
for _ in range(10):
    ev[0].record(); b.copy_(a); ev[1].record(); torch.cuda.synchronize(); ms.append(ev[0].elapsed_time(ev[1]))
res["d2d_copy_ms"] = min(ms)
print("HCCV_FORMS " + json.dumps(res))
shutil.rmtree(d, ignore_errors=True)
