"""Step 3 of the fused SNV chain on a C2-shaped sample (needs the GPU), in its four forms, alternating in one session: over the rows
lsg_step2_summary left resident (the default of run_chain), with LONGSOM_HOST_STEP3=1 (the survivors copied back, calling.step3 on the
host: the parent's path), over the uploaded step-2 file (calling.step3_device), and with the host twin of the row code
(calling.step3_native).  Prints per form the best and the median of the repetitions, the device's phases, and whether the files agree.
usage: python tools/step3_perf.py [n_reads] [reps]"""
import filecmp, json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, ".")
import torch
if not torch.cuda.is_available():
    sys.exit("step3_perf: no GPU")
from longsom_amd import calling, hostio, pipeline, synth
from longsom_amd.engine import Engine
n_reads = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
m = synth.named("C2", n_reads=n_reads)
d = tempfile.mkdtemp(prefix="lsg_step3_")
bam, fa, bct = os.path.join(d, "S.bam"), os.path.join(d, "ref.fa"), os.path.join(d, "bc.tsv")
hostio.synth_bam(m, bam, fa)
hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
sp = pipeline.SnvParams()
ARGS = (sp.delta_vaf, sp.delta_mcf, sp.min_ac_reads, sp.min_ac_cells, sp.clust_dist)
res = {"n_reads": n_reads, "reps": reps}
ref = os.path.join(d, "ref")                             # the files every form must write: the first host run's
os.makedirs(ref)


def summary(ts):
    return {"best": round(min(ts), 4), "median": round(statistics.median(ts), 4)}


def same(f, u):
    return filecmp.cmp(f, os.path.join(ref, "f.tsv"), shallow=False) and filecmp.cmp(u, os.path.join(ref, "u.tsv"), shallow=False)


with Engine(0) as eng:
    r = pipeline.load_sample(bam, bct, fa, eng, sp.min_mapping_quality)
    t3 = {"host": [], "device": []}; wait = {"host": [], "device": []}; ms = []; ok = {}
    for k in range(reps + 1):                            # (round 0 warms both forms up and leaves the reference files)
        for how in ("host", "device"):
            os.environ["LONGSOM_HOST_STEP3"] = "1" if how == "host" else "0"
            out = pipeline.run_chain(r, r.table.celltype_of, r.table.celltype_names, r.dec.report, os.path.join(d, how), "S", sp)
            if k == 0 and how == "host":
                shutil.copy(out.step3, os.path.join(ref, "f.tsv")); shutil.copy(out.step3_unfiltered, os.path.join(ref, "u.tsv"))
                shutil.copy(out.step2, os.path.join(d, "step2.tsv"))
                res["step2_bytes"] = os.path.getsize(out.step2); res["unfiltered_bytes"] = os.path.getsize(out.step3_unfiltered)
            ok[how] = same(out.step3, out.step3_unfiltered)
            if k:
                t3[how].append(out.timings["step3"]); wait[how].append(out.timings["tables_wait"])
                if how == "device":
                    ms.append(out.step3_report.get("ms"))
            res[how + "_path"] = out.step3_path
            if how == "device":
                res["device_report"] = {x: out.step3_report.get(x) for x in ("rows_in", "rows_all", "rows_pass", "rows_pass_unclustered", "n_clustered", "why")}
            shutil.rmtree(os.path.join(d, how), ignore_errors=True)      # (a run's tables are gigabytes at 10 M reads)
            print("run", k, how, out.timings["step3"], flush=True)
    os.environ.pop("LONGSOM_HOST_STEP3")
    for how in ("host", "device"):
        res["resident_" + how] = {"t_step3": summary(t3[how]), "tables_wait": summary(wait[how]), "same": ok[how]}
    res["resident_device"]["ms_rows_decide_cluster_print"] = [[round(x, 3) for x in q] for q in ms]
    print("STEP3_PERF partial " + json.dumps(res), flush=True)
    step2 = os.path.join(d, "step2.tsv")
    tu, tn = [], []
    for k in range(reps + 1):
        rep_u, rep_n = {}, {}
        t0 = time.time(); f, u = calling.step3_device(eng, step2, os.path.join(d, "uf.tsv"), os.path.join(d, "uu.tsv"), *ARGS, report=rep_u); tu.append(time.time() - t0)
        ok["uploaded"] = same(f, u)
        t0 = time.time(); f, u = calling.step3_native(step2, os.path.join(d, "nf.tsv"), os.path.join(d, "nu.tsv"), *ARGS, report=rep_n); tn.append(time.time() - t0)
        ok["native"] = same(f, u)
        print("forms", k, tu[-1], tn[-1], flush=True)
    res["uploaded"] = {"whole_call": summary(tu[1:]), "path": rep_u.get("path"), "ms_rows_decide_cluster_print": rep_u.get("ms"), "same": ok["uploaded"]}
    res["native"] = {"whole_call": summary(tn[1:]), "path": rep_n.get("path"), "same": ok["native"]}
print("STEP3_PERF " + json.dumps(res))
shutil.rmtree(d, ignore_errors=True)
