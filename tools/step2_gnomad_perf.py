"""What step 2's gnomAD filter costs a fused run: run_chain over one resident sample with a gnomAD source - a JSON table, a prepared set -
with step 2 on the device and, alternating, on the host (LONGSOM_HOST_STEP2=1: the path every run with a source took before the allele
set), beside the run without a source; then the pieces alone: format_table(TABLE_STEP2) with the set loaded and with none, the export
of the run's allele queries, and gnomad_hit_keys over a gnomad_db-shaped sqlite of the same alleles (a fixture: a real database is
hundreds of millions of rows, its lookup time is not measured here).  The source holds a fixed tenth of the run's own allele queries.
usage: python tools/step2_gnomad_perf.py [n_reads] [repeats] [host_repeats] [out.json]      (a C2-shaped BAM of n_reads is written first; needs the GPU)"""
import hashlib, json, os, shutil, sqlite3, sys, tempfile, time
sys.path.insert(0, ".")
import numpy as np
from longsom_amd import calling, hostio, pipeline, synth
from longsom_amd.engine import Engine

n_reads = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
host_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 1
out_json = sys.argv[4] if len(sys.argv) > 4 else None      # the result is printed; also written here when given
m = synth.named("C2", n_reads=n_reads)
d = tempfile.mkdtemp(prefix="lsg_gnomad_")
bam, fa, bct = os.path.join(d, "S.bam"), os.path.join(d, "ref.fa"), os.path.join(d, "bc.tsv")
hostio.synth_bam(m, bam, fa)
hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
params = pipeline.SnvParams()
res = {"reads": n_reads, "runs": [], "note": "host = LONGSOM_HOST_STEP2=1, the path of every run with a gnomAD source before the allele set"}


def say(what):
    print("[step2_gnomad_perf] %s" % what, flush=True)


def digest(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 24), b""):
            h.update(piece)
    return h.hexdigest()


with Engine(0) as eng:
    sample = pipeline.load_sample(bam, bct, fa, eng, params.min_mapping_quality, count_params=params.count())

    def chain(mode, source, host=False):
        if host:
            os.environ["LONGSOM_HOST_STEP2"] = "1"
        out_dir = os.path.join(d, "out")
        try:
            t0 = time.time()
            out = pipeline.run_chain(sample, sample.table.celltype_of, sample.table.celltype_names, sample.dec.report, out_dir, "S", params, gnomad_af_json=source)
            wall = time.time() - t0
        finally:
            os.environ.pop("LONGSOM_HOST_STEP2", None)
        run = {"mode": mode, "wall_s": round(wall, 3), "step2_s": round(float(out.timings["step2"]), 3), "step2_gnomad_s": round(float(out.timings.get("step2_gnomad", 0.0)), 3),
               "step3_s": round(float(out.timings.get("step3", 0.0)), 3), "step2_md5": digest(out.step2), "step3_md5": digest(out.step3_unfiltered),
               "tagged_rows": sum(1 for l in open(out.step2, "rb") if not l.startswith(b"#") and b"gnomAD" in l.split(b"\t", 6)[5])}
        say(json.dumps(run))
        res["runs"].append(run)
        return out

    chain("warm-up, no source", None)                       # (allocations, first launches; its files are not compared)
    t0 = time.time(); queries = eng.step2_allele_queries(); res["queries"] = {"n": len(queries), "first_export_s": round(time.time() - t0, 4)}
    export = []
    for _ in range(5):
        t0 = time.perf_counter(); eng.step2_allele_queries(); export.append(time.perf_counter() - t0)
    res["queries"]["export_s"] = [round(x, 5) for x in export]
    picked = np.sort(queries)[::10]                         # a fixed tenth of the run's own alleles
    table = {k: 0.5 for k in (("%s:%d:%s:%s" % (sample.contig_names[t], p, chr(r), chr(a))) for t, p, r, a in zip(*(x.tolist() for x in calling.unpack_allele_keys(picked))))}
    src_json, src_set, src_db = os.path.join(d, "af.json"), os.path.join(d, "alleles.npz"), os.path.join(d, "gnomad_db.sqlite3")
    json.dump(table, open(src_json, "w"))
    t0 = time.time(); calling.write_gnomad_set(table, src_set, 0.01); res["prepare_set_s"] = round(time.time() - t0, 3)
    db = sqlite3.connect(src_db)
    db.execute("CREATE TABLE gnomad_db (chrom TEXT, pos INTEGER, ref TEXT, alt TEXT, AF REAL, PRIMARY KEY (chrom, pos, ref, alt))")
    db.executemany("INSERT INTO gnomad_db VALUES (?,?,?,?,?)", [((k.split(":")[0][3:] if k.startswith("chr") else k.split(":")[0]), int(k.split(":")[1]), k.split(":")[2], k.split(":")[3], v) for k, v in table.items()])
    db.commit(); db.close()
    res["source_alleles"] = len(table)
    # the source's answers alone (host work, no GPU): per query, over this run's queries
    for name, src in (("json", src_json), ("sqlite_fixture", src_db), ("set", src_set)):
        s = calling.open_gnomad(src)
        t0 = time.time(); hits = calling.gnomad_hit_keys(s, sample.contig_names, queries, params.max_gnomad_vaf); dt = time.time() - t0
        assert len(hits) == len(picked), (name, len(hits), len(picked))
        res.setdefault("hit_keys", {})[name] = {"s": round(dt, 3), "us_per_query": round(dt / max(1, len(queries)) * 1e6, 3)}
    say(json.dumps({k: res[k] for k in ("queries", "source_alleles", "hit_keys", "prepare_set_s")}))
    # the table's print alone, set loaded / none loaded, alternating (the call returns after its stream has drained)
    fmt = {"loaded": [], "none": []}
    for _ in range(max(3, reps)):
        for how in ("loaded", "none"):
            eng.load_alleleset(picked if how == "loaded" else None)
            t0 = time.perf_counter(); n2 = eng.format_table(eng.TABLE_STEP2); fmt[how].append(round(time.perf_counter() - t0, 4))
    eng.load_alleleset(None); eng.free_table(eng.TABLE_STEP2)
    res["format_step2_s"] = fmt; res["step2_MB"] = round(n2 / 1e6, 1)
    say(json.dumps({"format_step2_s": fmt, "step2_MB": res["step2_MB"]}))
    for rep in range(reps):
        chain("device, json", src_json)
        if rep < host_reps:
            chain("host, json", src_json, host=True)
        chain("device, set", src_set)
        if rep < host_reps:
            chain("host, set", src_set, host=True)
        chain("device, no source", None)
    with_src = [r for r in res["runs"] if r["mode"].endswith(("json", "set"))]
    res["same_files"] = len({(r["step2_md5"], r["step3_md5"]) for r in with_src}) == 1 and all(r["tagged_rows"] == len(picked) for r in with_src)
print(json.dumps(res, indent=1))
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    json.dump(res, open(out_json, "w"), indent=1)
shutil.rmtree(d, ignore_errors=True)
if not res["same_files"]:
    sys.exit("the runs with a source did not write the same step-2 / step-3 files")
