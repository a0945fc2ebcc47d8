"""One load of every form (csrc/load_form.h), and the double restart, over the same small device-generated sample - to look at what a
load queues, form by form:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/load_forms.py
    python tools/load_forms.py --compare OUT_A OUT_B

The first prints lsg_get_layout_info's path of every load (LSG_TIMING=1 adds the library's own lines on stderr).  The second reads the
kernel traces of two such runs and compares, queue by queue, the sequence of (short kernel name, grid, workgroup size): two builds that
do the same work in the same order give the same sequences."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_loads():
    from longsom_amd import synth
    from longsom_amd._lib import CountParams
    from longsom_amd.engine import Engine

    m = synth.named("C1", layout=1, n_reads=20_000)          # (layout 1: the library's own producer hands over tile-phased events)
    p = CountParams.longsom_defaults()
    p0 = CountParams.longsom_defaults(); p0.min_bq = 0
    same = (p.min_mq, p.flag_exclude, p.ignore_orphans)
    # (what is wanted, the count at load, keep the store, the load filter, LSG_TEST_KEYS_ONLY_REFUSED)
    loads = [("store, count on request", 2, None, True, None, False),
             ("store written by the pass that counts", 3, p, True, None, False),
             ("no store, descriptors (min_bq 0)", 4, p0, False, None, False),
             ("no store, lines (default load filter)", 5, p, False, None, False),
             ("no store, windows (the count's load filter)", 6, p, False, same, False),
             ("no store, both restarts (keys alone refused)", 5, p, False, same, True)]
    got = []
    with Engine(0) as eng:
        eng.set_contigs(m.contig_len); eng.synth_reference(m.seed); eng.set_barcodes(m.celltype_of, 2)
        for what, want, count, keep, filt, refused in loads:
            eng.set_count_at_load(count)
            eng.set_store_policy(eng.STORE_KEEP if keep else eng.STORE_SKIP_WHEN_COUNTED)
            eng.set_load_filter(*(filt or (0, 0, 0)))
            if refused:
                os.environ["LSG_TEST_KEYS_ONLY_REFUSED"] = "1"
            try:
                eng.synth_reads(m)
            finally:
                os.environ.pop("LSG_TEST_KEYS_ONLY_REFUSED", None)
                eng.set_count_at_load(None); eng.set_store_policy(eng.STORE_KEEP); eng.set_load_filter()
            path = eng.layout_info()[0]
            rows, cols = eng.pileup_count(count or p)
            print("load: %-48s path %d (wanted %d)  rows %s columns %d" % (what, path, want, list(rows), cols), flush=True)
            got.append(path == want)
    return 0 if all(got) else 1


def queue_sequences(out_dir):
    """{queue, in order of first use: [(short name, grid, workgroup)]} of the kernel trace under out_dir"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from kernel_names import short_kernel_name
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % out_dir)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    seqs = {}
    for r in rows:
        grid = tuple(int(r["Grid_Size_" + a]) for a in "XYZ"); wg = tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ")
        seqs.setdefault(r["Queue_Id"], []).append((short_kernel_name(r["Kernel_Name"]), grid, wg))
    return list(seqs.values())


def compare(dir_a, dir_b):
    a, b = queue_sequences(dir_a), queue_sequences(dir_b)
    ok = len(a) == len(b)
    print("queues: %d and %d" % (len(a), len(b)))
    for q, (sa, sb) in enumerate(zip(a, b)):
        attempts = sum(1 for k in sa if k[0].endswith("k_seg_static"))
        first = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), None if len(sa) == len(sb) else min(len(sa), len(sb)))
        if first is None:
            print("queue %d: %d dispatches (%d attempts at a load), identical" % (q, len(sa), attempts))
        else:
            ok = False
            print("queue %d: %d and %d dispatches, first difference at %d: %s | %s" % (q, len(sa), len(sb), first, sa[first:first + 1], sb[first:first + 1]))
    print("same work in the same order" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--compare", nargs=2, metavar=("OUT_A", "OUT_B"))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run_loads())
