#!/usr/bin/env python3
"""Times the FormatInputBnpC step on the GPU: tools/bnpc_perf.py [barcodes] [sites] [--twin] [--keep DIR]

Cells are made from a seed (40 % uncovered, 35 % covered without alt reads, 25 % carried: VAF 1.0), loaded through cellgeno_load_counts and
given their text once.  Timed, by a host clock around calls that end in a device synchronise, warmed up and repeated: lsg_cellgeno_filter
plus the prints of LSG_TABLE_BNPC_BIN and LSG_TABLE_BNPC_VAF into their device buffers (thresholds 5 / 3, the rule's defaults).  Also
timed once: the same with both tables appended to files.  --twin: the device prints the step's INPUT matrices (LSG_TABLE_CELL_BIN / _VAF)
to files and cellclust.format_bnpc_input_host - the pandas restatement of the reference's script - is timed on them, its three files
compared with the device's.  --keep DIR: leave the files there (default: a temporary directory, removed).  Prints one JSON line."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longsom_amd import cellclust  # noqa: E402
from longsom_amd.engine import Engine  # noqa: E402


def make_cells(n_sites, n_cb, seed=7):
    rng = np.random.default_rng(seed)
    kind = rng.choice(3, size=(n_sites, n_cb), p=[0.4, 0.35, 0.25]).astype(np.uint8)
    dp = np.where(kind == 0, 0, 12).astype(np.uint32)
    alt = np.where(kind == 2, 12, 0).astype(np.uint32)
    return dp, alt


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_cb = int(args[0]) if args else 20000
    n_sites = int(args[1]) if len(args) > 1 else 5000
    twin = "--twin" in sys.argv
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    work = keep or tempfile.mkdtemp(prefix="bnpc_perf_")
    os.makedirs(work, exist_ok=True)
    c, p = 5, 3
    out = {"barcodes": n_cb, "sites": n_sites, "min_cells_per_mut": c, "min_pos_cov": p}
    try:
        dp, alt = make_cells(n_sites, n_cb)
        barcodes = ["BC%06d" % i for i in range(n_cb)]
        labels = ["chr%d:%d:A" % (1 + i % 22, 1000 + i) for i in range(n_sites)]
        bc_file = os.path.join(work, "barcodes.tsv")
        with open(bc_file, "w") as f:
            f.write("Index\tCell_type\tReannotated_cell_type\n" + "".join("%s\tCancer\t%s\n" % (b, "Non-Cancer" if i % 3 else "Cancer") for i, b in enumerate(barcodes)))
        with Engine(0) as eng:
            eng.cellgeno_load_counts(dp, alt, np.zeros(n_sites, np.uint8))
            eng.cellgeno_set_text([""] * n_sites, [""] * n_sites, labels, barcodes, [""] * n_cb, [], list(range(n_sites)), list(range(n_cb)), False)
            ok = np.ones(n_cb, np.uint8)

            def step():
                kept = eng.cellgeno_filter(c, p, ok)
                return kept, eng.format_table(eng.TABLE_BNPC_BIN) + eng.format_table(eng.TABLE_BNPC_VAF)
            for _ in range(3):
                kept, n_bytes = step()
            times = []
            for _ in range(20):
                t0 = time.perf_counter(); step(); times.append(time.perf_counter() - t0)
            out.update(rows_kept=kept[0], columns_kept=kept[1], text_bytes=n_bytes, filter_and_prints_ms_median=round(1e3 * float(np.median(times)), 3),
                       filter_and_prints_ms_min=round(1e3 * min(times), 3), filter_and_prints_ms_max=round(1e3 * max(times), 3), repeats=len(times))
            print("device step timed:", out, flush=True)
            t0 = time.perf_counter()
            cellclust.format_bnpc_input(eng, barcodes, [], bc_file, os.path.join(work, "dev"), c, p, float_cells=False)
            out["with_files_s"] = round(time.perf_counter() - t0, 3)
            print("device files written", flush=True)
            if twin:
                for m, slot in (("Binary", eng.TABLE_CELL_BIN), ("VAF", eng.TABLE_CELL_VAF)):
                    path = os.path.join(work, "in.%sMatrix.tsv" % m)
                    with open(path, "w") as f:
                        f.write("\t".join([""] + barcodes) + "\n")
                    eng.format_table(slot); eng.append_table(slot, path); eng.free_table(slot)
                    out["input_%s_bytes" % m] = os.path.getsize(path)
                print("input matrices written", flush=True)
        if twin:
            t0 = time.perf_counter()
            cellclust.format_bnpc_input_host(os.path.join(work, "in.BinaryMatrix.tsv"), os.path.join(work, "in.VAFMatrix.tsv"), bc_file, os.path.join(work, "twin"), c, p)
            out["pandas_twin_s"] = round(time.perf_counter() - t0, 3)
            out["twin_files_equal"] = all(open(os.path.join(work, "dev.%s.tsv" % o), "rb").read() == open(os.path.join(work, "twin.%s.tsv" % o), "rb").read() for o in cellclust.BNPC_OUTPUTS)
        print(json.dumps(out))
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
