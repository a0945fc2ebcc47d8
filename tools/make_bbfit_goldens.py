#!/usr/bin/env python3
"""Beta-binomial-fit goldens: RUN the reference's own PoN/BetaBinEstimation.py (unmodified, loaded from the reference tree given with
--reference, no bytecode written) on a small BaseCellCounter table and commit the table and what the script made of it under
tests/golden/bbfit/.

  counts.tsv            a table written by tsvio.format_counts_tsv: a few hundred rows over every REF letter a table can carry, N and an
                        IUPAC letter (R), rows on both sides of both thresholds and rows at exactly 0.10 (Alt_CC / NC) and 0.15 (Alt_BC / DP)
  sites.expected.tsv    the list extract_sites_for_betabinom_estimation returned for it, in order: Alt_CC, Ref_CC, Alt_BC, Ref_BC per kept row

rpy2 (and R, and VGAM) are not installed: the script imports them at its top and uses them in betabin_estimation alone, so empty
stand-in modules go into sys.modules for the import and the fit itself is never called - the fit's specification is the maximum of the
likelihood, which tests/test_bbfit_cpu.py takes from mpmath."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from longsom_amd import tsvio  # noqa: E402


def table():
    """keys, refs, counts [n, 42]: the hand-made edge rows first, then generated ones"""
    rows = []                                                    # (ref letter, DP, NC, alt BC by allele index, alt CC by allele index)

    def add(ref, dp, nc, alt_bc, alt_cc):
        rows.append((ref, dp, nc, dict(alt_bc), dict(alt_cc)))
    # exactly at the thresholds (not kept), one below and one above each; the other proportion far inside
    for ref, other in (("A", 1), ("C", 2), ("T", 3), ("G", 0)):
        add(ref, 20, 30, {other: 0}, {other: 3})                 # 3 / 30 == 0.10 in doubles: not kept
        add(ref, 20, 30, {other: 0}, {other: 2})
        add(ref, 20, 31, {other: 0}, {other: 3})                 # 3 / 31 < 0.10
        add(ref, 20, 10, {other: 3}, {other: 0})                 # 3 / 20 == 0.15: not kept
        add(ref, 40, 10, {other: 6}, {other: 0})                 # 6 / 40 == 0.15
        add(ref, 100, 50, {other: 15}, {other: 4})               # 15 / 100 == 0.15
        add(ref, 100, 50, {other: 14}, {other: 4})               # kept: both below
        add(ref, 100, 50, {other: 16}, {other: 4})
        add(ref, 100, 50, {other: 14}, {other: 5})               # 5 / 50 == 0.10
        add(ref, 21, 20, {other: 3, 4: 0}, {other: 1})           # 3 / 21 < 0.15, 1 / 20 < 0.10: kept
        add(ref, 200, 100, {4: 10, 5: 19}, {4: 4, 5: 5})         # insertions and deletions count as alternative: 29 / 200, 9 / 100: kept
        add(ref, 200, 100, {4: 10, 5: 20}, {4: 4, 5: 5})         # 30 / 200 == 0.15
    add("N", 50, 40, {}, {})                                     # REF outside the printed alleles: all six are summed, the row falls out by itself
    add("R", 50, 40, {}, {})
    add("N", 50, 40, {0: 1}, {0: 1})
    add("a", 50, 40, {}, {})                                     # a lower-case REF matches no allele either
    rng = np.random.default_rng(20240611)
    for _ in range(260):
        ref = "ACTG"[int(rng.integers(4))]
        dp = int(rng.integers(5, 400))
        nc = int(rng.integers(5, dp + 1))
        alt_bc, alt_cc = {}, {}
        if rng.random() < 0.6:
            for _k in range(int(rng.integers(1, 3))):
                s = int(rng.integers(6))
                if "ACTGID"[s] == ref:
                    continue
                alt_bc[s] = int(rng.integers(0, max(1, dp // 5)))
                alt_cc[s] = min(alt_bc[s], int(rng.integers(0, max(1, nc // 6))))
        add(ref, dp, nc, alt_bc, alt_cc)
    n = len(rows)
    counts = np.zeros((n, 42), np.uint32)
    refs = np.zeros(n, np.uint8)
    for i, (ref, dp, nc, alt_bc, alt_cc) in enumerate(rows):
        refs[i] = ord(ref)
        counts[i, 0], counts[i, 1] = dp, nc
        own = "ACTGID".find(ref)
        for s, v in alt_bc.items():
            counts[i, 10 + s] = v
        for s, v in alt_cc.items():
            counts[i, 2 + s] = v
        own = own if own >= 0 else 0                             # (REF N / R / a: the rest of the depth goes to A - all six are summed anyway)
        counts[i, 10 + own] += dp - int(counts[i, 10:16].sum())
        counts[i, 2 + own] += nc - int(counts[i, 2:8].sum())
        counts[i, 18:24] = counts[i, 10:16] * 30                 # BQ sums, strands: printed, not read by the fit
        counts[i, 26:32] = counts[i, 10:16] // 2
        counts[i, 34:40] = counts[i, 10:16] - counts[i, 26:32]
    keys = (np.arange(n, dtype=np.int64) * 7 + 100) | (np.int64(0) << 32)
    keys[n // 2:] += np.int64(1) << 32                            # two contigs
    keys[n // 2:] -= (n // 2) * 7
    return keys, refs, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference tree (workflow/scripts/PoN/BetaBinEstimation.py under it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bbfit"))
    a = ap.parse_args()
    for name in ("rpy2", "rpy2.robjects", "rpy2.robjects.packages", "rpy2.rinterface"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["rpy2.robjects.packages"].importr = None
    sys.modules["rpy2"].robjects = sys.modules["rpy2.robjects"]
    sys.modules["rpy2.rinterface"].RRuntimeWarning = Warning
    spec = importlib.util.spec_from_file_location("ref_betabin", os.path.join(a.reference, "workflow", "scripts", "PoN", "BetaBinEstimation.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    os.makedirs(a.out, exist_ok=True)
    keys, refs, counts = table()
    path = os.path.join(a.out, "counts.tsv")
    with open(path, "w") as f:
        f.write(tsvio.format_counts_tsv(keys, refs, counts, ["chr1", "chr2"], "N0_Norm.Epithelial", "##fileDate=01/01/2024\n"))
    sites = ref.extract_sites_for_betabinom_estimation(path)
    with open(os.path.join(a.out, "sites.expected.tsv"), "w") as f:
        f.write("Alt_CC\tRef_CC\tAlt_BC\tRef_BC\n")
        for row in sites:
            f.write("\t".join(str(int(x)) for x in row) + "\n")
    print("%d rows in the table, %d kept by the reference" % (len(keys), len(sites)))


if __name__ == "__main__":
    main()
