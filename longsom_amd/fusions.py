"""SomaticFusions on the host: ctat-LR-fusion's predictions + the barcode table -> the three fusion tables (FusionCalling.py:6-86, rule
SomaticFusions of rules/FusionCalling.smk:64-93).  A table job of a few hundred rows: pandas reads and writes the files (so numbers
print exactly as the reference's to_csv prints them), the counting in between is plain Python over the rows.

The read accessions of a prediction are the FASTQ names the BamToFastq step printed, `<BC>^<UMI>^<read name>`
(Engine.bam_fastq / hostio.bam_fastq): this is where the barcode and the UMI in a name are used."""
from typing import Dict, List, Tuple

import numpy as np

OUT_COLUMNS = ["#FusionName", "Filter", "UMI_Cancer", "UMI_Non-Cancer", "BC_Cancer", "BC_Non-Cancer", "MCF_Cancer", "MCF_Non-Cancer", "LeftGene",
               "LeftLocalBreakpoint", "LeftBreakpoint", "RightGene", "RightLocalBreakpoint", "RightBreakpoint", "SpliceType"]
LONG_COLUMNS = ["#FusionName", "LeftGene", "LeftBreakpoint", "RightGene", "RightBreakpoint", "SpliceType", "BC", "UMI", "ReadName"]


class FusionInputError(ValueError):
    pass


def number_duplicates(names: List[str]) -> List[str]:
    """A name that occurs more than once becomes name1, name2, ... in row order - different isoforms of one gene pair
    (rename_duplicates, FusionCalling.py:80-86); a name that occurs once stays."""
    total: Dict[str, int] = {}
    for n in names:
        total[n] = total.get(n, 0) + 1
    seen: Dict[str, int] = {}
    out = []
    for n in names:
        seen[n] = seen.get(n, 0) + 1
        out.append(n + str(seen[n]) if total[n] > 1 else n)
    return out


def split_accessions(cell, row_label) -> List[Tuple[str, str, str]]:
    """LR_accessions of one prediction: ','-separated `BC^UMI^ReadName` entries (FusionCalling.py:13,19-20).  An entry that does not
    have exactly three parts is an error naming the row (the reference's expand=True assignment fails or fills None there)."""
    if not isinstance(cell, str):
        raise FusionInputError("row %s: LR_accessions is empty" % (row_label,))
    out = []
    for entry in cell.split(","):
        parts = entry.split("^")
        if len(parts) != 3:
            raise FusionInputError("row %s: accession %r has %d '^'-separated parts, not BC^UMI^ReadName" % (row_label, entry, len(parts)))
        out.append((parts[0], parts[1], parts[2]))
    return out


def filter_of(umi_cancer: int, bc_cancer: int, mcf_cancer: float, mcf_noncancer: float, min_ac_reads: int, min_ac_cells: int,
              max_mcf_noncancer: float, delta_mcf: float) -> str:
    """The filter cascade in the reference's order (filtering, FusionCalling.py:68-78)"""
    if umi_cancer < min_ac_reads:
        return "Low_Cancer_UMI"
    if bc_cancer < min_ac_cells:
        return "Low_Cancer_BC"
    if mcf_noncancer > 0:
        if mcf_cancer - mcf_noncancer < delta_mcf:
            return "Low_delta_MCF"
        if mcf_noncancer > max_mcf_noncancer:
            return "High_Non-Cancer_MCF"
    return "PASS"


def fusion_report(fusions: str, barcodes: str, min_ac_reads: int, min_ac_cells: int, max_MCF_noncancer: float, deltaMCF: float, outdir: str) -> Dict[str, int]:
    """Writes outdir + 'unfiltered.Fusions.tsv' (no dot before 'unfiltered', as the reference), outdir + '.Fusions.tsv' and
    outdir + '.Fusions.SingleCellGenotype.tsv'; `outdir` is a path prefix (the rule passes FusionCalling/Somatic/{id}).  Returns the row
    counts of the three files."""
    import pandas as pd
    meta = pd.read_table(barcodes)
    cancer = meta[meta["Cell_type"] == "Cancer"]["Index"]
    noncancer = meta[meta["Cell_type"] == "Non-Cancer"]["Index"]
    cancer_set, noncancer_set = set(cancer), set(noncancer)

    df = pd.read_table(fusions)
    df = df[df["SpliceType"] == "ONLY_REF_SPLICE"].copy()
    df["#FusionName"] = number_duplicates(list(df["#FusionName"]))

    # the long form: one row per supporting read
    long_rows = []
    counts = {k: [] for k in ("UMI_Cancer", "UMI_Non-Cancer", "BC_Cancer", "BC_Non-Cancer")}
    for label, row in zip(df.index, df.itertuples(index=False)):
        rec = dict(zip(df.columns, row))
        reads = split_accessions(rec["LR_accessions"], label)
        for bc, umi, name in reads:
            long_rows.append([rec[c] for c in LONG_COLUMNS[:6]] + [bc, umi, name])
    # per fusion NAME (the numbered one: all rows that carry it), distinct barcodes and UMIs among the cancer and the non-cancer barcodes
    by_name: Dict[str, List[Tuple[str, str]]] = {}
    for r in long_rows:
        by_name.setdefault(r[0], []).append((r[6], r[7]))
    for name in df["#FusionName"]:
        reads = by_name.get(name, [])
        in_c = [(b, u) for b, u in reads if b in cancer_set]
        in_n = [(b, u) for b, u in reads if b in noncancer_set]
        counts["BC_Cancer"].append(len({b for b, _ in in_c})); counts["BC_Non-Cancer"].append(len({b for b, _ in in_n}))
        counts["UMI_Cancer"].append(len({u for _, u in in_c})); counts["UMI_Non-Cancer"].append(len({u for _, u in in_n}))
    for k in ("BC_Cancer", "BC_Non-Cancer", "UMI_Cancer", "UMI_Non-Cancer"):
        df[k] = np.asarray(counts[k], np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):      # (a table without cells of a type: inf / nan, as pandas divides)
        df["MCF_Cancer"] = np.asarray(counts["BC_Cancer"], np.float64) / np.float64(len(cancer))
        df["MCF_Non-Cancer"] = np.asarray(counts["BC_Non-Cancer"], np.float64) / np.float64(len(noncancer))
    df["Filter"] = [filter_of(int(u), int(b), float(mc), float(mn), min_ac_reads, min_ac_cells, max_MCF_noncancer, deltaMCF)
                    for u, b, mc, mn in zip(df["UMI_Cancer"], df["BC_Cancer"], df["MCF_Cancer"], df["MCF_Non-Cancer"])]
    if not len(df):
        df["Filter"] = df["Filter"].astype(object)

    out = df[OUT_COLUMNS]
    out.to_csv(outdir + "unfiltered.Fusions.tsv", sep="\t", index=False)
    passed = out[out["Filter"] == "PASS"]
    passed.to_csv(outdir + ".Fusions.tsv", sep="\t", index=False)
    keep = set(passed["#FusionName"])
    long_df = pd.DataFrame([r for r in long_rows if r[0] in keep], columns=LONG_COLUMNS)
    for c in LONG_COLUMNS[:6]:                                 # the columns keep the dtypes the predictions table gave them
        if len(long_df):
            long_df[c] = long_df[c].astype(df[c].dtype)
    long_df.to_csv(outdir + ".Fusions.SingleCellGenotype.tsv", sep="\t", index=False)
    return {"unfiltered": len(out), "pass": len(passed), "long": len(long_df)}
