#!/usr/bin/env python3
# MI355X drop-in for LongSom's rules split_per_bc + featureCount + format_featureCount of workflow/rules/CNACalling.smk: the unsplit BAM, the barcode
# table and the annotation in, {id}.counts.formated.txt out (longsom_amd.cli.gene_counts).
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from longsom_amd import cli  # noqa: E402

if __name__ == "__main__":
    cli.gene_counts()
