#!/usr/bin/env python3
# MI355X drop-in for the `samtools index` of LongSom's rule IndexBarcodedBam_PoN (workflow/rules/PoN.smk:78-96): --bam X [--out X.bai]
# [--device N] writes the BAM's .bai (longsom_amd.cli.index_bam).
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from longsom_amd import cli  # noqa: E402

if __name__ == "__main__":
    cli.index_bam()
