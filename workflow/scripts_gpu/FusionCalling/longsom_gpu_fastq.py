#!/usr/bin/env python3
# MI355X drop-in for LongSom's rules BamToFastq + ConcatFastq of workflow/rules/FusionCalling.smk: the unsplit BAM and the barcode table in, {id}.fastq out
# (longsom_amd.cli.fusion_fastq).
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from longsom_amd import cli  # noqa: E402

if __name__ == "__main__":
    cli.fusion_fastq()
