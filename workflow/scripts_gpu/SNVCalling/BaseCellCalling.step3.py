#!/usr/bin/env python3
# MI355X drop-in for LongSom's workflow/scripts/SNVCalling/BaseCellCalling.step3.py: same flags, same output files
# (longsom_amd.cli.calling_step3).  Flags of this script alone: --device N decides and prints the rows on GPU N (csrc/step3.hip over
# the uploaded table), --native with the host twin of the same row code; without either the host's step 3 runs, as before.
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from longsom_amd import cli  # noqa: E402

if __name__ == "__main__":
    cli.calling_step3()
