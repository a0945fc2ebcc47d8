#!/usr/bin/env python3
# MI355X drop-in for LongSom's workflow/scripts/CellClustering/run_BnpC.py: same flags, same output files.  The sampler is the
# vendored BnpC's of the checkout this script is dropped into (../../scripts/CellClustering/libs, or --bnpc_libs DIR); the posterior
# estimate runs on the GPU (longsom_amd.cli.run_bnpc, longsom_amd.bnpc).
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from longsom_amd import cli  # noqa: E402

if __name__ == "__main__":
    cli.run_bnpc()
