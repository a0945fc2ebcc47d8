#!/usr/bin/env python3
# MI355X-side drop-in for LongSom's workflow/scripts/PoN/BetaBinEstimation.py: same flags, same output file (longsom_amd.cli.betabin_estimation);
# needs neither R, rpy2 nor VGAM: the maximum-likelihood fit runs on the GPU over the listed BaseCellCounter tables.
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from longsom_amd import cli  # noqa: E402

if __name__ == "__main__":
    cli.betabin_estimation()
