#!/usr/bin/env python3
"""BnpC convergence goldens: RUN the reference's own scripts/CellClustering/libs/utils.py and libs/MCMC.py (unmodified, imported from the
tree given by --reference, no bytecode written) and commit what they return.  bottleneck and seaborn get the stand-ins of
tools/make_bnpc_estimate_goldens.py where they are not installed.  libs.MCMC is imported before anything is computed: its np.seterr
(MCMC.py:20) is what turns a zero variance or a negative quotient into get_lugsail_batch_means_est's FloatingPointError.

tests/golden/bnpcpsrf.values.npz   per case <c>: <c>.n (chains), <c>.s<i> (the series of chain i), <c>.b<i> (its burn-in) and <c>.psrf:
                                   get_lugsail_batch_means_est([(s0, b0), ...]) (utils.py:427-461), inf included.
  Series: AR(1) noise with rho in {0, 0.9, 0.99}; the part after the burn-in is standardised and placed at -2.99e4 + 3 z, so that
  |mean| / sd < 1e4 whatever the draw (asserted).  Lengths after burn-in 8, 9, 10, 15, 16, 35, 36, 100, 1023, 1024, 1025, 4097; 1 to 4
  chains with burn-ins that differ between them; a constant series (inf); chains of different lengths; and a case of length 17 with
  burn-in 8 whose value is below 1 (asserted).
tests/golden/bnpcpsrf.runs.npz     data [30][12] (NaN = missing) and per run <r> of MCMC.run((cutoff, 0), seed, 3, 0) (MCMC.py:79-123,
                                   138-177): <r>.cutoff, <r>.seed, <r>.ML [3][records], <r>.psrf_steps and <r>.psrf_values (every chain's
                                   "PSRF" list, asserted equal between the chains), <r>.burn_in, <r>.params_shape [3][3], <r>.assign_shape [3][2].
  Runs: cutoff 1.05 (a first run of 10 steps) and 1.01 (of 49).  Asserted: each ended within 5 extensions, and no recorded PSRF lies within
  1e-6 of its cutoff; a run that does not is made again under another seed.  The reference's run is not reproducible from its seed (its
  pool appends the chains in the order they finish, and extend_chain seeds by that position), so these are records, not regenerable bits.
The tool ends itself after 10 minutes.
"""
import argparse
import os
import signal
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import pandas as pd          # noqa: F401  (before the stand-ins)

from make_bnpc_estimate_goldens import stand_ins

LENGTHS = (8, 9, 10, 15, 16, 35, 36, 100, 1023, 1024, 1025, 4097)
RHOS = (0.0, 0.9, 0.99)
RUNS = (("ls105", 1.05, 7), ("ls101", 1.01, 8))                     # name, cutoff, --seed


def ar1(rng, n, rho):
    e = rng.standard_normal(n)
    x = np.empty(n)
    x[0] = e[0]
    for i in range(1, n):
        x[i] = rho * x[i - 1] + np.sqrt(1 - rho * rho) * e[i]
    return x


def series(rng, burn_in, length, rho):
    """burn_in + length values; the part after the burn-in has sample mean -2.99e4 and sample sd 3 up to rounding"""
    x = ar1(rng, burn_in + length, rho)
    kept = x[burn_in:]
    z = (x - kept.mean()) / kept.std(ddof=1)
    out = -2.99e4 + 3.0 * z
    assert abs(out[burn_in:].mean()) / out[burn_in:].std(ddof=1) <= 1e4
    return out


def value_cases(rng):
    cases = []
    for k, length in enumerate(LENGTHS):
        chains = 1 + k % 4 if length <= 100 else (2 if length == 1023 else 1)
        burns = [(3 + 5 * k + 7 * c) % 23 for c in range(chains)]
        cases.append(("len%d" % length, [(series(rng, b, length, RHOS[(k + c) % 3]), b) for c, b in enumerate(burns)]))
    for rho in RHOS:
        cases.append(("rho%g" % rho, [(series(rng, b, 100, rho), b) for b in (0, 11, 50)]))
    cases.append(("mixed", [(series(rng, 4, 36, 0.9), 4), (series(rng, 0, 100, 0.0), 0), (series(rng, 9, 15, 0.99), 9)]))      # n = round(mean n)
    cases.append(("short_one", [(series(rng, 2, 100, 0.9), 2), (series(rng, 5, 8, 0.0), 5)]))                                  # one chain below 9: inf
    cases.append(("constant", [(np.full(40, -30000.25), 7)]))
    cases.append(("constant2", [(np.full(40, -30000.25), 7), (np.full(33, -29000.5), 0)]))
    return cases


def below_one(ut, rng):
    """a series of length 17 with burn-in 8 whose value is below 1"""
    for _ in range(200):
        s = series(rng, 8, 9, 0.0)
        v = ut.get_lugsail_batch_means_est([(s, 8)])
        if np.isfinite(v) and v < 1 - 1e-6:
            return ("below1", [(s, 8)])
    sys.exit("no series of length 17 with burn-in 8 gave a value below 1")


def lugsail_run(data, cutoff, seed):
    import libs.CRP_learning_errors as CRP
    from libs.MCMC import MCMC
    model = CRP.CRP_errors_learning(data, DP_alpha=[-1, -1], param_beta=[.25, .25], FP_mean=0.01, FP_sd=0.01, FN_mean=0.2, FN_sd=0.1)
    mcmc = MCMC(model, sm_prob=0.33, dpa_prob=0.25, error_prob=0.25, sm_ratios=[0.75, 0.25], sm_steps=3)
    mcmc.run((cutoff, 0), seed, 3, 0)
    return mcmc.get_results()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a LongSom checkout (the directory that holds workflow/)")
    a = ap.parse_args()
    signal.alarm(600)
    stand_ins()
    sys.path.insert(0, os.path.join(a.reference, "workflow", "scripts", "CellClustering"))
    import libs.MCMC  # noqa: F401  (np.seterr, MCMC.py:20)
    import libs.utils as ut
    import scipy
    print("numpy", np.__version__, "scipy", scipy.__version__)
    rng = np.random.default_rng(20261019)

    arrays = {}
    cases = value_cases(rng)
    cases.append(below_one(ut, rng))
    for name, chains in cases:
        v = ut.get_lugsail_batch_means_est(chains)
        arrays[name + ".n"] = np.int64(len(chains))
        for i, (s, b) in enumerate(chains):
            arrays["%s.s%d" % (name, i)] = s
            arrays["%s.b%d" % (name, i)] = np.int64(b)
        arrays[name + ".psrf"] = np.float64(v)
        print("%-10s chains %d lengths %s psrf %.12g" % (name, len(chains), [len(s) - b for s, b in chains], v))
    assert arrays["below1.psrf"] < 1 and np.isinf(arrays["constant.psrf"]) and np.isinf(arrays["len8.psrf"]) and np.isfinite(arrays["len9.psrf"])
    path = os.path.join(OUT, "bnpcpsrf.values.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", len(arrays), "arrays,", os.path.getsize(path), "bytes")

    truth = rng.integers(0, 3, 30)
    proto = rng.random((3, 12)) < 0.5
    data = proto[truth].astype(float)
    flip = rng.random(data.shape) < 0.1
    data[flip] = 1 - data[flip]
    data[rng.random(data.shape) < 0.15] = np.nan
    arrays = {"data": data}
    for name, cutoff, seed in RUNS:
        for seed in range(seed, seed + 60, 10):                     # other seeds where a run does not meet the two conditions
            results = lugsail_run(data, cutoff, seed)
            assert len(results) == 3, "%s: %d chains came back" % (name, len(results))
            checks = results[0]["PSRF"]
            assert all(r["PSRF"] == checks and r["PSRF_cutoff"] == cutoff for r in results)
            if len(checks) <= 6 and all(abs(v - cutoff) > 1e-6 for _, v in checks):
                break
            print("%s: seed %d: %d extensions, PSRF %r: another seed" % (name, seed, len(checks) - 1, checks))
        assert len(checks) <= 6, "%s: %d extensions" % (name, len(checks) - 1)
        assert all(abs(v - cutoff) > 1e-6 for _, v in checks), "%s: a PSRF within 1e-6 of the cutoff: %r" % (name, checks)
        arrays[name + ".cutoff"], arrays[name + ".seed"] = np.float64(cutoff), np.int64(seed)
        arrays[name + ".ML"] = np.array([r["ML"] for r in results])
        arrays[name + ".psrf_steps"] = np.array([s for s, _ in checks], np.int64)
        arrays[name + ".psrf_values"] = np.array([v for _, v in checks], np.float64)
        arrays[name + ".burn_in"] = np.int64(results[0]["burn_in"])
        arrays[name + ".params_shape"] = np.array([r["params"].shape for r in results], np.int64)
        arrays[name + ".assign_shape"] = np.array([r["assignments"].shape for r in results], np.int64)
        print("%-6s cutoff %g records %d burn_in %d params %s PSRF %s" % (name, cutoff, arrays[name + ".ML"].shape[1], results[0]["burn_in"],
                                                                          [r["params"].shape[0] for r in results], checks))
    path = os.path.join(OUT, "bnpcpsrf.runs.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
