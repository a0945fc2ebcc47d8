#!/usr/bin/env python3
"""Time BnpC's sampler on the device: 2 000 cells x 200 mutations with 10 planted clusters, 16 chains (longsom_amd.bnpc_sampler.run_chains'
own calls, so that the first steps and the late steps can be timed apart).

  device      seconds per step over the first 10 steps from the random start, and over 100 steps after step 200
  --sm_prob P --sm_steps S   with the split-merge move in a share P of the steps, S restricted scans each (run_BnpC.py's -smp, -sms; the
              ratios stay 0.75 / 0.25); the result then counts the moves of each kind over all chains and steps
  --eup P     with the error rates learned: the update in a share P of the steps (run_BnpC.py's -eup), priors FP (0.01, 0.01) and FN
              (0.1, 0.1) around the rates the other runs keep fixed; the result then counts the moves of each rate over all chains
  --reference DIR   also time the reference's sampler (libs/CRP.py, libs/MCMC.py of the LongSom checkout DIR, with the same --sm_prob) at the same
              shape on this host, one process per chain: its first 10 steps from its random start, and 10 steps from the planted partition
              (the state a chain is in after a few hundred steps), per step
  --lugsail   what the lugsail rule adds to a run (run_chains' Lugsail stop rule): one PSRF check (lsg_bnpcs_psrf over the second half of the
              records) and one 200-step extension (lsg_bnpcs_extend, which moves the records to their new rows), at 1 000 and at 10 000
              recorded steps; the records are marked as made through the test hook, no step is run.  Seconds, the median of 5 checks
Prints one JSON line.  For a per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bnpc_sampler_perf.py --late_only`.
"""
import argparse
import json
import os
import sys
import time

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np


def planted(N, M, K, seed=1):
    rng = np.random.default_rng(seed)
    truth = np.arange(N) % K
    g = (rng.random((K, M)) < 0.5)[truth]
    data = g.astype(float)
    data[g & (rng.random((N, M)) < 0.1)] = 0
    data[~g & (rng.random((N, M)) < 0.01)] = 1
    data[rng.random((N, M)) < 0.2] = np.nan
    return data, truth


def device(data, chains, late_only, sm_prob=0.0, sm_steps=3, eup=0.0):
    from longsom_amd import bnpc_sampler as bs
    from longsom_amd.engine import Engine
    model = bs.Model(data, 0.1, 0.01)
    seeds = list(range(1, chains + 1))
    steps = 300
    out = {}
    with Engine(0) as e:
        e.bnpcs_create(model, seeds, steps, 1 << 15)
        if sm_prob > 0:
            e.bnpcs_set_split_merge(sm_prob, 0.75, 0.25, sm_steps)
        if eup > 0:
            e.bnpcs_set_error_learning(eup, 0.01, 0.01, 0.1, 0.1)
        for c, s in enumerate(seeds):
            st = bs.initial_state(model, s)
            e.bnpcs_set_state(c, st.labels, st.theta, st.alpha)
        e.bnpcs_run(0, 1, steps + 1)
        t = time.perf_counter()
        e.bnpcs_run(1, 10, steps + 1)
        out["first10_s_per_step"] = (time.perf_counter() - t) / 10
        if late_only:
            e.bnpcs_run(11, 40, steps + 1)
            e.bnpcs_destroy()
            return out
        e.bnpcs_run(11, 190, steps + 1)
        t = time.perf_counter()
        e.bnpcs_run(201, 100, steps + 1)
        out["late100_s_per_step"] = (time.perf_counter() - t) / 100
        _, scalars, _ = e.bnpcs_fetch()
        out["clusters_at_10_200_300"] = [float(np.mean(scalars[:, s, 3])) for s in (10, 200, 300)]
        if sm_prob > 0:
            seen = np.bincount(e.bnpcs_fetch_moves().ravel(), minlength=5)
            out["moves"] = {"sweeps": int(seen[0]) - chains, "splits_declined": int(seen[1]), "splits_accepted": int(seen[2]), "merges_declined": int(seen[3]),
                            "merges_accepted": int(seen[4])}
        if eup > 0:
            rates, moves = e.bnpcs_fetch_error_rates()
            out["error_moves"] = dict(zip(("FP_accepted", "FP_declined", "FN_accepted", "FN_declined"), (int(x) for x in moves.sum(axis=0))))
            out["rates_at_300"] = {"FP": float(rates[:, 300, 0].mean()), "FN": float(rates[:, 300, 1].mean())}
        e.bnpcs_destroy()
    return out


def lugsail(data, chains):
    from longsom_amd import bnpc_sampler as bs
    from longsom_amd.engine import Engine
    model = bs.Model(data, 0.1, 0.01)
    rng = np.random.default_rng(1)
    out = {}
    with Engine(0) as e:
        for records in (1000, 10000):
            e.bnpcs_create(model, list(range(1, chains + 1)), records - 1, 1 << 15)
            for c in range(chains):
                e.bnpcs_test_set_ml(c, 0, -1e4 + 3 * rng.standard_normal(records))
            e.bnpcs_psrf([records // 2] * chains, records)
            checks = []
            for _ in range(5):
                t = time.perf_counter()
                stats = e.bnpcs_psrf([records // 2] * chains, records)
                checks.append(time.perf_counter() - t)
            t = time.perf_counter()
            e.bnpcs_extend(200)
            out["at_%d" % records] = {"psrf_check_s": float(np.median(checks)), "extend_200_s": time.perf_counter() - t, "psrf": bs.psrf_of_stats(stats),
                                      "label_records_gb": chains * records * model.N * 4 / 1e9}
            e.bnpcs_destroy()
    return out


def _reference_chain(args):
    ref, data, seed, assign, sm_prob, sm_steps = args
    from make_bnpc_estimate_goldens import stand_ins
    stand_ins()
    sys.path.insert(0, os.path.join(ref, "workflow", "scripts", "CellClustering"))
    import libs.CRP as CRP
    from libs.MCMC import MCMC, Chain_steps
    np.random.seed(seed)
    model = CRP.CRP(data, DP_alpha=[-1, -1], param_beta=[1, 1], FN_error=0.1, FP_error=0.01)
    model.init(assign=assign)
    mcmc = MCMC(model, sm_prob=sm_prob, dpa_prob=0.5, error_prob=0, sm_ratios=[0.75, 0.25], sm_steps=sm_steps)
    chain = Chain_steps(model, 1, 10, 5, mcmc.params, 0, False)
    t = time.perf_counter()
    chain.run()
    return (time.perf_counter() - t) / 10


def reference(ref, data, truth, chains, sm_prob=0.0, sm_steps=3):
    import multiprocessing as mp
    out = {}
    with mp.Pool(chains) as pool:
        for name, assign in (("first10_s_per_step", None), ("planted10_s_per_step", [int(x) for x in truth])):
            t = time.perf_counter()
            per = pool.map(_reference_chain, [(ref, data, s, assign, sm_prob, sm_steps) for s in range(1, chains + 1)])
            out[name] = (time.perf_counter() - t) / 10                # the chains run side by side: wall time per step of the run
            out[name + "_one_chain"] = float(np.mean(per))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cells", type=int, default=2000); ap.add_argument("--muts", type=int, default=200); ap.add_argument("--clusters", type=int, default=10)
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--reference", default="", help="root of a LongSom checkout: time its sampler too")
    ap.add_argument("--sm_prob", type=float, default=0.0); ap.add_argument("--sm_steps", type=int, default=3)
    ap.add_argument("--eup", type=float, default=0.0, help="the share of the steps that update the error rates (device only)")
    ap.add_argument("--no_device", action="store_true"); ap.add_argument("--late_only", action="store_true", help="50 steps only: what a profiler should see")
    ap.add_argument("--lugsail", action="store_true", help="time a PSRF check and a 200-step extension at 1 000 and 10 000 recorded steps, and nothing else")
    a = ap.parse_args()
    data, truth = planted(a.cells, a.muts, a.clusters)
    out = {"cells": a.cells, "muts": a.muts, "clusters": a.clusters, "chains": a.chains, "cpus": os.cpu_count()}
    if a.lugsail:
        out["lugsail"] = lugsail(data, a.chains)
        print(json.dumps(out))
        return
    if not a.no_device:
        out["sm_prob"], out["sm_steps"], out["eup"] = a.sm_prob, a.sm_steps, a.eup
        out["device"] = device(data, a.chains, a.late_only, a.sm_prob, a.sm_steps, a.eup)
    if a.reference:
        out["reference"] = reference(a.reference, data, truth, a.chains, a.sm_prob, a.sm_steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
