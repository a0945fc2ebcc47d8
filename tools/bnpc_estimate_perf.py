#!/usr/bin/env python3
"""Times BnpC's posterior estimate: tools/bnpc_estimate_perf.py [cells] [samples] [clusters] [mutations]   (on the GPU)
                                    tools/bnpc_estimate_perf.py --cpu_reference DIR                        (on a CPU, no device)

On the GPU: generated chains (planted clusters, every sample relabelled through a random injection, 5 % of the cells moved; default 5000
cells, 10720 samples - 16 chains x 1000 steps after a burn-in of 0.33 - about 20 clusters, 200 mutations) are made resident, and the
device calls of the estimate are timed by a host clock around calls that end in a device synchronise, warmed up and repeated:
lsg_bnpc_codist, lsg_bnpc_cluster_counts, lsg_bnpc_linkage, lsg_bnpc_cut_tree over the candidate cuts, lsg_bnpc_mpear over them,
lsg_bnpc_mean_params of the best cut.  What the tree, the cuts and the cluster count cost on the host (scipy's linkage and cut_tree, numpy's
avg_cluster_number, and the fetch of D they need) is timed the same way beside them, in the same run, and the two sides' results are
compared.  Prints one JSON line.

--cpu_reference DIR: DIR is a LongSom checkout; its own utils.get_dist is timed at 1000 cells x 20 samples and the time per (pair, sample)
is scaled to the GPU shape.  The scaled figure is an extrapolation, and is named one."""
import json
import os
import sys
import time

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_chains(N, S, K, M, seed=3, noise=0.05):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, K, N)
    lab = np.broadcast_to(truth, (S, N)).copy()
    move = rng.random((S, N)) < noise
    lab[move] = rng.integers(0, K + 3, int(move.sum()))
    inj = np.argsort(rng.random((S, N)), axis=1)[:, :K + 3]                      # per sample, K + 3 distinct labels of [0, N)
    a = np.take_along_axis(inj, lab, axis=1).astype(np.int32)
    params = rng.random((S, K + 3, M), dtype=np.float32)
    return a, params


def timed(fn, warmup=2, repeats=5):
    for _ in range(warmup):
        out = fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); out = fn(); t.append(time.perf_counter() - t0)
    return out, {"ms_median": round(1e3 * float(np.median(t)), 3), "ms_min": round(1e3 * min(t), 3), "ms_max": round(1e3 * max(t), 3), "repeats": repeats}


def cpu_reference(ref, N=1000, S=20, at=(5000, 10720)):
    import pandas  # noqa: F401  (before the stand-ins)
    from make_bnpc_estimate_goldens import stand_ins
    stand_ins()
    sys.path.insert(0, os.path.join(ref, "workflow", "scripts", "CellClustering"))
    import libs.utils as ut
    a, _ = make_chains(N, S, 20, 1)
    a = a.astype(int)
    _, t = timed(lambda: ut.get_dist(a), warmup=1, repeats=3)
    per = t["ms_median"] * 1e-3 / (N * (N - 1) / 2 * S)
    pairs_samples = at[0] * (at[0] - 1) / 2 * at[1]
    print(json.dumps({"what": "the reference's utils.get_dist on this CPU, one thread", "cells": N, "samples": S, **t, "ns_per_pair_sample": round(per * 1e9, 3),
                      "extrapolated_to": {"cells": at[0], "samples": at[1], "pair_samples": pairs_samples, "seconds": round(per * pairs_samples, 1)}}))


def main():
    if "--cpu_reference" in sys.argv:
        return cpu_reference(sys.argv[sys.argv.index("--cpu_reference") + 1])
    from scipy.cluster.hierarchy import cut_tree, linkage
    from longsom_amd import bnpc
    from longsom_amd.engine import Engine
    args = [int(x) for x in sys.argv[1:]]
    N, S, K, M = (args + [5000, 10720, 20, 200][len(args):])[:4]
    a, params = make_chains(N, S, K, M)
    out = {"cells": N, "samples": S, "clusters": K, "mutations": M, "pair_samples": N * (N - 1) // 2 * S}
    with Engine(0) as eng:
        t0 = time.perf_counter(); eng.bnpc_load_samples(a, params); out["load_s"] = round(time.perf_counter() - t0, 3)
        _, out["codist"] = timed(lambda: eng.bnpc_codist(fetch=False))
        out["codist"]["pair_samples_per_s"] = float("%.4g" % (out["pair_samples"] / (out["codist"]["ms_median"] * 1e-3)))
        print("codist timed:", out["codist"], flush=True)
        D, out["fetch_dist"] = timed(eng.bnpc_codist, warmup=1, repeats=3)          # (codist with its fetch: the copy is the difference to "codist")
        avg, out["cluster_counts"] = timed(eng.bnpc_avg_cluster_number)
        host_avg, out["host_avg_cluster_number"] = timed(lambda: bnpc.avg_cluster_number(a), warmup=1)
        n_range = bnpc.cut_range(avg, N)
        out["cuts"] = len(n_range)
        Zd, out["linkage"] = timed(eng.bnpc_linkage)
        dcuts, out["cut_tree"] = timed(lambda: eng.bnpc_cut_tree(n_range))
        print("device tree timed:", out["linkage"], out["cut_tree"], flush=True)
        Z, out["host_linkage"] = timed(lambda: linkage(D / S, method="ward"), warmup=1)
        cuts, out["host_cut_tree"] = timed(lambda: np.ascontiguousarray(cut_tree(Z, n_clusters=list(n_range)).T), warmup=1)
        out["device_tree_and_cuts_ms"] = round(out["linkage"]["ms_median"] + out["cut_tree"]["ms_median"], 3)
        out["host_tree_and_cuts_ms"] = round(out["host_linkage"]["ms_median"] + out["host_cut_tree"]["ms_median"], 3)
        out["equal"] = {"avg_cluster_number": bool(avg == host_avg), "Z": bool(np.array_equal(Zd.view(np.uint64), Z.view(np.uint64))), "cuts": bool(np.array_equal(dcuts, cuts))}
        (pairs, sim, dsum), out["mpear"] = timed(lambda: eng.bnpc_mpear(cuts))
        scores = bnpc.mpear_scores(pairs, sim, dsum, S, N)
        best = int(np.argmax(scores))
        out["best_n"] = int(n_range[best])
        (_, branch, _), out["mean_params"] = timed(lambda: eng.bnpc_mean_params(cuts[best]))
        out["branches"] = np.bincount(branch, minlength=4).tolist()
        eng.bnpc_unload()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
