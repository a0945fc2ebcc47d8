#!/usr/bin/env python3
"""BnpC posterior-estimate goldens: RUN the reference's own scripts/CellClustering/libs/utils.py and libs/dpmmIO.py (unmodified, imported
from the tree given by --reference, no bytecode written) on chains written here as data, and commit what they return and write.

The reference imports bottleneck and seaborn.  Where they are not installed this tool supplies stand-ins: bottleneck's nansum, nanargmax,
nanmean, nanvar, move_std and replace restated in numpy, seaborn as an empty module.  They are registered AFTER pandas is imported
(pandas adopts a module named bottleneck for its own reductions otherwise).

Per case, under tests/golden/:
  bnpcest.<case>.chains.npz     the chains, in longsom_amd.bnpc.save_chains' layout (the input of every test)
  bnpcest.<case>.npz            data (cells x mutations, NaN = missing), forced (the final assignment the case forces, or empty), and
                                what the reference made of the chains: concat_* (_concat_chain_results), D, dist (get_dist),
                                n_range, scores (_calc_MPEAR of every cut), best_n, assignment (_get_MPEAR), params (the transposed
                                unique columns of get_mean_hierarchy_assignment's frame), genotypes, a, FN, FP, FN_geno, FP_geno
                                (_get_latents_posterior_chain), branch and n_used (stated here: which of utils.py:157-189's paths
                                each cluster took), rows (the chains argument save_errors / save_assignments were given)
  bnpcest.<case>.assignment.txt, .errors.txt, .genotypes.tsv, .genotypes_cont.tsv (where the reference writes one)
                                save_assignments, save_errors, save_geno (dpmmIO.py:464-521)

Cases: generated chains (K planted clusters, every sample relabelled through a random injection into [0, N), a `noise` share of the cells
moved to a random one of K + 3 clusters, or of N where that is fewer) at N in {2, 3, 63, 64, 65, 130} and S in {1, 2, 33, 257}; every cell alone in every sample; all
cells together; forced final assignments (one-cell clusters, a single cluster, all cells separate: ut._get_MPEAR replaced at run time by a
function returning it); and, if the reference's sampler runs here, real chains (MCMC.run(..., debug=True) per seed).

Asserted on every case (conditions on the inputs): the best and second-best MPEAR scores differ by >= 1e-6; no mean parameter of a
branch-2 cluster lies within 1e-9 of 0.5 or, times 1e4, within 1e-6 of a rounding tie.  Across the set every branch 0-3 occurs.
"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import numpy as np
import pandas as pd          # before the stand-ins below


def stand_ins():
    try:
        import bottleneck  # noqa: F401
    except ImportError:
        bn = types.ModuleType("bottleneck")

        def move_std(a, window, axis=-1):
            a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)
            out = np.full(a.shape, np.nan)
            for k in range(window - 1, a.shape[-1]):
                out[..., k] = np.std(a[..., k - window + 1:k + 1], axis=-1)
            return np.moveaxis(out, -1, axis)

        def replace(a, old, new):
            if isinstance(old, float) and np.isnan(old):
                a[np.isnan(a)] = new
            else:
                a[a == old] = new
        bn.nansum, bn.nanargmax, bn.nanmean, bn.nanvar, bn.move_std, bn.replace = np.nansum, np.nanargmax, np.nanmean, np.nanvar, move_std, replace
        sys.modules["bottleneck"] = bn
    try:
        import seaborn  # noqa: F401
    except ImportError:
        sys.modules["seaborn"] = types.ModuleType("seaborn")


def generated(rng, N, S, K, noise, M, chains=1, burn_in=0):
    """chains of S kept samples in all (split over `chains`, each with `burn_in` leading steps that carry no parameters)"""
    truth = rng.integers(0, K, N)
    data = (rng.random((N, M)) < 0.5).astype(float)
    data[rng.random((N, M)) < 0.2] = np.nan
    per = [S // chains + (1 if i < S % chains else 0) for i in range(chains)]
    out = []
    for n in per:
        steps = n + burn_in
        assign = np.zeros((steps, N), dtype=int)
        blocks = []
        for s in range(steps):
            lab = truth.copy()
            move = rng.random(N) < noise
            inj = rng.permutation(N)[:K + 3]
            lab[move] = rng.integers(0, len(inj), int(move.sum()))
            assign[s] = inj[lab]
            if s >= burn_in:
                k = len(np.unique(assign[s]))
                blocks.append(rng.random((k, M)).astype(np.float32))
        k_max = max(b.shape[0] for b in blocks)
        params = np.zeros((n, k_max, M), np.float32)
        for s, b in enumerate(blocks):
            params[s, :b.shape[0]] = b
        out.append({"assignments": assign, "params": params, "DP_alpha": rng.random(steps) * 3, "FN": rng.random(steps) * 0.3, "FP": rng.random(steps) * 0.01,
                    "ML": -rng.random(steps) * 100, "MAP": -rng.random(steps) * 100, "burn_in": burn_in})
    return out, data


def fixed(rng, assign, M):
    """one chain whose samples are given"""
    assign = np.asarray(assign, dtype=int)
    S, N = assign.shape
    k_max = max(len(np.unique(a)) for a in assign)
    params = np.zeros((S, k_max, M), np.float32)
    for s, a in enumerate(assign):
        k = len(np.unique(a))
        params[s, :k] = rng.random((k, M)).astype(np.float32)
    data = (rng.random((N, M)) < 0.5).astype(float)
    data[rng.random((N, M)) < 0.2] = np.nan
    return [{"assignments": assign, "params": params, "DP_alpha": rng.random(S) * 3, "FN": rng.random(S) * 0.3, "FP": rng.random(S) * 0.01,
             "ML": -rng.random(S) * 100, "MAP": -rng.random(S) * 100, "burn_in": 0}], data


def real_chains(ref_dir, rng):
    """the reference's sampler in-process: 3 chains x 60 steps over 30 cells x 12 mutations"""
    import libs.CRP_learning_errors as CRP
    from libs.MCMC import MCMC
    truth = rng.integers(0, 3, 30)
    proto = rng.random((3, 12)) < 0.5
    data = proto[truth].astype(float)
    flip = rng.random(data.shape) < 0.1
    data[flip] = 1 - data[flip]
    data[rng.random(data.shape) < 0.15] = np.nan
    results = []
    for seed in (11, 12, 13):
        model = CRP.CRP_errors_learning(data, DP_alpha=[-1, -1], param_beta=[.25, .25], FP_mean=0.01, FP_sd=0.01, FN_mean=0.2, FN_sd=0.1)
        mcmc = MCMC(model, sm_prob=0.33, dpa_prob=0.25, error_prob=0.25, sm_ratios=[0.75, 0.25], sm_steps=3)
        with contextlib.redirect_stdout(io.StringIO()):
            mcmc.run((60, 20), seed, 1, 0, "", True)
        results.extend(mcmc.get_results())
    return results, data


def branches(assignments, assign):
    """which path of utils.py:157-189 each cluster of `assign` takes, and over how many samples: stated with sets, one sample at a time"""
    S = assignments.shape[0]
    out_b, out_n = [], []
    for c in np.unique(assign):
        inside = np.nonzero(assign == c)[0]; outside = np.nonzero(assign != c)[0]
        same = [len(set(a[inside])) == 1 for a in assignments]
        both = [sm and a[inside[0]] not in set(a[outside]) for sm, a in zip(same, assignments)]
        b = 0 if any(both) else 1 if any(same) else 2
        out_n.append(sum(both) if any(both) else sum(same) if any(same) else S)
        out_b.append(3 if len(inside) == 1 else b)
    return np.array(out_b, np.uint8), np.array(out_n, np.int32)


def run_case(ut, dio, name, results, data, forced, rows, work):
    from longsom_amd import bnpc
    bnpc.save_chains(os.path.join(OUT, "bnpcest.%s.chains.npz" % name), results)
    cat = ut._concat_chain_results(results)
    A, P = cat["assignments"], cat["params"]
    S, N = A.shape
    gold = {"data": data, "forced": np.asarray(forced if forced is not None else [], dtype=np.int64), "rows": np.int64(rows)}
    for k in ("assignments", "params", "DP_alpha", "FN", "FP", "ML", "MAP"):
        gold["concat_" + k] = cat[k]
    dist = ut.get_dist(A)
    gold["dist"] = dist
    gold["D"] = np.rint(dist * S).astype(np.uint32)
    assert np.array_equal(gold["D"] / S, dist)
    real_mpear = ut._get_MPEAR
    if forced is None:
        Z = ut.linkage(dist, method="ward")
        avg = np.mean([len([i for i in zip(*np.unique(a, return_counts=True)) if i[1] > 2]) for a in A])
        n_range = np.arange(max(2, avg * 0.2), min(avg * 2.5, A.shape[1]), dtype=int)
        scores = np.array([ut._calc_MPEAR(1 - dist, ut.cut_tree(Z, n_clusters=n).flatten()) for n in n_range])
        assign = real_mpear(A)
        order = np.sort(scores)[::-1]
        assert len(order) < 2 or order[0] - order[1] >= 1e-6, "%s: best and second-best MPEAR %r" % (name, order[:2])
        gold.update(n_range=n_range, scores=scores, best_n=np.int64(n_range[int(np.argmax(scores))]))
        assert np.array_equal(assign, ut.cut_tree(Z, n_clusters=int(gold["best_n"])).flatten())
    else:
        ut._get_MPEAR = lambda assignments: np.asarray(forced)
        gold.update(n_range=np.zeros(0, np.int64), scores=np.zeros(0), best_n=np.int64(-1))
    try:
        assign2, geno = ut.get_mean_hierarchy_assignment(A, P)
        latents = ut._get_latents_posterior_chain(cat, data)
    finally:
        ut._get_MPEAR = real_mpear
    if forced is None:
        assert np.array_equal(assign2, assign)
    assign = np.asarray(assign2)
    clusters = np.unique(assign)
    first = [int(np.nonzero(assign == c)[0][0]) for c in clusters]
    params = geno.values.T[first]                                     # one row per cluster, ascending
    br, nu = branches(A, assign)
    for k in np.nonzero(br == 2)[0]:
        assert np.abs(params[k] - 0.5).min() > 1e-9, "%s: a branch-2 mean within 1e-9 of 0.5" % name
        frac = params[k] * 1e4 - np.floor(params[k] * 1e4)
        assert np.abs(frac - 0.5).min() > 1e-6, "%s: a branch-2 mean x 1e4 within 1e-6 of a rounding tie" % name
    gold.update(assignment=assign, params=params, branch=br, n_used=nu, genotypes=latents["genotypes"].values, a=np.array(latents["a"]), FN=np.array(latents["FN"]),
                FP=np.array(latents["FP"]), FN_geno=np.float64(latents["FN_geno"]), FP_geno=np.float64(latents["FP_geno"]))
    assert np.array_equal(latents["genotypes"].values, geno.values)
    np.savez_compressed(os.path.join(OUT, "bnpcest.%s.npz" % name), **gold)
    # the three files
    out_dir = os.path.join(work, name)
    os.makedirs(out_dir)
    args = types.SimpleNamespace(estimator=["posterior"], chains=rows)
    inferred = {"mean": {"posterior": latents}}
    dio.save_errors(inferred, args, out_dir)
    dio.save_assignments(inferred, args, out_dir)
    dio.save_geno(inferred, out_dir, np.array(["m%02d" % i for i in range(data.shape[1])]))
    for src, dst in (("errors.txt", "errors.txt"), ("assignment.txt", "assignment.txt"), ("genotypes_posterior_mean.tsv", "genotypes.tsv"),
                     ("genotypes_cont_posterior_mean.tsv", "genotypes_cont.tsv")):
        if os.path.exists(os.path.join(out_dir, src)):
            shutil.copy(os.path.join(out_dir, src), os.path.join(OUT, "bnpcest.%s.%s" % (name, dst)))
    print("%-12s N %3d S %3d k_max %2d clusters %3d n %3d branch %s n_used %s" % (name, N, S, P.shape[1], len(clusters), int(gold["best_n"]), br.tolist(), nu.tolist()))
    return set(br.tolist())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a LongSom checkout (the directory that holds workflow/)")
    ap.add_argument("--no_sampler", action="store_true", help="leave the real-chains case out")
    a = ap.parse_args()
    stand_ins()
    ref_dir = os.path.join(a.reference, "workflow", "scripts", "CellClustering")
    sys.path.insert(0, ref_dir)
    import libs.utils as ut
    import libs.dpmmIO as dio
    import scipy
    print("numpy", np.__version__, "scipy", scipy.__version__, "pandas", pd.__version__)
    rng = np.random.default_rng(20261018)
    cases = []                                                        # (name, chains, data, forced final assignment, index rows)
    r, d = generated(rng, 2, 1, 1, 0.0, 3);                  cases.append(("n2s1", r, d, [0, 1], 1))
    r, d = generated(rng, 3, 2, 2, 0.3, 4);                  cases.append(("n3s2", r, d, [0, 0, 1], 1))
    r, d = generated(rng, 63, 33, 4, 0.05, 7, chains=2, burn_in=3);  cases.append(("n63s33", r, d, None, 2))
    r, d = generated(rng, 64, 257, 3, 0.08, 5, chains=3, burn_in=2); cases.append(("n64s257", r, d, None, 3))
    r, d = generated(rng, 65, 2, 4, 0.05, 6);                cases.append(("n65s2", r, d, None, 1))
    r, d = generated(rng, 130, 9, 5, 0.05, 12, chains=2, burn_in=1); cases.append(("n130s9", r, d, None, 4))
    r130 = r
    cases.append(("n130one", r130, d, [0] * 130, 1))                                      # a single cluster: no sample keeps 130 cells together
    cases.append(("n130cells", r130, d, [0] * 100 + list(range(1, 31)), 1))               # thirty one-cell clusters beside a big one
    r, d = fixed(rng, [rng.permutation(20) for _ in range(5)], 4)
    cases.append(("sep", r, d, list(range(20)), 1))                                       # every cell alone in every sample, and in the final assignment
    r, d = fixed(rng, [[int(rng.integers(0, 20))] * 20 for _ in range(5)], 4)
    cases.append(("together", r, d, None, 1))
    if not a.no_sampler:
        try:
            r, d = real_chains(ref_dir, rng)
            cases.append(("real", r, d, None, 3))
        except Exception as e:      # noqa: BLE001
            print("the reference's sampler did not run here: %s: %s" % (type(e).__name__, e))
    seen = set()
    work = tempfile.mkdtemp(prefix="bnpcest_gold_")
    try:
        for name, results, data, forced, rows in cases:
            seen |= run_case(ut, dio, name, results, data, forced, rows, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    missing = {0, 1, 2, 3} - seen
    if missing:
        sys.exit("no case reaches branch %s" % sorted(missing))


if __name__ == "__main__":
    main()
