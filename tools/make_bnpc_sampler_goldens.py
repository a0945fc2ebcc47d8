#!/usr/bin/env python3
"""BnpC sampler goldens: RUN the reference's own scripts/CellClustering/libs/CRP.py and libs/MCMC.py (unmodified, imported from the tree
given by --reference, no bytecode written) on states written here as data, and commit what their methods return.  bottleneck and seaborn
get the stand-ins of tools/make_bnpc_estimate_goldens.py where they are not installed.

Under tests/golden/:
  bnpcs.fixture.npz               data [60][40] (NaN = missing) and truth [60]: 3 planted clusters with truth = i % 3, FN 0.1, FP 0.01, 20 %
                                  missing.  Asserted here: the reference's sampler with sm_prob = 0 (seed 1, 300 steps, burn-in 100) and its
                                  posterior estimate give back the planted partition.
  bnpcs.fixture.BinaryMatrix.tsv  the same matrix as run_BnpC.py reads it (mutations x cells, 3 = missing)
  bnpcs.states.npz                per case <c> the arrays <c>.*: the state (data, labels, theta, alpha, FN, FP, pp, ap) and what the methods
                                  of a CRP in that state return: mix (_beta_mix_const), dp_gamma (DP_a_gamma), alpha0 (the initial DP_a),
                                  crp_prior (CRP_prior), new_post (get_lpost_single_new_cluster), lpost [N][K] / lpost_ids [N][K]
                                  (get_lpost_single of every cell after its removal, NaN / -1 padded), probs [N][K + 1]
                                  (_normalize_log_probs of those with the new cluster's appended), mh_new, mh_sd, mh_A [K][M] (_get_log_A of
                                  given proposals per live cluster), ll_full, lprior_full
Cases: 12 cells x 9 mutations with an all-missing cell, an all-missing column and a one-cell cluster, under pp (1, 1) and (0.25, 0.25) and
under a negative and a given -ap.
"""
import argparse
import contextlib
import copy
import io
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import pandas as pd          # noqa: F401  (before the stand-ins)

from make_bnpc_estimate_goldens import stand_ins

TMIN = 1e-5


def fixture():
    rng = np.random.default_rng(20261018)
    N, M, K = 60, 40, 3
    truth = np.arange(N) % K
    proto = rng.random((K, M)) < 0.5
    g = proto[truth]
    data = g.astype(float)
    fn = g & (rng.random((N, M)) < 0.1)
    fp = ~g & (rng.random((N, M)) < 0.01)
    data[fn] = 0
    data[fp] = 1
    data[rng.random((N, M)) < 0.2] = np.nan
    return data, truth


def same_partition(a, b):
    return len(set(zip(a, b))) == len(set(a)) == len(set(b))


def check_fixture(CRP, MCMC, ut, data, truth):
    model = CRP.CRP(data, DP_alpha=[-1, -1], param_beta=[1, 1], FN_error=0.1, FP_error=0.01)
    mcmc = MCMC(model, sm_prob=0, dpa_prob=0.5, error_prob=0, sm_ratios=[0.75, 0.25], sm_steps=3)
    with contextlib.redirect_stdout(io.StringIO()):
        mcmc.run((300, 100), 1, 1, 0, "", True)
    cat = ut._concat_chain_results(mcmc.get_results())
    est = ut._get_latents_posterior_chain(cat, data)
    assert same_partition(est["assignment"], truth), "the reference's sampler with sm_prob = 0 does not recover the fixture at seed 1"
    print("fixture: the reference's sampler (sm_prob 0, seed 1) recovers the planted partition")


def state_case(CRP, rng, pp, ap):
    N, M = 12, 9
    data = (rng.random((N, M)) < 0.5).astype(float)
    data[rng.random((N, M)) < 0.2] = np.nan
    data[3] = np.nan                                                  # an all-missing cell
    data[:, 4] = np.nan                                               # an all-missing column
    labels = np.array([0, 0, 2, 2, 5, 0, 2, 7, 7, 0, 2, 7])           # cluster 5 has one cell; ids with gaps
    FN, FP = 0.15, 0.02
    model = CRP.CRP(data, DP_alpha=ap, param_beta=pp, FN_error=FN, FP_error=FP)
    gold = {"data": data, "labels": labels, "FN": FN, "FP": FP, "pp": np.array(pp, float), "ap": np.array(ap, float),
            "mix": model._beta_mix_const, "dp_gamma": np.array(model.DP_a_gamma, float), "alpha0": np.float64(model.DP_a)}
    theta = np.zeros((N, M), np.float32)
    live = np.unique(labels)
    theta[live] = np.clip(rng.random((len(live), M)), TMIN, 1 - TMIN).astype(np.float32)
    theta[0, 0], theta[2, 1] = np.float32(TMIN), np.float32(1 - TMIN)
    alpha = 5.75
    model.assignment = labels.copy()
    model.parameters = theta.copy()
    model.cells_per_cluster = {int(k): int((labels == k).sum()) for k in live}
    model.DP_a = alpha
    model.init_DP_prior()
    gold.update(theta=theta, alpha=np.float64(alpha), crp_prior=model.CRP_prior, new_post=model.get_lpost_single_new_cluster())
    K = len(live)
    lpost = np.full((N, K), np.nan); ids = np.full((N, K), -1); probs = np.full((N, K + 1), np.nan)
    for i in range(N):
        m = copy.deepcopy(model)
        old = m.assignment[i]
        if m.cells_per_cluster[old] == 1:
            del m.cells_per_cluster[old]
        else:
            m.cells_per_cluster[old] -= 1
        cl = np.fromiter(m.cells_per_cluster.keys(), dtype=int)
        post = m.get_lpost_single(i, cl)
        lpost[i, :len(cl)] = post; ids[i, :len(cl)] = cl
        probs[i, :len(cl) + 1] = m._normalize_log_probs(np.append(post, gold["new_post"][i]))
    gold.update(lpost=lpost, lpost_ids=ids, probs=probs)
    mh_new = np.zeros((K, M), np.float32); mh_sd = np.zeros((K, M)); mh_A = np.zeros((K, M))
    for j, k in enumerate(live):
        old = model.parameters[k]
        sd = rng.choice(model.param_proposal_sd, size=M)
        new = np.clip(old + sd * rng.standard_normal(M) * 0.5, TMIN, 1 - TMIN).astype(np.float32)
        a, b = (TMIN - old) / sd, ((1 - TMIN) - old) / sd
        mh_new[j], mh_sd[j] = new, sd
        mh_A[j] = model._get_log_A(new, old, np.argwhere(labels == k).flatten(), a, b, sd, False)
    gold.update(mh_new=mh_new, mh_sd=mh_sd, mh_A=mh_A, ll_full=np.float64(model.get_ll_full()), lprior_full=np.float64(model.get_lprior_full()))
    return gold


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a LongSom checkout (the directory that holds workflow/)")
    a = ap.parse_args()
    stand_ins()
    sys.path.insert(0, os.path.join(a.reference, "workflow", "scripts", "CellClustering"))
    import libs.CRP as CRP
    import libs.utils as ut
    from libs.MCMC import MCMC
    import scipy
    print("numpy", np.__version__, "scipy", scipy.__version__)
    data, truth = fixture()
    check_fixture(CRP, MCMC, ut, data, truth)
    np.savez_compressed(os.path.join(OUT, "bnpcs.fixture.npz"), data=data, truth=truth)
    frame = pd.DataFrame(np.where(np.isnan(data), 3, data).astype(int).T, index=["chr1:%d:A:T" % (100 + m) for m in range(data.shape[1])],
                         columns=["cell%02d" % i for i in range(data.shape[0])])
    frame.to_csv(os.path.join(OUT, "bnpcs.fixture.BinaryMatrix.tsv"), sep="\t")
    rng = np.random.default_rng(7)
    arrays = {}
    for name, pp, dpa in (("uniform_neg", [1, 1], [-1, -1]), ("quarter_given", [.25, .25], [0.001, 5.0]), ("uniform_given", [1, 1], [2.0, 0.5]),
                          ("quarter_neg", [.25, .25], [-1, -1])):
        for k, v in state_case(CRP, rng, pp, dpa).items():
            arrays["%s.%s" % (name, k)] = np.asarray(v)
        print("case", name, "ll_full", arrays[name + ".ll_full"], "lprior_full", arrays[name + ".lprior_full"])
    np.savez_compressed(os.path.join(OUT, "bnpcs.states.npz"), **arrays)


if __name__ == "__main__":
    main()
