#!/usr/bin/env python3
"""BnpC error-rate goldens: RUN the reference's own scripts/CellClustering/libs/CRP_learning_errors.py (unmodified, imported from the tree
given by --reference, no bytecode written) on states written here as data, and commit what its methods return.  bottleneck and seaborn
get the stand-ins of tools/make_bnpc_estimate_goldens.py where they are not installed.

tests/golden/bnpcs.errors.npz holds per case <c> the arrays <c>.*:
  the state           data, labels, theta, alpha, pp, priors (FP_mean, FP_sd, FN_mean, FN_sd), FP, FN (the model's current rates)
  ll_pairs, ll        get_ll_full_error(FP, FN) at listed pairs [n][2]
  prior_x, prior_fp,  FP_prior.logpdf / FN_prior.logpdf at listed values
  prior_fn
  lprior_full,        get_lprior_full() of CRP_errors_learning and of its base class in the same state: they differ by the two priors' terms
  lprior_base
  trans, trans_new,   the two truncnorm.logpdf transition terms of MH_error_rates (:87-91) at listed (old, new, std) [n][3]
  trans_old
  mh_rate, mh_std,    MH_error_rates itself (0 = 'FP', 1 = 'FN') with the module's sources of randomness (np.random.choice, truncnorm.rvs,
  mh_new, mh_v,       np.random.random) replaced for the call by functions that return the listed std, new and v; mh_accept: whether it
  mh_accept           returned the new rate.  For each (rate, std, new) the listed v lie on both sides of exp(A) where A < 0.
Cases: 2 cells x 1 mutation; 20 x 65 with an all-missing column and an all-missing cell under both prior pairs; 60 x 130 with cluster ids
that have gaps.  Prior pairs: (0.01, 0.01) / (0.2, 0.1) and (0.001, 0.0005) / (0.25, 0.05).
"""
import argparse
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
WIDE = (0.01, 0.01, 0.2, 0.1)
TIGHT = (0.001, 0.0005, 0.25, 0.05)


class Listed:
    """scipy's truncnorm for everything but rvs, which returns the listed value"""

    def __init__(self, real, value):
        self.real, self.value = real, value

    def rvs(self, *args, **kw):
        return self.value

    def __getattr__(self, name):
        return getattr(self.real, name)

    def __call__(self, *args, **kw):
        return self.real(*args, **kw)


def mh_call(mod, model, rate, std, new, v):
    """MH_error_rates(rate) with the module's three sources of randomness returning std, new and v"""
    real, choice, random = mod.truncnorm, np.random.choice, np.random.random
    mod.truncnorm, np.random.choice, np.random.random = Listed(real, new), (lambda a: std), (lambda: v)
    try:
        value, count = model.MH_error_rates(rate)
    finally:
        mod.truncnorm, np.random.choice, np.random.random = real, choice, random
    assert (value == new and count == [1, 0]) or (value == (model.FP if rate == "FP" else model.FN) and count == [0, 1])
    return value == new and count == [1, 0]


def log_A(mod, model, rate, std, new):
    """A as MH_error_rates adds it (:86-106), from the reference's own methods: only to place the listed v on both of its sides"""
    old = model.FP if rate == "FP" else model.FN
    prior = model.FP_prior if rate == "FP" else model.FN_prior
    new_p = mod.truncnorm.logpdf(new, (0 - old) / std, (1 - old) / std, loc=old, scale=std)
    old_p = mod.truncnorm.logpdf(old, (0 - new) / std, (1 - new) / std, loc=new, scale=std)
    if rate == "FP":
        new_ll, old_ll = model.get_ll_full_error(new, model.FN), model.get_ll_full_error(old, model.FN)
    else:
        new_ll, old_ll = model.get_ll_full_error(model.FP, new), model.get_ll_full_error(model.FP, old)
    return new_ll + prior.logpdf(new) - old_ll - prior.logpdf(old) + old_p - new_p


def case(mod, CRP, rng, N, M, labels, pp, priors, rates, holes):
    data = (rng.random((N, M)) < 0.5).astype(float)
    data[rng.random((N, M)) < 0.2] = np.nan
    if holes:
        data[N // 2] = np.nan                                         # an all-missing cell
        data[:, M // 3] = np.nan                                      # an all-missing column
    labels = np.asarray(labels)
    model = mod.CRP_errors_learning(data, DP_alpha=[-1, -1], param_beta=list(pp), FP_mean=priors[0], FP_sd=priors[1], FN_mean=priors[2], FN_sd=priors[3])
    live = np.unique(labels)
    theta = np.zeros((N, M), np.float32)
    theta[live] = np.clip(rng.random((len(live), M)), TMIN, 1 - TMIN).astype(np.float32)
    theta[live[0], 0] = np.float32(TMIN)
    alpha = 3.25
    model.assignment = labels.copy()
    model.parameters = theta.copy()
    model.cells_per_cluster = {int(k): int((labels == k).sum()) for k in live}
    model.DP_a = alpha
    model.init_DP_prior()
    model.FP, model.FN = rates
    gold = {"data": data, "labels": labels, "theta": theta, "alpha": np.float64(alpha), "pp": np.array(pp, float), "priors": np.array(priors, float),
            "FP": np.float64(rates[0]), "FN": np.float64(rates[1])}
    pairs = np.array([rates, (priors[0], priors[2]), (rates[0] * 0.5, rates[1]), (rates[0], rates[1] * 1.5), (1e-6, 1e-6), (0.3, 0.6), (0.999, 0.001)])
    gold["ll_pairs"], gold["ll"] = pairs, np.array([model.get_ll_full_error(fp, fn) for fp, fn in pairs])
    xs = np.array([1e-9, 1e-4, priors[0], priors[2], rates[0], rates[1], 0.5, 0.97, 1 - 1e-9])
    gold["prior_x"], gold["prior_fp"], gold["prior_fn"] = xs, model.FP_prior.logpdf(xs), model.FN_prior.logpdf(xs)
    gold["lprior_full"], gold["lprior_base"] = np.float64(model.get_lprior_full()), np.float64(CRP.CRP.get_lprior_full(model))
    trans, mh = [], []
    for e, rate in enumerate(("FP", "FN")):
        old = rates[e]
        for f in (0.5, 1.0, 1.5):
            std = priors[2 * e + 1] * f
            for step in (-0.6, -0.05, 0.02, 0.4, 1.7):
                new = old + step * std
                if not 0 < new < 1:
                    continue
                trans.append((old, new, std))
                A = float(log_A(mod, model, rate, std, new))
                edge = np.exp(min(A, 0.0))
                for v in sorted({edge * 0.5, edge * 0.98, min(edge * 1.02, 1 - 1e-12), min(edge * 4 + 1e-3, 1 - 1e-9)}):
                    if v > 0:
                        mh.append((e, std, new, v, mh_call(mod, model, rate, std, new, v)))
    trans = np.array(trans)
    gold["trans"] = trans
    gold["trans_new"] = np.array([mod.truncnorm.logpdf(n, (0 - o) / s, (1 - o) / s, loc=o, scale=s) for o, n, s in trans])
    gold["trans_old"] = np.array([mod.truncnorm.logpdf(o, (0 - n) / s, (1 - n) / s, loc=n, scale=s) for o, n, s in trans])
    mh = np.array(mh)
    gold["mh_rate"], gold["mh_std"], gold["mh_new"], gold["mh_v"], gold["mh_accept"] = mh[:, 0].astype(np.int8), mh[:, 1], mh[:, 2], mh[:, 3], mh[:, 4].astype(bool)
    return gold


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a LongSom checkout (the directory that holds workflow/)")
    a = ap.parse_args()
    stand_ins()
    sys.path.insert(0, os.path.join(a.reference, "workflow", "scripts", "CellClustering"))
    import libs.CRP as CRP
    import libs.CRP_learning_errors as mod
    import scipy
    print("numpy", np.__version__, "scipy", scipy.__version__)
    rng = np.random.default_rng(11)
    gaps = np.sort(rng.permutation(60)[:7])
    cases = {"tiny": (2, 1, [0, 0], (1, 1), WIDE, (0.02, 0.15), False),
             "holes_wide": (20, 65, np.arange(20) % 3, (1, 1), WIDE, (0.015, 0.25), True),
             "holes_tight": (20, 65, np.arange(20) % 4, (.25, .25), TIGHT, (0.0012, 0.22), True),
             "gaps": (60, 130, gaps[np.arange(60) % 7], (.25, .25), TIGHT, (0.001, 0.25), False)}
    arrays = {}
    for name, (N, M, labels, pp, priors, rates, holes) in cases.items():
        for k, v in case(mod, CRP, rng, N, M, labels, pp, priors, rates, holes).items():
            arrays["%s.%s" % (name, k)] = np.asarray(v)
        acc = arrays[name + ".mh_accept"]
        print("case", name, "ll", arrays[name + ".ll"][0], "moves", len(acc), "accepted", int(acc.sum()))
    np.savez_compressed(os.path.join(OUT, "bnpcs.errors.npz"), **arrays)


if __name__ == "__main__":
    main()
