#!/usr/bin/env python3
"""Goldens of BnpC's split-merge move: RUN the reference's own scripts/CellClustering/libs/CRP.py (unmodified, imported from the tree given
by --reference, no bytecode written; libs.MCMC is imported too, so that its np.seterr is in force: the log(|S| - 1) fallback depends on it)
on states written here as data, and commit what its methods return.  bottleneck gets the stand-in of tools/make_bnpc_estimate_goldens.py.

Where a method draws, numpy's global generator is seeded, the method run, the generator seeded again and the draws REPLAYED in the method's
own order; they are stored as data beside the method's result, and the twin's functions (longsom_amd.bnpc_sampler) are fed them.

tests/golden/bnpcs.sm.npz holds, per state <c> and move <v>, the arrays <c>.<v>.*:
  kind (0 split, 1 merge), cl (the clusters), cells (i, S ascending, j)                        the move
  launch_assign, launch_rows [3][M]     _rg_init_split's assignment and rows 0, 1; _init_cl_params_new(cells) as row 2 (the Beta draws are data)
  cell_ll [|S|][2]                      _rg_get_ll(S, rows 0 and 1)
  scan_perm, scan_us, scan_assign, scan_prob     one _rg_scan_assign(trans_prob=True) from the launch assignment: the permutation, the uniform
                                        of every position of S, the assignment after it and the returned sum (absent when S is empty)
  mh_sd, mh_new, mh_lv [3][M]           per row one MH_cluster_params(trans_prob=True): the replayed sds, proposals and ln(uniforms), and
  mh_A [3][M], mh_row [3][M], mh_sum [3]    _get_log_A(clip=True) of those proposals, the row it returns, and its sum of A with log(-expm1(A))
  rev_sd [M], rev_sum                   a split's reverse probability: sum of _get_log_A(parameters[cluster], row 2, clip=True)
  lprior, ll_ratio, size_ratio          _get_lprior_ratio_*, _get_ll_ratio, _get_ltrans_prob_size_ratio_* of the move's kind, in the state
                                        the reference evaluates them in (a merge: after _rg_get_split_prob)
  split_sd [2][M], split_prob           a merge's _rg_get_split_prob and its replayed sds
  size_data, size_rest                  do_split_move's (ltrans_prob_size, the other clusters' sizes) / do_merge_move's cluster_size_data, caught
                                        as the method hands them to run_rg_nc
  refused                               a split: np.unique(rg_assignment).size == 1 after the scan
  done_*                                an accepted move of the kind as the reference applies it (the seed is searched until do_*_move accepts):
                                        done_cl, done_cells, done_assign, done_rows, and after it done_labels, done_ids, done_sizes, done_theta
and per state <c>.data, labels, theta, alpha, FN, FP, pp, ap.
States: the 12 x 9 layout of tools/make_bnpc_sampler_goldens.py's state_case under its four prior cases (an all-missing cell, an all-missing
column, a one-cell cluster, ids with gaps, theta touching TMIN and TMAX; one move has the all-missing cell as an anchor), and the small ends:
N = 2 with K = 1 and with K = 2 (S empty; the merge meets log(-1)), a merge with |S| = 1 (log 0), a split that ends one-sided (refused).

Asserted here: the reference's sampler with sm_prob = 0.33 (seed 1, 300 steps, burn-in 100) recovers the 60 x 40 fixture of
tests/golden/bnpcs.fixture.npz.
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
from make_bnpc_sampler_goldens import same_partition

TMIN = 1e-5
TMAX = 1 - TMIN


def put_state(CRP, data, labels, theta, alpha, pp, ap, FN, FP):
    model = CRP.CRP(data, DP_alpha=ap, param_beta=pp, FN_error=FN, FP_error=FP)
    model.assignment = np.array(labels)
    model.parameters = theta.copy()
    model.cells_per_cluster = {int(k): int((labels == k).sum()) for k in np.unique(labels)}
    model.DP_a = alpha
    model.init_DP_prior()
    return model


def layout_state(CRP, rng, pp, ap):
    """state_case's layout"""
    N, M = 12, 9
    data = (rng.random((N, M)) < 0.5).astype(float)
    data[rng.random((N, M)) < 0.2] = np.nan
    data[3] = np.nan
    data[:, 4] = np.nan
    labels = np.array([0, 0, 2, 2, 5, 0, 2, 7, 7, 0, 2, 7])
    theta = np.zeros((N, M), np.float32)
    live = np.unique(labels)
    theta[live] = np.clip(rng.random((len(live), M)), TMIN, TMAX).astype(np.float32)
    theta[0, 0], theta[2, 1] = np.float32(TMIN), np.float32(TMAX)
    return data, labels, theta, 5.75


def small_state(rng, name):
    M = 5
    if name == "n2k1":
        return np.array([[1, 0, np.nan, 1, 0], [0, 0, 1, np.nan, 1]], float), np.array([1, 1])
    if name == "n2k2":
        return np.array([[1, 0, np.nan, 1, 0], [0, 0, 1, np.nan, 1]], float), np.array([0, 1])
    if name == "s1":
        return np.array([[1, 0, np.nan, 1, 0], [1, 1, 1, np.nan, 1], [0, 0, 1, 0, 1]], float), np.array([0, 0, 2])
    data = np.ones((5, 9))                                            # one_sided: the cells of S are the i anchor's twins, j is its opposite
    data[4] = 0
    return data, np.zeros(5, int)


def cells_of(labels, kind, cl, i, j):
    members = np.nonzero(np.isin(labels, cl))[0]
    S = members[(members != i) & (members != j)]
    return np.concatenate([[i], S, [j]]).astype(int)


def catch_size_data(model, kind, cl, scans=3):
    """do_*_move's size_data for the clusters cl: the move is run under seeds until it chooses them, with run_rg_nc caught"""
    for seed in range(1, 100000):
        m = copy.deepcopy(model)
        got = []
        m.run_rg_nc = lambda move, cells, size_data, scan_no: got.append((cells.copy(), size_data)) or ((False, [], []) if move == "split" else (False, []))
        np.random.seed(seed)
        (m.do_split_move if kind == 0 else m.do_merge_move)(scans)
        cells, size_data = got[0]
        if kind == 0 and m.assignment[cells[0]] == cl[0]:
            return size_data
        if kind == 1 and m.assignment[cells[0]] == cl[0] and m.assignment[cells[-1]] == cl[1]:
            return size_data
    raise AssertionError("no seed chooses the clusters %r" % (cl,))


def accepted_move(model, kind, scans=3):
    """the first seed under which do_*_move accepts: what run_rg_nc got and returned, and the state after it"""
    for seed in range(1, 100000):
        m = copy.deepcopy(model)
        got = []
        inner = m.run_rg_nc

        def through(move, cells, size_data, scan_no):
            before = m.assignment.copy()
            r = inner(move, cells, size_data, scan_no)
            got.append((cells.copy(), before, r))
            return r
        m.run_rg_nc = through
        np.random.seed(seed)
        if (m.do_split_move if kind == 0 else m.do_merge_move)(scans) == [1, 0]:
            cells, before, r = got[0]
            ids = np.array(sorted(m.cells_per_cluster), int)
            out = {"done_cl": np.array([before[cells[0]], before[cells[-1]]]), "done_cells": cells,
                   "done_assign": np.asarray(r[1], int) if kind == 0 else np.zeros(0, int),
                   "done_rows": np.asarray(r[2] if kind == 0 else r[1], np.float32), "done_labels": m.assignment.copy(), "done_ids": ids,
                   "done_sizes": np.array([m.cells_per_cluster[k] for k in ids], int), "done_theta": m.parameters.copy()}
            return out
    raise AssertionError("no seed accepts the move")


def record(model, rng, kind, cl, i, j):
    M = model.muts_total
    m = copy.deepcopy(model)
    cells = cells_of(m.assignment, kind, cl, i, j)
    S = cells[1:-1]
    g = {"kind": np.int64(kind), "cl": np.array(cl, int), "cells": cells}
    np.random.seed(int(rng.integers(1, 2 ** 31)))
    m._rg_init_split(cells)
    m.rg_params_merge = m._init_cl_params_new(cells)
    m.rg_assignment = np.asarray(m.rg_assignment)
    g["launch_assign"] = m.rg_assignment.astype(int)
    g["launch_rows"] = np.concatenate([m.rg_params_split, m.rg_params_merge[None, :]]).astype(np.float32)
    g["cell_ll"] = np.asarray(m._rg_get_ll(S, m.rg_params_split)).reshape(len(S), 2)
    if len(S):
        seed = int(rng.integers(1, 2 ** 31))
        np.random.seed(seed)
        g["scan_prob"] = np.float64(m._rg_scan_assign(cells, True))
        g["scan_assign"] = m.rg_assignment.astype(int)
        np.random.seed(seed)
        perm = np.random.permutation(len(S))
        us = np.zeros(len(S))
        for pos in perm:
            us[pos] = np.random.random()
        g["scan_perm"], g["scan_us"] = perm, us
    side = [np.append(S[m.rg_assignment == 0], cells[0]).astype(int), np.append(S[m.rg_assignment == 1], cells[-1]).astype(int), cells]
    rows = g["launch_rows"]
    from scipy.stats import truncnorm
    sds, news, lvs, As, after, sums = (np.zeros((3, M)) for _ in range(6))
    for r in range(3):
        seed = int(rng.integers(1, 2 ** 31))
        np.random.seed(seed)
        after[r], sums[r, 0], _ = m.MH_cluster_params(rows[r], side[r], True)
        np.random.seed(seed)
        std = np.random.choice(m.param_proposal_sd, size=M)
        a, b = (TMIN - rows[r]) / std, (TMAX - rows[r]) / std
        new = truncnorm.rvs(a, b, loc=rows[r], scale=std, size=M).astype(np.float32)
        sds[r], news[r], lvs[r] = std, new, np.log(np.random.random(M))
        As[r] = m._get_log_A(new, rows[r], side[r], a, b, std, True)
    g.update(mh_sd=sds, mh_new=news.astype(np.float32), mh_lv=lvs, mh_A=As, mh_row=after.astype(np.float32), mh_sum=sums[:, 0].copy())
    size_data = catch_size_data(model, kind, cl)
    if kind == 0:
        g["size_data"], g["size_rest"] = np.float64(size_data[0][0]), np.asarray(size_data[1], int)
        std = rng.choice(m.param_proposal_sd, size=M)
        a, b = (TMIN - m.rg_params_merge) / std, (TMAX - m.rg_params_merge) / std
        g["rev_sd"] = std
        g["rev_sum"] = np.float64(np.nansum(m._get_log_A(m.parameters[cl[0]], m.rg_params_merge, cells, a, b, std, True)))
        g["lprior"] = np.float64(m._get_lprior_ratio_split(cells))
        g["ll_ratio"] = np.float64(m._get_ll_ratio(cells, "split"))
        g["size_ratio"] = np.float64(m._get_ltrans_prob_size_ratio_split(*size_data))
        g["refused"] = np.bool_(np.unique(m.rg_assignment).size == 1)
    else:
        g["size_data"] = np.float64(size_data)
        seed = int(rng.integers(1, 2 ** 31))
        np.random.seed(seed)
        g["split_prob"] = np.float64(m._rg_get_split_prob(cells))
        np.random.seed(seed)
        g["split_sd"] = np.random.choice(m.param_proposal_sd, size=(2, M))
        g["lprior"] = np.float64(m._get_lprior_ratio_merge(cells))
        g["ll_ratio"] = np.float64(m._get_ll_ratio(cells, "merge"))
        g["size_ratio"] = np.float64(m._get_ltrans_prob_size_ratio_merge(size_data))
    return g


def check_fixture(CRP, MCMC, ut):
    with np.load(os.path.join(OUT, "bnpcs.fixture.npz")) as z:
        data, truth = z["data"], z["truth"]
    model = CRP.CRP(data, DP_alpha=[-1, -1], param_beta=[1, 1], FN_error=0.1, FP_error=0.01)
    mcmc = MCMC(model, sm_prob=0.33, dpa_prob=0.5, error_prob=0, sm_ratios=[0.75, 0.25], sm_steps=3)
    with contextlib.redirect_stdout(io.StringIO()):
        mcmc.run((300, 100), 1, 1, 0, "", True)
    cat = ut._concat_chain_results(mcmc.get_results())
    est = ut._get_latents_posterior_chain(cat, data)
    assert same_partition(est["assignment"], truth), "the reference's sampler with sm_prob = 0.33 does not recover the fixture at seed 1"
    print("fixture: the reference's sampler (sm_prob 0.33, seed 1) recovers the planted partition")


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
    check_fixture(CRP, MCMC, ut)
    rng = np.random.default_rng(11)
    arrays = {}

    def state(name, model, moves, done=()):
        arrays.update({"%s.data" % name: model.data, "%s.labels" % name: model.assignment, "%s.theta" % name: model.parameters,
                       "%s.alpha" % name: np.float64(model.DP_a), "%s.FN" % name: np.float64(model.FN), "%s.FP" % name: np.float64(model.FP),
                       "%s.pp" % name: np.array([model.p, model.q], float), "%s.ap" % name: np.array(model.ap_given, float)})
        for move, (kind, cl, i, j) in moves.items():
            g = record(model, rng, kind, cl, i, j)
            if move in done:
                g.update(accepted_move(model, kind))
            for k, v in g.items():
                arrays["%s.%s.%s" % (name, move, k)] = np.asarray(v)
            print(name, move, "lprior", g["lprior"], "ll_ratio", g["ll_ratio"], "size_ratio", g["size_ratio"], "refused", g.get("refused"))

    for name, pp, dpa in (("uniform_neg", [1, 1], [-1, -1]), ("quarter_given", [.25, .25], [0.001, 5.0]), ("uniform_given", [1, 1], [2.0, 0.5]),
                          ("quarter_neg", [.25, .25], [-1, -1])):
        data, labels, theta, alpha = layout_state(CRP, rng, pp, dpa)
        model = put_state(CRP, data, labels, theta, alpha, pp, dpa, 0.15, 0.02)
        model.ap_given = dpa
        state(name, model, {"split0": (0, [0], 9, 1), "split_missing": (0, [2], 3, 10),          # cell 3 is the all-missing one
                            "merge27": (1, [2, 7], 6, 8), "merge50": (1, [5, 0], 4, 5), "merge_missing": (1, [7, 2], 11, 3)},
              done=("split0", "merge27"))
    for name, pp in (("n2k1", [1, 1]), ("n2k2", [.25, .25]), ("s1", [.25, .25]), ("one_sided", [1, 1])):
        data, labels = small_state(rng, name)
        theta = np.zeros(data.shape, np.float32)
        live = np.unique(labels)
        theta[live] = np.clip(rng.random((len(live), data.shape[1])), TMIN, TMAX).astype(np.float32)
        model = put_state(CRP, data, labels, theta, 2.5, pp, [2.0, 0.5], 0.15, 0.02)
        model.ap_given = [2.0, 0.5]
        moves = {"n2k1": {"split": (0, [1], 1, 0)}, "n2k2": {"merge": (1, [1, 0], 1, 0)}, "s1": {"merge": (1, [2, 0], 2, 1)},
                 "one_sided": {"split": (0, [0], 0, 4)}}[name]
        state(name, model, moves)
    assert arrays["one_sided.split.refused"] and not arrays["n2k1.split.refused"]
    np.savez_compressed(os.path.join(OUT, "bnpcs.sm.npz"), **arrays)
    print("wrote", len(arrays), "arrays,", os.path.getsize(os.path.join(OUT, "bnpcs.sm.npz")), "bytes")


if __name__ == "__main__":
    main()
