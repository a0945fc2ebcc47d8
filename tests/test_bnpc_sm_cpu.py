"""CPU: the split-merge move of the numpy twin (longsom_amd.bnpc_sampler) held to the reference's own methods.

tests/golden/bnpcs.sm.npz holds what CRP.py's split-merge methods return in given states and under replayed draws
(tools/make_bnpc_sm_goldens.py ran them, unmodified); the twin's functions take the same draws as arguments.  Integers and assignments are
exact; a sum of n terms is held within tests/test_bnpc_sampler_cpu.bound(n, sum |term|); a single log-density term within 1e-12 (the
truncated-normal test's reasoning: z^2 / 2 reaches 50 and a few ulp of that is the error to expect)."""
import os

import numpy as np
import pytest

from longsom_amd import bnpc, bnpc_sampler as bs
from tests.test_bnpc_sampler_cpu import GOLD, bound, same_partition

LAYOUT = ("uniform_neg", "quarter_given", "uniform_given", "quarter_neg")
MOVES = [(c, v) for c in LAYOUT for v in ("split0", "split_missing", "merge27", "merge50", "merge_missing")] + \
        [("n2k1", "split"), ("n2k2", "merge"), ("s1", "merge"), ("one_sided", "split")]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "bnpcs.sm.npz")) as z:
        return {k: z[k] for k in z.files}


def load_move(gold, case, move):
    s = {k[len(case) + 1:]: v for k, v in gold.items() if k.startswith(case + ".") and k.count(".") == 1}
    g = {k[len(case) + len(move) + 2:]: v for k, v in gold.items() if k.startswith("%s.%s." % (case, move))}
    model = bs.Model(s["data"], float(s["FN"]), float(s["FP"]), tuple(s["pp"]), tuple(s["ap"]))
    st = bs.State(s["labels"], s["theta"], float(s["alpha"]))
    cells = g["cells"]
    return g, model, st, int(cells[0]), int(cells[-1]), cells[1:-1]


def test_every_array_of_the_goldens_is_read(gold):
    """the names this file compares, so that an array added to the tool does not go unread"""
    per_move = {"kind", "cl", "cells", "launch_assign", "launch_rows", "cell_ll", "scan_perm", "scan_us", "scan_assign", "scan_prob", "mh_sd", "mh_new", "mh_lv", "mh_A",
                "mh_row", "mh_sum", "rev_sd", "rev_sum", "lprior", "ll_ratio", "size_ratio", "split_sd", "split_prob", "size_data", "size_rest", "refused",
                "done_cl", "done_cells", "done_assign", "done_rows", "done_labels", "done_ids", "done_sizes", "done_theta"}
    per_state = {"data", "labels", "theta", "alpha", "FN", "FP", "pp", "ap"}
    for k in gold:
        parts = k.split(".")
        assert parts[-1] in (per_state if len(parts) == 2 else per_move), k
    assert {(k.split(".")[0], k.split(".")[1]) for k in gold if k.count(".") == 2} == set(MOVES)


@pytest.mark.parametrize("case,move", MOVES)
def test_the_cells_and_the_launch_assignment(gold, case, move):
    g, model, st, i, j, S = load_move(gold, case, move)
    members = np.nonzero(np.isin(st.labels, g["cl"]))[0]
    assert np.array_equal(S, members[(members != i) & (members != j)]), "S is the move's other cells in ascending id"
    margin = bs.Margin()
    assign = bs.sm_launch_assign(model, i, j, S, margin)
    assert np.array_equal(assign, g["launch_assign"])
    if len(S):
        # the anchor likelihoods themselves: a theta of 0, 1 or mix[0] per mutation, as the reference forms it
        ll, mag, _ = bs.sm_anchor_ll(model, S, i)
        theta = np.nan_to_num(model.one[i] * 1.0 + np.where(model.one[i] | model.zero[i], 0.0, np.nan), nan=model.mix[0])
        x = np.where(model.one[S], 1.0, np.where(model.zero[S], 0.0, np.nan))
        with np.errstate(all="ignore"):
            want = np.nansum(np.log(theta * ((1 - model.FN) ** x * model.FN ** (1 - x)) + (1 - theta) * ((1 - model.FP) ** (1 - x) * model.FP ** x)), axis=1)
        assert (np.abs(ll - want) <= bound(model.M, mag)).all()


def test_an_anchor_may_be_the_all_missing_cell(gold):
    for case in LAYOUT:
        for move in ("split_missing", "merge_missing"):
            g, model, st, i, j, S = load_move(gold, case, move)
            assert min(model.pop1[i] + model.pop0[i], model.pop1[j] + model.pop0[j]) == 0


@pytest.mark.parametrize("case,move", MOVES)
def test_cell_likelihoods_and_one_scan(gold, case, move):
    g, model, st, i, j, S = load_move(gold, case, move)
    rows = g["launch_rows"]
    ll, mag = bs.sm_cell_ll(model, S, rows[:2])
    assert ll.shape == g["cell_ll"].shape
    assert (np.abs(ll - g["cell_ll"]) <= bound((model.pop1 + model.pop0)[S][:, None], mag)).all()
    if not len(S):
        assert "scan_prob" not in g
        return
    assign = g["launch_assign"].copy()
    total, tmag = bs.sm_scan_assign(g["cell_ll"], assign, len(S) + 2, st.alpha, g["scan_perm"], g["scan_us"])
    assert np.array_equal(assign, g["scan_assign"])
    # each log probability is a difference of sums of the size of ll: its error is a few ulp of |ll|, not of itself
    assert abs(total - float(g["scan_prob"])) <= bound(len(S), tmag + np.abs(g["cell_ll"]).sum())


@pytest.mark.parametrize("case,move", MOVES)
def test_parameter_moves_with_their_transition_probability(gold, case, move):
    g, model, st, i, j, S = load_move(gold, case, move)
    n1, n0 = bs.sm_row_counts(model, i, j, S, g["scan_assign"] if len(S) else g["launch_assign"])
    rows = g["launch_rows"]
    for r in range(3):
        A, mag = bs.log_A(model, g["mh_new"][r], rows[r], n1[r], n0[r], g["mh_sd"][r], terms=True, clip=True)
        n = 2 * (len(S) + 2) + 6
        assert (np.abs(A - g["mh_A"][r]) <= bound(n, mag)).all() and (A <= 0).all()
        row, total, tmag = bs.sm_param_move(model, rows[r], g["mh_new"][r], n1[r], n0[r], g["mh_sd"][r], g["mh_lv"][r])
        assert np.array_equal(row, g["mh_row"][r])
        # (tmag carries, for a declined entry, the magnitudes of A's terms times the slope of log(-expm1(.)) at A)
        assert abs(total - float(g["mh_sum"][r])) <= bound(n * model.M, tmag)


@pytest.mark.parametrize("case,move", MOVES)
def test_the_four_terms(gold, case, move):
    g, model, st, i, j, S = load_move(gold, case, move)
    kind = "split" if int(g["kind"]) == 0 else "merge"
    n, live = len(S) + 2, st.live()
    rows = g["launch_rows"]
    after_scan = g["scan_assign"] if len(S) else g["launch_assign"]
    if kind == "split":
        cl = int(g["cl"][0])
        assert abs(bs.sm_split_size_data(st.sizes, live, cl) - float(g["size_data"])) <= 8 * 2.0 ** -52 * 10
        rest = np.delete(st.sizes[live], np.searchsorted(live, cl))
        assert np.array_equal(rest, g["size_rest"])
        n1, n0 = bs.sm_row_counts(model, i, j, S, after_scan)
        A, mag = bs.log_A(model, st.theta[cl], rows[2], n1[2], n0[2], g["rev_sd"], terms=True, clip=True)
        assert abs(A.sum() - float(g["rev_sum"])) <= bound((2 * n + 6) * model.M, mag.sum())
        n_j = int(after_scan.sum()) + 1
        lp, lmag = bs.sm_lprior_ratio(model, kind, n, n_j, st.alpha, rows[:2], st.theta[[cl]])
        assert abs(bs.sm_size_ratio_split(float(g["size_data"]), rest, n, n_j) - float(g["size_ratio"])) <= bound(len(rest) + 8, 10.0)
        assert bool(g["refused"]) == (len(S) > 0 and len(np.unique(after_scan)) == 1)
    else:
        cl_i, cl_j = (int(x) for x in g["cl"])
        assert abs(bs.sm_merge_size_data(st.sizes, live, cl_i, cl_j) - float(g["size_data"])) <= bound(len(live) + 4, 20.0)
        # _rg_get_split_prob: the parameter part over the launch state's members, the walk over the original assignment
        n1, n0 = bs.sm_row_counts(model, i, j, S, after_scan)
        total, mag = 0.0, 0.0
        for r, cl in enumerate((cl_i, cl_j)):
            A, m = bs.log_A(model, st.theta[cl], rows[r], n1[r], n0[r], g["split_sd"][r], terms=True, clip=True, unit_bounds=True)
            total += A.sum(); mag += m.sum()
        original = (st.labels[S] == cl_j).astype(np.int64)
        assign = after_scan.copy()
        if len(S):
            ll, lmag = bs.sm_cell_ll(model, S, st.theta[[cl_i, cl_j]])
            pa, pmag = bs.sm_scan_assign(ll, assign, n, st.alpha, np.arange(len(S)), None, original)
            total += pa; mag += pmag + lmag.sum()
        assert np.array_equal(assign, original)
        assert abs(total - float(g["split_prob"])) <= bound((2 * n + 6) * model.M * 2 + len(S), mag)
        n1, n0 = bs.sm_row_counts(model, i, j, S, original)
        n_j = int(original.sum()) + 1
        lp, lmag = bs.sm_lprior_ratio(model, kind, n, n_j, st.alpha, rows[2], st.theta[[cl_i, cl_j]])
        assert abs(bs.sm_size_ratio_merge(float(g["size_data"]), model.N, len(S)) - float(g["size_ratio"])) <= 8 * 2.0 ** -52 * 10
    assert abs(lp - float(g["lprior"])) <= bound(4 + 3 * model.M, lmag)
    ratio, rmag = bs.sm_ll_ratio(model, kind, n1, n0, rows)
    assert abs(ratio - float(g["ll_ratio"])) <= bound(2 * int((model.pop1 + model.pop0)[np.append(S, [i, j])].sum()), rmag)


def test_the_small_ends_fall_back_as_the_reference_does(gold):
    """log(|S| - 1) raises for |S| of 0 and 1 and the term is -log N - size_data"""
    for case in ("n2k2", "s1"):
        g, model, st, i, j, S = load_move(gold, case, "merge")
        assert len(S) == (0 if case == "n2k2" else 1)
        assert float(g["size_ratio"]) == -np.log(model.N) - float(g["size_data"])
    g, model, st, i, j, S = load_move(gold, "n2k1", "split")
    assert len(S) == 0 and not g["refused"]
    assert load_move(gold, "one_sided", "split")[0]["refused"]


@pytest.mark.parametrize("case", LAYOUT)
@pytest.mark.parametrize("move", ["split0", "merge27"])
def test_an_accepted_move_is_applied_as_the_reference_applies_it(gold, case, move):
    g, model, st, _, _, _ = load_move(gold, case, move)
    kind = "split" if int(g["kind"]) == 0 else "merge"
    cells = g["done_cells"]
    cl_i, cl_j = (int(x) for x in g["done_cl"])
    if kind == "split":
        cl_j = int(np.nonzero(st.sizes == 0)[0][0])                  # get_empty_cluster
    bs.sm_apply(st, kind, cl_i, cl_j, int(cells[-1]), cells[1:-1], g["done_assign"], g["done_rows"])
    assert np.array_equal(st.labels, g["done_labels"])
    assert np.array_equal(st.live(), g["done_ids"]) and np.array_equal(st.sizes[st.live()], g["done_sizes"])
    assert np.array_equal(st.theta[st.live()], g["done_theta"][st.live()])


# ---- the twin's run ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    with np.load(os.path.join(GOLD, "bnpcs.fixture.npz")) as z:
        return z["data"], z["truth"]


KEYS = ("assignments", "params", "DP_alpha", "ML", "MAP", "FN", "FP", "sm_moves")


def test_without_the_move_the_run_is_unchanged(planted):
    data, _ = planted
    a = bs.run_chains_host(data, [5, 6], 12, 4, 0.1, 0.01, pp=(0.25, 0.25))
    b = bs.run_chains_host(data, [5, 6], 12, 4, 0.1, 0.01, pp=(0.25, 0.25), sm_prob=0)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for k in KEYS:
            assert ra[k].tobytes() == rb[k].tobytes()
        assert not ra["sm_moves"].any() and ra["sm_moves"].dtype == np.int8


@pytest.fixture(scope="module")
def sm_run(planted):
    data, _ = planted
    return bs.run_chains_host(data, [1, 2], 300, 100, 0.1, 0.01, sm_prob=0.33)


def test_the_run_with_the_move_recovers_the_planted_partition(planted, sm_run):
    data, truth = planted
    for r in sm_run:
        assert r["variate_errors"] == 0 and r["sm_moves"].shape == (301,) and r["sm_moves"][0] == 0
    cat = bnpc.concat_chains(sm_run)
    assert "sm_moves" not in cat or len(cat["assignments"]) == 402      # concat_chains takes the keys it knows
    est = bnpc.posterior_estimate_host(cat["assignments"], cat["params"], data, cat["DP_alpha"], cat["FN"], cat["FP"])
    assert same_partition(est["assignment"], truth)


def test_save_chains_ignores_the_new_key(tmp_path, sm_run):
    path = str(tmp_path / "chains.npz")
    bnpc.save_chains(path, sm_run)
    back = bnpc.load_chains(path)
    assert len(back) == 2 and np.array_equal(back[0]["assignments"], sm_run[0]["assignments"])


def test_all_four_outcomes_occur(planted, sm_run):
    """the fixture's chains from the random start split and merge but accept no merge (the reference accepts one in a few hundred too): a
    short run from the all-singletons start, where a split of a fresh pair is merged back, supplies it; the `together` start is next in line"""
    data, _ = planted
    model = bs.Model(data, 0.1, 0.01)
    seen = np.zeros(5, int)
    for r in sm_run:
        seen += np.bincount(r["sm_moves"], minlength=5)
    for labels in (np.arange(model.N), np.zeros(model.N, int)):
        if seen[1:].all():
            break
        theta = np.zeros((model.N, model.M), np.float32)
        live = np.unique(labels)
        theta[live] = np.clip(np.random.default_rng(3).random((len(live), model.M)), bs.TMIN, bs.TMAX).astype(np.float32)
        start = [bs.State(labels, theta, model.alpha0) for _ in range(2)]
        for r in bs.run_chains_host(data, [2, 3], 40, 20, 0.1, 0.01, states=start, sm_prob=0.9):
            seen += np.bincount(r["sm_moves"], minlength=5)
    print("sweeps, splits declined / accepted, merges declined / accepted:", seen)
    assert seen[1:].all()


def test_ml_is_the_likelihood_of_the_recorded_state(planted, sm_run):
    data, _ = planted
    model = bs.Model(data, 0.1, 0.01)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    for r in sm_run:
        for s in range(100, 301):
            block = r["params"][s - 100]
            k = len(np.unique(r["assignments"][s]))
            assert not block[k:].any() and (block[:k] > 0).all()
            ll, mag = bs.likelihood(model, r["assignments"][s], block)
            assert abs(r["ML"][s] - ll) <= bound(n_obs, mag), s


def test_refusals_of_the_new_arguments(planted):
    data, _ = planted
    for kw in (dict(sm_prob=1.5), dict(sm_prob=0.3, sm_ratios=(0.5, 0.6)), dict(sm_prob=0.3, sm_ratios=(1.0, 0.0)), dict(sm_prob=0.3, sm_steps=-1)):
        with pytest.raises(ValueError, match="sm_prob"):
            bs.run_chains_host(data, [1], 5, 2, 0.1, 0.01, **kw)


# ---- the script --------------------------------------------------------------------------------------------------------------------------
def test_script_device_sm_refusals(tmp_path):
    """--sampler device-sm refuses what --sampler device refuses, but not the split-merge move; all of it before a device is opened"""
    from tests.test_bnpc_cpu import run_script
    inp = os.path.join(GOLD, "bnpcs.fixture.BinaryMatrix.tsv")
    base = [inp, "--sampler", "device-sm", "--no_plots", "-o", str(tmp_path / "o"), "--bnpc_libs", str(tmp_path / "nowhere")]
    for extra, words in ((["-eup", "0.25"], ("--error_update_prob", "-eup 0")), (["-eup", "0", "-fa", "x.txt"], ("--fixed_assignment",)),
                         (["-eup", "0", "-r", "5"], ("--runtime",)), (["-eup", "0", "-ls", "1.05"], ("--lugsail",)), (["-eup", "0", "-sc"], ("--single_chains",)),
                         (["-smp", "0.33", "-eup", "0", "-ls", "1.05"], ("--lugsail",))):
        r = run_script(base + extra)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (extra, r.stderr)
        assert "--split_merge_prob" not in r.stderr and ("device-sm" in r.stderr or "--single_chains" in r.stderr)
    assert not (tmp_path / "o").exists()


def test_rule_file_names_both_samplers():
    rule = os.path.join(os.path.dirname(GOLD), "..", "workflow", "rules", "CellClustering.gpu.smk")
    text = open(rule).read()
    assert "--sampler device-sm" in text and "--sampler device -smp 0" in text
