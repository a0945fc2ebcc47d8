"""BnpC's split-merge move on the device (k_bnpcs_sm in csrc/bnpc_sampler.hip) against its numpy twin (longsom_amd.bnpc_sampler), which
tests/test_bnpc_sm_cpu.py holds to the reference.  Device and twin share the random stream, so from a loaded state one move gives the same
decisions wherever the twin's own decisions are clear of their edges: the walk's uniforms and the parameter acceptances by 1e-9, the move's
final |ln v - A| by 100 times the bound of A's sum (a fixed 1e-9 is too tight for a sum this long).  That is asserted on the twin for the
seeds listed here: a condition on the seeds, not on the device; a seed that violates it fails the test, it does not skip it."""
import os

import numpy as np
import pandas as pd
import pytest

from longsom_amd import bnpc, bnpc_sampler as bs
from tests.test_bnpc_cpu import run_script
from tests.test_bnpc_sampler_cpu import GOLD, bound, same_partition
from tests.test_bnpc_sampler_gpu import FIXTURE_TSV, KEYS, load, random_data, state_of, ulps32

pytestmark = pytest.mark.gpu

MOVE_SEEDS = (1, 2, 3, 4)
MOVE_CASES = ("n2k1", "n2k2", "singletons3", "together20", "gaps65", "big300")
MISSING_CELLS = (10, 30, 50)                                       # gaps65: the cells of cluster 40, all of them all-missing
ULP = 2.0 ** -52


def move_case(name, M, pp):
    """the model and the labels of a case: the smallest shapes at which the kernel can still go wrong"""
    rng = np.random.default_rng(sum(map(ord, name)) * 1000 + M)
    if name == "n2k1":
        labels = np.array([1, 1])                                     # K = 1 forces a split; S is empty
    elif name == "n2k2":
        labels = np.array([0, 1])                                     # K = N forces a merge; S is empty
    elif name == "singletons3":
        labels = np.arange(3)                                         # a forced merge with |S| = 0
    elif name == "together20":
        labels = np.full(20, 5)                                       # a forced split
    elif name == "gaps65":
        labels = np.where(rng.random(65) < 0.5, 3, 17)                # more than one wave of cells, ids with gaps
        labels[list(MISSING_CELLS)] = 40                              # whichever anchor this cluster gives is all-missing
    else:
        labels = np.where(rng.random(300) < 0.4, 0, 7)                # more cells than the workgroup has lanes
    data = random_data(rng, len(labels), M)
    if M > 1:
        data[:, M // 2] = np.nan                                      # an all-missing column
    if name == "gaps65":
        data[list(MISSING_CELLS)] = np.nan
    return bs.Model(data, 0.1, 0.01, pp), labels


_TWIN = {}


def twin_moves(name, pp):
    """the twin's move of every (M, scans, seed) of a case, made once: [(M, scans, model, start states, [(outcome, state after, margin)])]"""
    if (name, pp) not in _TWIN:
        out = []
        for M in (1, 64, 65, 130):
            model, labels = move_case(name, M, pp)
            for scans in (0, 3):
                start = [state_of(np.random.default_rng(s), model, labels) for s in MOVE_SEEDS]
                moved = []
                for seed, st0 in zip(MOVE_SEEDS, start):
                    st = bs.State(st0.labels, st0.theta, st0.alpha)
                    margin = bs.Margin()
                    want = bs.split_merge_move(model, st, seed, 1, (0.75, 0.25), scans, margin)
                    bs.alpha_update(model, st, seed, 1, margin)
                    moved.append((want, st, margin))
                out.append((M, scans, model, start, moved))
        _TWIN[(name, pp)] = out
    return _TWIN[(name, pp)]


@pytest.mark.parametrize("pp", [(1, 1), (0.25, 0.25)])
@pytest.mark.parametrize("name", MOVE_CASES)
def test_one_move_equals_twin(engine, name, pp):
    for M, scans, model, start, moved in twin_moves(name, pp):
        load(engine, model, MOVE_SEEDS, start)
        engine.bnpcs_set_split_merge(0.33, 0.75, 0.25, scans)
        engine.bnpcs_test_move(2, 1)
        for c, (seed, (want, st, margin)) in enumerate(zip(MOVE_SEEDS, moved)):
            where = "%s M %d pp %r scans %d seed %d" % (name, M, pp, scans, seed)
            assert want["errors"] == 0
            assert margin.value >= 1e-9, "%s: a decision of the twin lies within %g of its edge" % (where, margin.value)
            tol = bs.sm_bound_of_A(want)
            assert abs(want["lv"] - want["A"]) >= 100 * tol, "%s: the twin's ln v - A = %g is within 100 x %g" % (where, want["lv"] - want["A"], tol)
            got = engine.bnpcs_test_move_outcome(c)
            print(where, "code", want["code"], "A", want["A"], got["A"], "bound", tol)
            assert got["code"] == want["code"] and got["clusters"] == want["clusters"] and got["anchors"] == want["anchors"], where
            assert abs(got["lv"] - want["lv"]) <= 4 * ULP * abs(want["lv"])           # the same uniform, a log apart
            assert (np.abs(got["terms"] - want["terms"]) <= (want["counts"] + 4) * ULP * want["mags"]).all(), (where, got["terms"], want["terms"])
            assert abs(got["A"] - want["A"]) <= tol, where
            labels_d, theta, alpha = engine.bnpcs_get_state(c)
            assert np.array_equal(labels_d, st.labels), where
            live = st.live()
            assert ulps32(theta[live], st.theta[live]).max() <= 1, where
            assert abs(alpha - st.alpha) <= 1e-12 * st.alpha, where
        n1, _ = engine.bnpcs_test_counts(0)                       # the counts the host makes after a move are those of the moved labels
        assert np.array_equal(n1, bs.counts(model, moved[0][1])[0])
        engine.bnpcs_destroy()


def test_the_cases_hold_both_outcomes_of_both_moves():
    """over the cases above, on the twin (which the device equalled there): every code occurs, and a move whose anchor is all-missing"""
    codes, missing_anchor = np.zeros(5, int), 0
    for name in MOVE_CASES:
        for pp in ((1, 1), (0.25, 0.25)):
            for _, _, _, _, moved in twin_moves(name, pp):
                for want, _, _ in moved:
                    codes[want["code"]] += 1
                    missing_anchor += name == "gaps65" and bool(set(want["anchors"]) & set(MISSING_CELLS))
    print("splits declined / accepted, merges declined / accepted:", codes[1:], "moves with an all-missing anchor:", missing_anchor)
    assert codes[1:].all() and missing_anchor > 0


def test_refusals(engine):
    model, labels = move_case("n2k1", 1, (1, 1))
    load(engine, model, [1], [state_of(np.random.default_rng(1), model, labels)])
    for args in ((-0.1, 0.75, 0.25, 3), (1.5, 0.75, 0.25, 3), (0.3, 0.75, 0.5, 3), (0.3, 1.0, 0.0, 3), (0.3, 0.75, 0.25, -1)):
        with pytest.raises(Exception, match="lsg_bnpcs_set_split_merge"):
            engine.bnpcs_set_split_merge(*args)
    engine.bnpcs_destroy()


# ---- runs ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    with np.load(os.path.join(GOLD, "bnpcs.fixture.npz")) as z:
        return z["data"], z["truth"]


SM_KEYS = KEYS + ("sm_moves",)
SHORT_SEED = 7


def test_short_run_equals_twin(engine, planted):
    """30 steps with the move in a third of them, under the non-uniform prior: every step's labels and moves as the twin's"""
    data, _ = planted
    kw = dict(pp=(0.25, 0.25), dpa=(2.0, 0.5), dpa_prob=0.25, sm_prob=0.33)
    host = bs.run_chains_host(data, [SHORT_SEED], 30, 10, 0.1, 0.01, **kw)[0]
    seen = np.bincount(host["sm_moves"], minlength=5)
    assert seen[1] + seen[2] > 0 and seen[3] + seen[4] > 0, "the seed's 30 steps hold no move of each kind: %r" % (seen,)
    dev = bs.run_chains(engine, data, [SHORT_SEED], 30, 10, 0.1, 0.01, **kw)[0]
    assert np.array_equal(host["sm_moves"], dev["sm_moves"]) and dev["sm_moves"].dtype == np.int8
    assert np.array_equal(host["assignments"], dev["assignments"])
    assert ulps32(host["params"], dev["params"]).max() <= 1
    assert np.array_equal(host["DP_alpha"][0], dev["DP_alpha"][0]) and np.allclose(host["DP_alpha"], dev["DP_alpha"], rtol=1e-12, atol=0)
    model = bs.Model(data, 0.1, 0.01, (0.25, 0.25), (2.0, 0.5), 0.25)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    assert (np.abs(host["ML"] - dev["ML"]) <= bound(n_obs, np.abs(host["ML"]))).all()
    for s in range(10, 31):
        k = len(np.unique(host["assignments"][s]))
        terms = np.abs(bs.beta_logpdf(host["params"][s - 10][:k], 0.25, 0.25)).sum() + 10.0 * k + abs(float(bs.alpha_logpdf(model, host["DP_alpha"][s])))
        assert np.isfinite(host["MAP"][s]) and abs(host["MAP"][s] - dev["MAP"][s]) <= bound(n_obs + k * model.M + 2 * k + 1, abs(host["ML"][s]) + terms)


def test_without_the_move_the_run_is_the_parent_s(engine, planted):
    data, _ = planted
    a = bs.run_chains(engine, data, [1, 2], 40, 10, 0.1, 0.01)
    b = bs.run_chains(engine, data, [1, 2], 40, 10, 0.1, 0.01, sm_prob=0)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for k in SM_KEYS:
            assert ra[k].tobytes() == rb[k].tobytes()
        assert not ra["sm_moves"].any()


@pytest.fixture(scope="module")
def run(engine, planted):
    data, _ = planted
    return bs.run_chains(engine, data, [1, 2], 300, 100, 0.1, 0.01, sm_prob=0.33)


def test_run_recovers_the_planted_partition(engine, planted, run):
    data, truth = planted
    cat = bnpc.concat_chains(run)
    est = bnpc.posterior_estimate(engine, cat["assignments"], cat["params"], data, cat["DP_alpha"], cat["FN"], cat["FP"])
    assert same_partition(est["assignment"], truth)
    seen = sum(np.bincount(r["sm_moves"], minlength=5) for r in run)
    print("sweeps, splits declined / accepted, merges declined / accepted:", seen)
    assert 150 < seen[1:].sum() < 250                                 # a third of 600 steps


def test_run_records_are_tied_to_the_state(planted, run):
    data, _ = planted
    model = bs.Model(data, 0.1, 0.01)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    for r in run:
        assert r["variate_errors"] == 0 and r["burn_in"] == 100
        assert r["assignments"].shape == (301, 60) and r["assignments"].min() >= 0 and r["assignments"].max() < 60
        assert r["params"].shape[0] == 201 and r["params"].dtype == np.float32 and r["sm_moves"].shape == (301,)
        assert np.isfinite(r["ML"]).all() and np.isfinite(r["MAP"]).all() and (r["DP_alpha"] > 1).all()
        for s in range(1, 301):
            # a declined move leaves the labels, an accepted one changes the number of clusters by one
            k0, k1 = len(np.unique(r["assignments"][s - 1])), len(np.unique(r["assignments"][s]))
            code = r["sm_moves"][s]
            if code in (1, 3):
                assert np.array_equal(r["assignments"][s], r["assignments"][s - 1]), s
            elif code:
                assert k1 - k0 == (1 if code == 2 else -1), s
        for s in range(100, 301):
            block = r["params"][s - 100]
            k = len(np.unique(r["assignments"][s]))
            assert not block[k:].any() and (block[:k] > 0).all()
            ll, mag = bs.likelihood(model, r["assignments"][s], block)
            assert abs(r["ML"][s] - ll) <= bound(n_obs, mag), s


def test_run_is_deterministic_and_chains_are_independent(engine, planted, run):
    data, _ = planted
    again = bs.run_chains(engine, data, [1, 2], 300, 100, 0.1, 0.01, sm_prob=0.33)
    for a, b in zip(run, again):
        for k in SM_KEYS:
            assert a[k].tobytes() == b[k].tobytes()
    three = bs.run_chains(engine, data, [9, 2, 1], 300, 100, 0.1, 0.01, sm_prob=0.33)
    for k in SM_KEYS:
        assert np.array_equal(three[1][k], run[1][k]) and np.array_equal(three[2][k], run[0][k])


def test_run_with_an_arena_that_overflows(engine, planted, run):
    data, _ = planted
    small = bs.run_chains(engine, data, [1, 2], 300, 100, 0.1, 0.01, arena_rows=60, sm_prob=0.33)
    for a, b in zip(run, small):
        for k in SM_KEYS:
            assert np.array_equal(a[k], b[k])


# ---- the script ---------------------------------------------------------------------------------------------------------------------------
def test_script_device_sm_sampler(tmp_path, planted):
    """LongSom's BnpC_clustering flags (CellClustering.smk:162-176, config.yaml:111-119), no -smp: the reference's defaults apply"""
    _, truth = planted
    out = str(tmp_path / "out")
    r = run_script([FIXTURE_TSV, "--sampler", "device-sm", "-cup", "0", "-eup", "0", "-FP", "-1", "-FN", "-1", "-pp", "1", "1", "-ap", "0.001", "5.0", "-n", "2", "-s", "300",
                    "--seed", "1", "--no_plots", "-o", out, "-v", "0", "--bnpc_libs", str(tmp_path / "nowhere")])
    assert r.returncode == 0, r.stderr
    row = pd.read_csv(os.path.join(out, "assignment.txt"), sep="\t").iloc[0]
    assert same_partition([int(x) for x in row["Assignment"].split()], truth)
    assert os.path.exists(os.path.join(out, "errors.txt")) and os.path.exists(os.path.join(out, "genotypes_posterior_mean.tsv"))
