"""The error-rate update and the fixed assignment of BnpC's sampler on the device (csrc/bnpc_sampler.hip: k_bnpcs_err, the per-chain rates)
against the numpy twin (longsom_amd.bnpc_sampler), which tests/test_bnpc_errors_cpu.py holds to the reference.  Device and twin share the
random stream, so one update from a loaded state must take the same sd and make the same decision wherever the twin's own decision is not
at its edge: |ln v - A| >= 100 x the bound of A and the deciding draw at least 1e-9 from error_prob, asserted on the TWIN for the seeds
used here: a condition on the seeds, not on the device.  The proposal may differ by 4 ulp (ndtr, ndtri); the likelihoods and A are then
compared with the twin's AT THE DEVICE'S proposal, sums with |a - b| <= (n + 4) 2^-52 sum |term|."""
import os

import numpy as np
import pandas as pd
import pytest

from longsom_amd import bnpc_sampler as bs
from tests.test_bnpc_cpu import run_script
from tests.test_bnpc_sampler_cpu import GOLD, bound, same_partition
from tests.test_bnpc_sampler_gpu import FIXTURE_TSV, load, random_data, state_of, ulps32

pytestmark = pytest.mark.gpu

WIDE = (0.01, 0.01, 0.2, 0.1)
TIGHT = (0.001, 0.0005, 0.25, 0.05)
UPDATE_SEEDS = (1, 2, 3, 4)
UPDATE_PROB = 0.75                                                    # the hook honours the deciding draw: some chains only decline to update
UPDATE_CASES = [(name, pp, priors) for name in ("tiny", "one_word", "holes", "two_words", "singletons") for pp in ((1, 1), (0.25, 0.25)) for priors in (WIDE, TIGHT)]


def update_case(name, pp, priors):
    """(model, start(seed)): the smallest shapes at which the kernel can go wrong.  The rates start off the priors' means, by a factor per
    seed, so that moves towards them are accepted and moves away declined"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "tiny":
        data, labels = np.array([[1.0], [0.0]]), np.array([1, 1])
    elif name == "one_word":
        data, labels = random_data(rng, 3, 64), np.array([0, 2, 2])
    elif name == "holes":
        data = random_data(rng, 20, 65)
        data[7] = np.nan                                              # an all-missing cell
        data[:, 64] = np.nan                                          # an all-missing column, the only one of the second word
        labels = np.array([3, 9, 17])[np.arange(20) % 3]
    elif name == "two_words":
        data = random_data(rng, 65, 130)
        labels = np.sort(rng.permutation(65)[:5])[np.arange(65) % 5]  # ids with gaps
    else:
        data, labels = random_data(rng, 300, 130), np.arange(300)     # more live clusters than the workgroup has lanes
    model = bs.Model(data, priors[2], priors[0], pp, error_prob=UPDATE_PROB, error_priors=priors)

    def start(seed):
        st = state_of(np.random.default_rng(seed), model, labels)
        f = (0.5, 0.9, 1.2, 2.0)[seed % 4]
        st.FP, st.FN = priors[0] * f, priors[2] * (2.5 - f) / 1.5
        return st
    return model, start


def twin_update(model, st, seed, step=3):
    """the twin's update of a copy of the state: (outcome, margin)"""
    st = bs.State(st.labels, st.theta, st.alpha, st.FP, st.FN)
    margin = bs.Margin()
    return bs.error_update(model.of_chain(st.FP, st.FN), st, seed, step, margin), margin


def test_update_seeds_reach_both_decisions_of_both_rates():
    """on the twin: over the cases of test_one_update_equals_twin FP and FN are each accepted and each declined, and some chain's draw
    says no update"""
    seen = set()
    for name, pp, priors in UPDATE_CASES:
        model, start = update_case(name, pp, priors)
        for seed in UPDATE_SEEDS:
            out, _ = twin_update(model, start(seed), seed)
            seen |= {(None, None)} if out is None else {(rate, out[rate]["code"]) for rate in ("FP", "FN")}
    assert seen >= {("FP", 1), ("FP", 0), ("FN", 1), ("FN", 0), (None, None)}, seen


@pytest.mark.parametrize("name,pp,priors", UPDATE_CASES)
def test_one_update_equals_twin(engine, name, pp, priors):
    model, start = update_case(name, pp, priors)
    states = [start(s) for s in UPDATE_SEEDS]
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    load(engine, model, UPDATE_SEEDS, states)
    engine.bnpcs_set_error_learning(UPDATE_PROB, *priors)
    for c, st in enumerate(states):
        engine.bnpcs_set_error_rates(c, st.FP, st.FN)
    engine.bnpcs_test_move(3, 3)
    for c, (seed, st) in enumerate(zip(UPDATE_SEEDS, states)):
        twin, margin = twin_update(model, st, seed)
        assert margin.value >= 1e-9, "seed %d: the twin's deciding draw lies within %g of error_prob" % (seed, margin.value)
        dev = engine.bnpcs_test_error_outcome(c)
        assert (dev is None) == (twin is None)
        if twin is None:
            continue
        cur = bs.State(st.labels, st.theta, st.alpha, st.FP, st.FN)
        for e, rate in enumerate(("FP", "FN")):
            d, t = dev[rate], twin[rate]
            assert abs(t["lv"] - t["A"]) >= 100 * bs.error_bound_of_A(model, t), "seed %d: the twin's %s decision lies at its edge" % (seed, rate)
            assert d["pick"] == t["pick"] and d["code"] == t["code"] and t["code"] >= 0
            assert abs(d["new"] - t["new"]) <= 4 * np.spacing(t["new"]) and abs(d["lv"] - t["lv"]) <= 4 * np.spacing(abs(t["lv"]))
            psd = priors[2 * e + 1]
            ref = bs.error_log_A(model, cur, rate, d["new"], (psd * 0.5, psd, psd * 1.5)[d["pick"]])      # the twin at the device's proposal
            print(name, seed, rate, "A", d["A"], ref["A"], "bound", bs.error_bound_of_A(model, ref), "ll", d["new_ll"] - ref["new_ll"], d["old_ll"] - ref["old_ll"])
            assert abs(d["new_ll"] - ref["new_ll"]) <= bound(n_obs, ref["ll_mag"][0]) and abs(d["old_ll"] - ref["old_ll"]) <= bound(n_obs, ref["ll_mag"][1])
            for k in ("prior", "new_p", "old_p"):
                assert abs(d[k] - ref[k]) <= 64 * 2.0 ** -52 * (abs(ref["new_prior"]) + abs(ref["old_prior"]) + abs(ref["new_p"]) + abs(ref["old_p"]) + 40.0)
            assert abs(d["A"] - ref["A"]) <= bs.error_bound_of_A(model, ref)
            if d["code"] == 1:
                cur.FP, cur.FN = (d["new"], cur.FN) if e == 0 else (cur.FP, d["new"])
    engine.bnpcs_destroy()


# ---- runs -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    with np.load(os.path.join(GOLD, "bnpcs.fixture.npz")) as z:
        return z["data"], z["truth"]


KEYS = ("assignments", "params", "DP_alpha", "ML", "MAP", "FN", "FP", "sm_moves", "error_moves")
RUN = dict(pp=(0.25, 0.25), sm_prob=0.33, error_prob=0.5, error_priors=WIDE)


@pytest.fixture(scope="module")
def host(planted):
    return bs.run_chains_host(planted[0], [1, 2], 30, 10, 0.2, 0.01, **RUN)


@pytest.fixture(scope="module")
def run(engine, planted):
    return bs.run_chains(engine, planted[0], [1, 2], 30, 10, 0.2, 0.01, **RUN)


def test_short_run_equals_twin(planted, host, run):
    data, _ = planted
    model = bs.Model(data, 0.2, 0.01, (0.25, 0.25), error_prob=0.5, error_priors=WIDE)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    assert any(h["error_moves"][0] > 0 for h in host) and any(h["error_moves"][2] > 0 for h in host), "the twin's run accepts no move of a rate"
    for h, d in zip(host, run):
        assert np.array_equal(h["assignments"], d["assignments"]) and np.array_equal(h["sm_moves"], d["sm_moves"]) and np.array_equal(h["error_moves"], d["error_moves"])
        assert np.allclose(h["FP"], d["FP"], rtol=1e-12, atol=0) and np.allclose(h["FN"], d["FN"], rtol=1e-12, atol=0)
        assert h["variate_errors"] == d["variate_errors"] == 0
        assert ulps32(h["params"], d["params"]).max() <= 1
        assert (np.abs(h["ML"] - d["ML"]) <= bound(n_obs, np.abs(h["ML"]))).all()
        for s in range(10, 31):
            k = len(np.unique(h["assignments"][s]))
            terms = (np.abs(bs.beta_logpdf(h["params"][s - 10][:k], 0.25, 0.25)).sum() + 10.0 * k + abs(float(bs.alpha_logpdf(model, h["DP_alpha"][s])))
                     + abs(float(bs.error_prior_logpdf(model, h["FP"][s], h["FN"][s]))) + 40.0)
            assert np.isfinite(h["MAP"][s]) and abs(h["MAP"][s] - d["MAP"][s]) <= bound(n_obs + k * model.M + 2 * k + 3, abs(h["ML"][s]) + terms)


@pytest.mark.parametrize("sm_prob", [0.0, 0.33])
def test_off_is_the_run_without_it(engine, planted, sm_prob):
    data, _ = planted
    kw = dict(pp=(0.25, 0.25), sm_prob=sm_prob)
    plain = bs.run_chains(engine, data, [4, 5], 30, 10, 0.2, 0.01, **kw)
    off = bs.run_chains(engine, data, [4, 5], 30, 10, 0.2, 0.01, error_prob=0.0, error_priors=WIDE, **kw)
    twin = bs.run_chains_host(data, [4, 5], 30, 10, 0.2, 0.01, **kw)
    for a, b, h in zip(plain, off, twin):
        assert set(a) == set(b)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        assert np.array_equal(a["assignments"], h["assignments"]) and not a["error_moves"].any() and (a["FP"] == 0.01).all() and (a["FN"] == 0.2).all()


def test_records_are_tied_to_the_state(planted, run):
    data, _ = planted
    model = bs.Model(data, 0.2, 0.01, (0.25, 0.25))
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    for seed, r in zip((1, 2), run):
        assert r["FP"][0] == 0.01 and r["FN"][0] == 0.2
        assert ((r["FP"] > 0) & (r["FP"] < 1) & (r["FN"] > 0) & (r["FN"] < 1)).all()
        for s in range(10, 31):
            k = len(np.unique(r["assignments"][s]))
            ll, mag = bs.likelihood(model.of_chain(r["FP"][s], r["FN"][s]), r["assignments"][s], r["params"][s - 10][:k])
            assert abs(r["ML"][s] - ll) <= bound(n_obs, mag), s
        made = np.array([s > 0 and float(bs.doubles(seed, 0, s, bs.P_ERR)[0]) < 0.5 for s in range(31)])
        assert r["error_moves"][:2].sum() == r["error_moves"][2:].sum() == made.sum()
        for e, k in enumerate(("FP", "FN")):
            changed = np.nonzero(np.diff(r[k]))[0] + 1
            assert made[changed].all() and len(changed) == r["error_moves"][2 * e]


def test_run_is_deterministic_chains_are_independent_and_the_arena_may_overflow(engine, planted, run):
    data, _ = planted
    again = bs.run_chains(engine, data, [1, 2], 30, 10, 0.2, 0.01, **RUN)
    small = bs.run_chains(engine, data, [1, 2], 30, 10, 0.2, 0.01, arena_rows=60, **RUN)
    three = bs.run_chains(engine, data, [9, 2, 1], 30, 10, 0.2, 0.01, **RUN)
    for k in KEYS:
        for a, b, c in zip(run, again, small):
            assert a[k].tobytes() == b[k].tobytes() and np.array_equal(a[k], c[k]), k
        assert np.array_equal(three[1][k], run[1][k]) and np.array_equal(three[2][k], run[0][k]), k


def test_fixed_assignment_on_the_device(engine, planted):
    data, truth = planted
    kw = dict(pp=(0.25, 0.25), sm_prob=0.33, error_prob=0.5, error_priors=WIDE, fixed_assignment=truth * 3 + 2)
    twin = bs.run_chains_host(data, [5, 6], 30, 10, 0.2, 0.01, **kw)
    dev = bs.run_chains(engine, data, [5, 6], 30, 10, 0.2, 0.01, **kw)
    model = bs.Model(data, 0.2, 0.01, (0.25, 0.25))
    for h, d in zip(twin, dev):
        assert (d["assignments"] == truth[None, :]).all() and np.array_equal(d["assignments"], h["assignments"])
        assert not d["sm_moves"].any() and (d["DP_alpha"] == model.alpha0).all()
        assert ulps32(h["params"], d["params"]).max() <= 1
        assert np.array_equal(h["error_moves"], d["error_moves"]) and d["error_moves"].sum() > 0
        assert np.allclose(h["FP"], d["FP"], rtol=1e-12, atol=0) and np.allclose(h["FN"], d["FN"], rtol=1e-12, atol=0)


def test_refusals(engine):
    model = bs.Model(np.array([[1.0, 0.0], [0.0, np.nan]]), 0.2, 0.01)
    load(engine, model, [1], [bs.initial_state(model, 1)])
    for args in ((-0.1,) + WIDE, (1.1,) + WIDE, (0.5, 0.0, 0.01, 0.2, 0.1), (0.5, 0.01, 1.0, 0.2, 0.1), (0.5, 0.01, 0.01, 1.5, 0.1), (0.5, 0.01, 0.01, 0.2, -1.0),
                 (0.5, 0.01, 0.01, float("nan"), 0.1)):
        with pytest.raises(Exception, match="lsg_bnpcs_set_error_learning"):
            engine.bnpcs_set_error_learning(*args)
    for args in ((0, 0.0, 0.2), (0, 0.01, 1.0), (0, -0.5, 0.2), (0, 0.01, float("nan")), (1, 0.01, 0.2)):
        with pytest.raises(Exception, match="lsg_bnpcs_set_error_rates"):
            engine.bnpcs_set_error_rates(*args)
    with pytest.raises(Exception, match="lsg_bnpcs_test_move"):
        engine.bnpcs_test_move(3, 1)                                  # no error update before lsg_bnpcs_set_error_learning
    engine.bnpcs_set_error_learning(0.0, *WIDE)
    engine.bnpcs_set_error_learning(1.0, *WIDE)
    engine.bnpcs_set_error_rates(0, 0.02, 0.3)
    engine.bnpcs_destroy()


# ---- the script -------------------------------------------------------------------------------------------------------------------------
def test_script_device_errors(tmp_path, planted):
    """BnpC's own defaults: -eup 0.25 and no -FP / -FN, the split-merge move in a third of the steps"""
    _, truth = planted
    out = str(tmp_path / "out")
    r = run_script([FIXTURE_TSV, "--sampler", "device-errors", "-n", "2", "-s", "300", "--seed", "1", "--no_plots", "-pp", "1", "1", "-ap", "0.001", "5.0",
                    "-o", out, "-v", "0", "--bnpc_libs", str(tmp_path / "nowhere")])
    assert r.returncode == 0, r.stderr
    row = pd.read_csv(os.path.join(out, "assignment.txt"), sep="\t").iloc[0]
    assert same_partition([int(x) for x in row["Assignment"].split()], truth)
    first = pd.read_csv(os.path.join(out, "errors.txt"), sep="\t").iloc[0]
    print(first)
    for k in ("FN_model", "FP_model"):                                # mean+-sd over the kept samples: the rates moved, so the sd is not 0
        mean, sd = (float(x) for x in first[k].split("+-"))
        assert 0 < mean < 1 and sd > 0, (k, first[k])
    assert 0 <= float(first["FN_data"]) <= 1 and 0 <= float(first["FP_data"]) <= 1
