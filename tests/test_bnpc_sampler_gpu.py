"""BnpC's sampler on the device (csrc/bnpc_sampler.hip, lsg_bnpcs_*) against its numpy twin (longsom_amd.bnpc_sampler), which
tests/test_bnpc_sampler_cpu.py holds to the reference.  Device and twin share the random stream, so from a loaded state one sweep and one
parameter move must give the same decisions wherever the twin's own decision is not within 1e-9 of its edge: that is asserted on the twin
for the seeds used here, it is a condition on the seeds and not on the device.  Sums are compared with the CPU tests' bound
|a - b| <= (n + 4) 2^-52 sum |term|."""
import os

import numpy as np
import pandas as pd
import pytest

from longsom_amd import bnpc, bnpc_sampler as bs
from tests.test_bnpc_cpu import run_script
from tests.test_bnpc_sampler_cpu import GOLD, bound, same_partition

pytestmark = pytest.mark.gpu

FIXTURE_TSV = os.path.join(GOLD, "bnpcs.fixture.BinaryMatrix.tsv")


def ulps32(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def random_data(rng, N, M, missing=0.2):
    data = (rng.random((N, M)) < 0.5).astype(float)
    data[rng.random((N, M)) < missing] = np.nan
    return data


def planted_data(rng, N, M, K):
    truth = np.arange(N) % K
    g = (rng.random((K, M)) < 0.5)[truth]
    data = g.astype(float)
    data[g & (rng.random((N, M)) < 0.1)] = 0
    data[~g & (rng.random((N, M)) < 0.01)] = 1
    data[rng.random((N, M)) < 0.2] = np.nan
    return data, truth


def state_of(rng, model, labels):
    theta = np.zeros((model.N, model.M), np.float32)
    live = np.unique(labels)
    theta[live] = np.clip(rng.random((len(live), model.M)), bs.TMIN, bs.TMAX).astype(np.float32)
    return bs.State(labels, theta, model.alpha0)


def load(engine, model, seeds, states, steps=1):
    engine.bnpcs_create(model, seeds, steps, max(model.N, 64))
    for c, st in enumerate(states):
        engine.bnpcs_set_state(c, st.labels, st.theta, st.alpha)


# ---- the stream and the variates --------------------------------------------------------------------------------------------------
def test_stream_equals_twin(engine):
    edge = np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    grid = np.stack(np.meshgrid(edge, edge, edge, edge[:3], indexing="ij"), -1).reshape(-1, 4)
    ctr = np.concatenate([grid, np.random.default_rng(1).integers(0, 2 ** 32, (5000, 4), dtype=np.uint64).astype(np.uint32)])
    for key in (0, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF):
        words, dbl = engine.bnpcs_test_stream(key, ctr)
        want = bs.philox(key, ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3])
        for k in range(4):
            assert np.array_equal(words[:, k], want[k])
        assert np.array_equal(dbl[:, 0], bs.to_double(want[0], want[1])) and np.array_equal(dbl[:, 1], bs.to_double(want[2], want[3]))
        assert dbl.min() > 0 and dbl.max() < 1


def agree(x, want):
    """the share of draws within relative 1e-10 of the twin's: only a rejection test flipped by an ulp may differ"""
    share = np.mean(np.abs(x - want) <= 1e-10 * np.abs(want))
    print("share of draws within 1e-10 of the twin: %.5f" % share)
    return share >= 0.999


@pytest.mark.parametrize("a,b", [(1, 1), (1, 2), (2, 1), (0.25, 1.25), (50.25, 30.25)])
def test_beta_variates(engine, a, b):
    from scipy import stats
    n = 20000
    x, err = engine.bnpcs_test_variates(7, 0, n, a, b)
    want, _ = bs.beta_variate(7, a, b, np.arange(n), 0, bs.P_BIRTH)
    assert err == 0 and agree(x, want)
    p = stats.kstest(x, stats.beta(a, b).cdf).pvalue
    print("KS p", p)
    assert p > 1e-4


@pytest.mark.parametrize("sd", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("old", [bs.TMIN, 0.5, bs.TMAX])
def test_truncated_normal_variates(engine, old, sd):
    from scipy import stats
    n = 20000
    x, _ = engine.bnpcs_test_variates(7, 1, n, old, sd)
    u, _ = bs.doubles(7, np.arange(n), 0, bs.P_MH)
    old32 = np.float32(old)
    want = bs.truncnorm_variate(u, old32, sd).astype(np.float64)
    assert agree(x, want)
    a, b = (bs.TMIN - old32) / sd, (bs.TMAX - old32) / sd
    p = stats.kstest(x, stats.truncnorm(a, b, loc=old32, scale=sd).cdf).pvalue
    print("KS p", p)
    assert p > 1e-4


def test_gamma_variates_below_and_above_one(engine):
    for a in (0.001, 0.5, 1.0, 8.7):
        x, err = engine.bnpcs_test_variates(11, 2, 5000, a, 0)
        want, _ = bs.gamma_variate(11, a, np.arange(5000), 0, bs.P_ALPHA)
        assert err == 0 and np.mean(np.abs(x - want) <= 1e-10 * np.abs(want)) >= 0.999


# ---- counts and the likelihood matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(2, 1), (2, 2), (65, 1), (65, 3), (65, 65)])
def test_counts_and_likelihood_matrix(engine, N, K):
    for M in (1, 63, 64, 65, 130):
        rng = np.random.default_rng(N * 1000 + K * 10 + M)
        data = random_data(rng, N, M)
        data[N - 1] = np.nan                                          # an all-missing cell
        if M > 1:
            data[:, M // 2] = np.nan                                  # an all-missing column
        model = bs.Model(data, 0.1, 0.01)
        ids = np.sort(rng.permutation(N)[:K])                         # cluster ids with gaps
        labels = ids[np.concatenate([np.arange(K), rng.integers(0, K, N - K)])]
        st = state_of(rng, model, labels)
        load(engine, model, [3], [st])
        n1, n0 = engine.bnpcs_test_counts(0)
        w1, w0 = bs.counts(model, st)
        assert np.array_equal(n1, w1) and np.array_equal(n0, w0)
        ll, cols = engine.bnpcs_test_ll(0)
        assert np.array_equal(cols, ids) and ll.shape == (N, K)
        L1, L0 = bs.log_tables(st.theta[ids], model.FN, model.FP)
        want = model.one_f @ L1.T + model.zero_f @ L0.T
        mag = model.one_f @ np.abs(L1).T + model.zero_f @ np.abs(L0).T
        assert (np.abs(ll - want) <= bound((model.pop1 + model.pop0)[:, None], mag)).all()
        assert not ll[N - 1].any()
        engine.bnpcs_destroy()


# ---- one sweep from a loaded state ----------------------------------------------------------------------------------------------------
def sweep_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "singletons":                                          # every removal frees an id that a birth can issue again: the stale-column case
        data = np.array([[1, 0], [0, 1], [1, np.nan]], float)
        model = bs.Model(data, 0.1, 0.01, (0.25, 0.25))
        return model, lambda seed: state_of(np.random.default_rng(seed), model, np.arange(3))
    if name == "random_start":
        model = bs.Model(random_data(rng, 65, 65), 0.1, 0.01)
        return model, lambda seed: bs.initial_state(model, seed)
    if name == "planted":
        data, truth = planted_data(rng, 130, 200, 4)
        model = bs.Model(data, 0.1, 0.01, (0.25, 0.25), (0.001, 5.0))
        return model, lambda seed: state_of(np.random.default_rng(seed), model, truth * 7)
    if name == "together":
        model = bs.Model(random_data(rng, 20, 10), 0.1, 0.01)
        return model, lambda seed: state_of(np.random.default_rng(seed), model, np.full(20, 5))
    data = random_data(rng, 40, 33)
    data[17] = np.nan                                                 # one all-missing cell
    model = bs.Model(data, 0.1, 0.01)
    return model, lambda seed: bs.initial_state(model, seed)


SWEEP_SEEDS = (1, 2, 3, 4)


@pytest.mark.parametrize("name", ["singletons", "random_start", "planted", "together", "missing_cell"])
def test_one_sweep_equals_twin(engine, name):
    model, start = sweep_case(name)
    states = [start(s) for s in SWEEP_SEEDS]
    load(engine, model, SWEEP_SEEDS, states)
    engine.bnpcs_test_move(0, 1)
    births = 0
    for c, (seed, st) in enumerate(zip(SWEEP_SEEDS, states)):
        margin = bs.Margin()
        assert bs.gibbs_sweep(model, st, seed, 1, margin) == 0
        bs.alpha_update(model, st, seed, 1, margin)
        assert margin.value >= 1e-9, "seed %d: a decision of the twin lies within %g of its edge" % (seed, margin.value)
        labels, theta, alpha = engine.bnpcs_get_state(c)
        assert np.array_equal(labels, st.labels)
        assert np.array_equal(np.bincount(labels, minlength=model.N), st.sizes)
        live = st.live()
        assert ulps32(theta[live], st.theta[live]).max() <= 1
        assert abs(alpha - st.alpha) <= 1e-12 * st.alpha
        births += margin.births
    engine.bnpcs_destroy()
    assert births, "no chain of the case opened a cluster: its seeds do not reach the birth path"


# ---- one parameter move from a loaded state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pp", [(1, 1), (0.25, 0.25)])
@pytest.mark.parametrize("K", [1, 3, 65])
def test_one_parameter_move_equals_twin(engine, K, pp):
    N = 70
    for M in (1, 64, 65, 200):
        rng = np.random.default_rng(K * 1000 + M)
        data = random_data(rng, N, M)
        if M > 1:
            data[:, M - 1] = np.nan                                   # a column with n1 = n0 = 0 in every cluster
        model = bs.Model(data, 0.1, 0.01, pp)
        ids = np.sort(rng.permutation(N)[:K])
        labels = ids[np.concatenate([np.arange(K), rng.integers(min(1, K - 1), K, N - K)])]      # K > 1: the first cluster keeps one cell
        seeds = (5, 6)
        states = [state_of(np.random.default_rng(s), model, labels) for s in seeds]
        for st in states:
            st.theta[ids[0], 0] = bs.TMIN32
        load(engine, model, seeds, states)
        engine.bnpcs_test_move(1, 4)
        for c, (seed, st) in enumerate(zip(seeds, states)):
            old = st.theta.copy()
            margin = bs.Margin()
            bs.parameter_move(model, st, seed, 4, margin)
            assert margin.value >= 1e-9, "seed %d: an acceptance of the twin lies within %g of its threshold" % (seed, margin.value)
            labels_d, theta, _ = engine.bnpcs_get_state(c)
            assert np.array_equal(labels_d, labels)
            assert ulps32(theta[ids], st.theta[ids]).max() <= 1
            assert (st.theta[ids] != old[ids]).any()
        engine.bnpcs_destroy()


# ---- a run --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    with np.load(os.path.join(GOLD, "bnpcs.fixture.npz")) as z:
        return z["data"], z["truth"]


KEYS = ("assignments", "params", "DP_alpha", "ML", "MAP", "FN", "FP")


@pytest.fixture(scope="module")
def run(engine, planted):
    data, _ = planted
    return bs.run_chains(engine, data, [1, 2], 300, 100, 0.1, 0.01)


def test_run_recovers_the_planted_partition(engine, planted, run):
    data, truth = planted
    cat = bnpc.concat_chains(run)
    est = bnpc.posterior_estimate(engine, cat["assignments"], cat["params"], data, cat["DP_alpha"], cat["FN"], cat["FP"])
    assert same_partition(est["assignment"], truth)


def test_run_records_are_tied_to_the_state(planted, run):
    data, _ = planted
    model = bs.Model(data, 0.1, 0.01)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    for r in run:
        assert r["variate_errors"] == 0 and r["burn_in"] == 100
        assert r["assignments"].shape == (301, 60) and r["assignments"].min() >= 0 and r["assignments"].max() < 60
        assert r["params"].shape[0] == 201 and r["params"].dtype == np.float32
        assert np.isfinite(r["ML"]).all() and np.isfinite(r["MAP"]).all() and (r["DP_alpha"] > 1).all()
        for s in range(100, 301):
            block = r["params"][s - 100]
            k = len(np.unique(r["assignments"][s]))
            assert not block[k:].any() and (block[:k] > 0).all()
            ll, mag = bs.likelihood(model, r["assignments"][s], block)
            assert abs(r["ML"][s] - ll) <= bound(n_obs, mag), s


def test_run_is_deterministic_and_chains_are_independent(engine, planted, run):
    data, _ = planted
    again = bs.run_chains(engine, data, [1, 2], 300, 100, 0.1, 0.01)
    for a, b in zip(run, again):
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes()
    three = bs.run_chains(engine, data, [9, 2, 1], 300, 100, 0.1, 0.01)
    for k in KEYS:
        assert np.array_equal(three[1][k], run[1][k]) and np.array_equal(three[2][k], run[0][k])


def test_run_with_an_arena_that_overflows(engine, planted, run):
    data, _ = planted
    small = bs.run_chains(engine, data, [1, 2], 300, 100, 0.1, 0.01, arena_rows=60)
    for a, b in zip(run, small):
        for k in KEYS:
            assert np.array_equal(a[k], b[k])


def test_short_run_equals_twin(engine, planted):
    """30 steps from the random start under the non-uniform prior: the labels of every step as the twin's, ML and MAP within the bound"""
    data, _ = planted
    kw = dict(pp=(0.25, 0.25), dpa=(2.0, 0.5), dpa_prob=0.25)
    host = bs.run_chains_host(data, [4], 30, 10, 0.1, 0.01, **kw)[0]
    dev = bs.run_chains(engine, data, [4], 30, 10, 0.1, 0.01, **kw)[0]
    assert np.array_equal(host["assignments"], dev["assignments"])
    assert ulps32(host["params"], dev["params"]).max() <= 1
    assert np.array_equal(host["DP_alpha"][0], dev["DP_alpha"][0]) and np.allclose(host["DP_alpha"], dev["DP_alpha"], rtol=1e-12, atol=0)
    model = bs.Model(data, 0.1, 0.01, **kw)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    assert (np.abs(host["ML"] - dev["ML"]) <= bound(n_obs, np.abs(host["ML"]))).all()         # every term of ML is negative: sum |term| = |ML|
    for s in range(10, 31):
        # MAP adds the prior's terms: per live cluster and mutation one beta log density, per cluster two logs below 10, one gamma log density
        k = len(np.unique(host["assignments"][s]))
        terms = np.abs(bs.beta_logpdf(host["params"][s - 10][:k], 0.25, 0.25)).sum() + 10.0 * k + abs(float(bs.alpha_logpdf(model, host["DP_alpha"][s])))
        assert np.isfinite(host["MAP"][s]) and abs(host["MAP"][s] - dev["MAP"][s]) <= bound(n_obs + k * model.M + 2 * k + 1, abs(host["ML"][s]) + terms)


# ---- the script ---------------------------------------------------------------------------------------------------------------------------
def test_script_device_sampler(tmp_path, planted):
    _, truth = planted
    out = str(tmp_path / "out")
    r = run_script([FIXTURE_TSV, "--sampler", "device", "-smp", "0", "--no_plots", "-FN", "0.1", "-FP", "0.01", "-pp", "1", "1", "-n", "2", "-s", "300", "--seed", "1",
                    "-o", out, "-v", "0", "--bnpc_libs", str(tmp_path / "nowhere")])
    assert r.returncode == 0, r.stderr
    row = pd.read_csv(os.path.join(out, "assignment.txt"), sep="\t").iloc[0]
    assert same_partition([int(x) for x in row["Assignment"].split()], truth)
    assert os.path.exists(os.path.join(out, "errors.txt")) and os.path.exists(os.path.join(out, "genotypes_posterior_mean.tsv"))
    r = run_script([FIXTURE_TSV, "--sampler", "device", "-smp", "0.33", "--no_plots", "-FN", "0.1", "-FP", "0.01", "-o", out, "--bnpc_libs", str(tmp_path / "nowhere")])
    assert r.returncode != 0 and "--split_merge_prob" in r.stderr and "-smp 0" in r.stderr
