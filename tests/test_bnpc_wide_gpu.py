"""BnpC on the device past 256 cells: csrc/bnpc_sampler.hip and csrc/bnpc.hip against their numpy twins at the widths where a lane of the
per-chain workgroups owns a run of ids in place of one (N, hi + 1 or K above 256), the likelihood matrix has more than 16 column tiles,
the record copies more than 256 clusters, the estimate's bitmap, prefix and ranks go past 256 and the pair tiles past four rows.

The cases and the twin's answers are tests/support/bnpc_wide_cases.py's; tests/test_bnpc_wide_cpu.py asserts on the twin alone that they
cross these widths and that no decision of the twin lies within 1e-9 of its edge.  The assertions and every tolerance are those of
tests/test_bnpc_sampler_gpu.py and tests/test_bnpc_gpu.py for the same quantities."""
import numpy as np
import pytest

from longsom_amd import bnpc_sampler as bs
from tests.support import bnpc_wide_cases as wc
from tests.test_bnpc_sampler_cpu import bound
from tests.test_bnpc_sampler_gpu import KEYS, load, ulps32

pytestmark = pytest.mark.gpu


# ---- one sweep from a loaded state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.SWEEP_CASES)
def test_one_wide_sweep_equals_twin(engine, name):
    model, chains = wc.swept(name)
    load(engine, model, wc.SWEEP_SEEDS, [ch["start"] for ch in chains])
    engine.bnpcs_test_move(0, wc.SWEEP_STEP)
    try:
        for c, ch in enumerate(chains):
            st = ch["end"]
            labels, theta, alpha = engine.bnpcs_get_state(c)
            differ = np.nonzero(labels != st.labels)[0]
            print(name, "seed", ch["seed"], "cells that differ", len(differ), differ[:8].tolist())
            assert np.array_equal(labels, st.labels)
            assert np.array_equal(np.bincount(labels, minlength=model.N), st.sizes)
            live = st.live()
            assert ulps32(theta[live], st.theta[live]).max() <= 1
            assert abs(alpha - st.alpha) <= 1e-12 * st.alpha
            # after the sweep: the counts over two or three workgroups of cells, the live list over runs of ids
            n1, n0 = engine.bnpcs_test_counts(c)
            w1, w0 = bs.counts(model, st)
            assert np.array_equal(n1, w1) and np.array_equal(n0, w0)
            ll, cols = engine.bnpcs_test_ll(c)
            assert np.array_equal(cols, live) and ll.shape == (model.N, len(live))
    finally:
        engine.bnpcs_destroy()


# ---- counts and the likelihood matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", wc.COUNT_SHAPES)
def test_wide_counts_and_likelihood_matrix(engine, N, K):
    for M in wc.COUNT_M:
        model, ids, st = wc.count_case(N, K, M)
        load(engine, model, [3], [st])
        try:
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
        finally:
            engine.bnpcs_destroy()


# ---- one parameter move from a loaded state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pp", wc.MOVE_PP)
@pytest.mark.parametrize("K", wc.MOVE_K)
def test_one_wide_parameter_move_equals_twin(engine, K, pp):
    for M in wc.MOVE_M:
        model, ids, labels, chains = wc.moved(K, M, pp)
        load(engine, model, wc.MOVE_SEEDS, [ch["start"] for ch in chains])
        try:
            engine.bnpcs_test_move(1, wc.MOVE_STEP)
            for c, ch in enumerate(chains):
                labels_d, theta, _ = engine.bnpcs_get_state(c)
                assert np.array_equal(labels_d, labels)
                assert ulps32(theta[ids], ch["end"].theta[ids]).max() <= 1
                assert (ch["end"].theta[ids] != ch["start"].theta[ids]).any()
        finally:
            engine.bnpcs_destroy()


# ---- a short run whose K crosses 256 --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_run(engine):
    return bs.run_chains(engine, wc.run_data(), [wc.RUN_SEED], wc.RUN_STEPS, wc.RUN_BURN_IN, wc.RUN_FN, wc.RUN_FP, **wc.RUN_KW)[0]


def test_wide_short_run_equals_twin(wide_run):
    host, dev = wc.run_host(), wide_run
    burn = wc.RUN_BURN_IN
    assert np.array_equal(host["assignments"], dev["assignments"])
    assert host["params"].shape == dev["params"].shape and ulps32(host["params"], dev["params"]).max() <= 1
    assert np.array_equal(host["DP_alpha"][0], dev["DP_alpha"][0]) and np.allclose(host["DP_alpha"], dev["DP_alpha"], rtol=1e-12, atol=0)
    model = bs.Model(wc.run_data(), wc.RUN_FN, wc.RUN_FP, **wc.RUN_KW)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    assert (np.abs(host["ML"] - dev["ML"]) <= bound(n_obs, np.abs(host["ML"]))).all()         # every term of ML is negative: sum |term| = |ML|
    for s in range(burn, wc.RUN_STEPS + 1):
        # MAP adds the prior's terms: per live cluster and mutation one beta log density, per cluster two logs below 10, one gamma log density
        k = len(np.unique(host["assignments"][s]))
        terms = np.abs(bs.beta_logpdf(host["params"][s - burn][:k], 0.25, 0.25)).sum() + 10.0 * k + abs(float(bs.alpha_logpdf(model, host["DP_alpha"][s])))
        assert np.isfinite(host["MAP"][s]) and abs(host["MAP"][s] - dev["MAP"][s]) <= bound(n_obs + k * model.M + 2 * k + 1, abs(host["ML"][s]) + terms)
    assert dev["variate_errors"] == 0


def test_wide_run_with_an_arena_that_overflows(engine, wide_run):
    """300 rows hold any one step of the run and not two: every kept step after the first finds the arena full and waits for a fetch"""
    small = bs.run_chains(engine, wc.run_data(), [wc.RUN_SEED], wc.RUN_STEPS, wc.RUN_BURN_IN, wc.RUN_FN, wc.RUN_FP, arena_rows=wc.RUN_SMALL_ARENA, **wc.RUN_KW)[0]
    for k in KEYS:
        assert np.array_equal(wide_run[k], small[k]), k


# ---- the posterior estimate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,K", wc.ESTIMATE_SHAPES)
def test_wide_codist_and_mpear_against_twin(engine, N, S, K):
    e = wc.estimated(N, S, K)
    engine.bnpc_load_samples(e["a"], e["p"])
    try:
        assert np.array_equal(engine.bnpc_codist(), e["D"])
        pairs, sim, dsum = engine.bnpc_mpear(e["cuts"])
        hp, hs, hd = e["sums"]
        assert np.array_equal(pairs, hp) and np.array_equal(sim, hs) and dsum == hd
        pairs0, sim0, dsum0 = engine.bnpc_mpear(np.zeros((0, N), np.int32))              # no cut: the distance sum alone
        assert len(pairs0) == 0 and dsum0 == hd
        for final, hw in e["finals"]:
            got = engine.bnpc_mean_params(final)
            assert np.array_equal(got[1], hw[1]) and np.array_equal(got[2], hw[2])
            sizes = np.unique(final, return_counts=True)[1]
            exact = hw[1] != 2
            assert np.array_equal(got[0][exact], hw[0][exact])
            rel = 4 * S * sizes[~exact, None] * 2.0 ** -53
            assert np.all(np.abs(got[0][~exact] - hw[0][~exact]) <= rel * np.abs(hw[0][~exact]))
    finally:
        engine.bnpc_unload()
