"""CPU: the error-rate update and the fixed assignment of the numpy twin (longsom_amd.bnpc_sampler) held to the reference's own methods.

tests/golden/bnpcs.errors.npz holds what CRP_learning_errors.py's methods return in given states (tools/make_bnpc_errors_goldens.py ran
them, unmodified).  The twin takes get_ll_full_error from the clusters' counts (K x M terms) where the reference adds N x M, so the two are
compared with the bound of tests/test_bnpc_sampler_cpu.py; the prior and transition densities are scalar formulas of the same ndtr and are
compared with rtol 1e-12."""
import os

import numpy as np
import pytest

from longsom_amd import bnpc_sampler as bs
from tests.test_bnpc_sampler_cpu import GOLD, bound

CASES = ("tiny", "holes_wide", "holes_tight", "gaps")
WIDE = (0.01, 0.01, 0.2, 0.1)


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLD, "bnpcs.errors.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def planted():
    with np.load(os.path.join(GOLD, "bnpcs.fixture.npz")) as z:
        return z["data"], z["truth"]


def load_case(gold, name):
    g = {k.split(".", 1)[1]: v for k, v in gold.items() if k.startswith(name + ".")}
    model = bs.Model(g["data"], float(g["FN"]), float(g["FP"]), tuple(g["pp"]), error_prob=0.5, error_priors=tuple(g["priors"]))
    return g, model, bs.State(g["labels"], g["theta"], float(g["alpha"]), float(g["FP"]), float(g["FN"]))


@pytest.mark.parametrize("name", CASES)
def test_likelihood_from_counts_equals_the_reference(gold, name):
    g, model, st = load_case(gold, name)
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    for (fp, fn), want in zip(g["ll_pairs"], g["ll"]):
        ll, mag = bs.error_ll(model, st, fp, fn)
        print(name, fp, fn, "ll", ll, "reference", want, "bound", bound(n_obs, mag))
        assert abs(ll - want) <= bound(n_obs, mag)


@pytest.mark.parametrize("name", CASES)
def test_prior_and_transition_densities_equal_the_reference(gold, name):
    """rtol 1e-12 holds on every listed value, the tail ones (1e-9, 1 - 1e-9: some 1e5 sds out) included: there the density is z^2 / 2 and
    the mass log(ndtr(b) - ndtr(a)) is the same small number in both forms"""
    g, model, st = load_case(gold, name)
    fm, fs, nm, ns = model.error_priors
    worst = 0.0
    for got, want in ((bs.unit_truncnorm_logpdf(g["prior_x"], fm, fs), g["prior_fp"]), (bs.unit_truncnorm_logpdf(g["prior_x"], nm, ns), g["prior_fn"]),
                      (bs.unit_truncnorm_logpdf(g["trans"][:, 1], g["trans"][:, 0], g["trans"][:, 2]), g["trans_new"]),
                      (bs.unit_truncnorm_logpdf(g["trans"][:, 0], g["trans"][:, 1], g["trans"][:, 2]), g["trans_old"])):
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
        assert np.allclose(got, want, rtol=1e-12, atol=0)
    print(name, "largest relative deviation of a density from scipy's truncnorm.logpdf: %.3g" % worst)
    both = bs.error_prior_logpdf(model, g["prior_x"], g["prior_x"])
    assert np.allclose(both, g["prior_fp"] + g["prior_fn"], rtol=1e-12, atol=0)
    assert np.isclose(float(g["lprior_full"]) - float(g["lprior_base"]), float(bs.error_prior_logpdf(model, st.FP, st.FN)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", CASES)
def test_A_reproduces_the_decisions_of_MH_error_rates(gold, name):
    g, model, st = load_case(gold, name)
    seen = set()
    for e, sd, new, v, accepted in zip(g["mh_rate"], g["mh_std"], g["mh_new"], g["mh_v"], g["mh_accept"]):
        out = bs.error_log_A(model, st, ("FP", "FN")[e], float(new), float(sd))
        assert abs(np.log(v) - out["A"]) > 100 * bs.error_bound_of_A(model, out), "a listed v lies at the edge"
        assert (np.log(v) < out["A"]) == bool(accepted), (e, sd, new, v, out)
        seen.add((int(e), bool(accepted)))
    assert seen == {(0, True), (0, False), (1, True), (1, False)}


def test_error_prob_zero_is_the_run_without_it(planted):
    data, _ = planted
    for sm_prob in (0.0, 0.33):
        kw = dict(pp=(0.25, 0.25), sm_prob=sm_prob)
        a = bs.run_chains_host(data, [3], 12, 4, 0.2, 0.01, **kw)[0]
        b = bs.run_chains_host(data, [3], 12, 4, 0.2, 0.01, error_prob=0.0, error_priors=WIDE, **kw)[0]
        assert set(a) == set(b)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        assert not a["error_moves"].any() and (a["FP"] == 0.01).all() and (a["FN"] == 0.2).all()


def test_learning_needs_its_priors_and_starts_at_their_means(planted):
    data, _ = planted
    with pytest.raises(ValueError, match="error_priors"):
        bs.run_chains_host(data, [1], 2, 1, 0.2, 0.01, error_prob=0.5)
    with pytest.raises(ValueError, match="means"):
        bs.run_chains_host(data, [1], 2, 1, 0.1, 0.01, error_prob=0.5, error_priors=WIDE)
    with pytest.raises(ValueError, match="error_prob"):
        bs.run_chains_host(data, [1], 2, 1, 0.2, 0.01, error_prob=1.5, error_priors=WIDE)


@pytest.fixture(scope="module")
def learned(planted):
    data, _ = planted
    return bs.run_chains_host(data, [1, 2], 30, 10, 0.2, 0.01, pp=(0.25, 0.25), sm_prob=0.33, error_prob=0.5, error_priors=WIDE)


def test_recorded_rates_follow_the_moves(planted, learned):
    data, _ = planted
    for seed, r in zip((1, 2), learned):
        assert r["FP"][0] == 0.01 and r["FN"][0] == 0.2 and r["variate_errors"] == 0
        assert ((r["FP"] > 0) & (r["FP"] < 1) & (r["FN"] > 0) & (r["FN"] < 1)).all()
        made = np.array([s > 0 and float(bs.doubles(seed, 0, s, bs.P_ERR)[0]) < 0.5 for s in range(31)])
        assert r["error_moves"][:2].sum() == r["error_moves"][2:].sum() == made.sum()
        for e, k in enumerate(("FP", "FN")):
            changed = np.nonzero(np.diff(r[k]))[0] + 1
            assert made[changed].all() and len(changed) == r["error_moves"][2 * e]
    assert all(r["error_moves"][0] > 0 and r["error_moves"][2] > 0 for r in learned[:1])


def test_MAP_holds_the_two_priors_at_the_recorded_rates(planted, learned):
    data, _ = planted
    model = bs.Model(data, 0.2, 0.01, (0.25, 0.25), error_prob=0.5, error_priors=WIDE)
    for r in learned:
        labels, alpha = r["assignments"], r["DP_alpha"]
        for s in range(10, 31):
            k = len(np.unique(labels[s]))
            st = bs.State(np.unique(labels[s], return_inverse=True)[1].reshape(-1), np.zeros((model.N, model.M), np.float32), alpha[s])
            st.theta[:k] = r["params"][s - 10][:k]
            crp, beta = bs.prior_parts(model, st)
            rest = float(bs.alpha_logpdf(model, alpha[s])) + crp + beta
            want = float(bs.error_prior_logpdf(model, r["FP"][s], r["FN"][s]))
            got = r["MAP"][s] - r["ML"][s] - rest
            # MAP and ML are sums of some N M terms each of magnitude |ML|: their difference keeps the priors' terms to that rounding
            assert abs(got - want) <= 64 * 2.0 ** -52 * (abs(r["ML"][s]) + abs(rest) + abs(want)), s
    assert len({float(bs.error_prior_logpdf(model, f, n)) for f, n in zip(learned[0]["FP"], learned[0]["FN"])}) > 1


def test_fixed_assignment_run(planted, tmp_path):
    data, truth = planted
    model = bs.Model(data, 0.2, 0.01, (0.25, 0.25))
    assign = truth * 3 + 2                                            # labels with gaps: compacted in ascending order
    runs = bs.run_chains_host(data, [5, 6], 20, 5, 0.2, 0.01, pp=(0.25, 0.25), sm_prob=0.33, error_prob=0.5, error_priors=WIDE, fixed_assignment=assign)
    for seed, r in zip((5, 6), runs):
        assert (r["assignments"] == truth[None, :]).all()
        assert not r["sm_moves"].any() and (r["DP_alpha"] == model.alpha0).all()
        assert r["error_moves"].sum() > 0 and r["params"].shape == (16, 3, model.M)
        st = bs.assigned_state(model, seed, assign)
        n1, n0 = bs.counts(model, bs.State(truth, np.zeros((model.N, model.M), np.float32), 1.0))
        b, _ = bs.beta_variate(seed, 0.25 + n1[:3], 0.25 + n0[:3], np.arange(model.M)[None, :], 0, bs.P_INIT_ASSIGN, np.arange(3)[:, None])
        assert np.array_equal(st.theta[:3], np.clip(b, bs.TMIN, bs.TMAX).astype(np.float32)) and np.array_equal(st.labels, truth)
        # step 0 records the start; burn-in hides its parameters, so a run without burn-in shows them
    first = bs.run_chains_host(data, [5], 1, 0, 0.2, 0.01, pp=(0.25, 0.25), fixed_assignment=assign)[0]
    assert np.array_equal(first["params"][0], bs.assigned_state(model, 5, assign).theta[:3])
    assert not np.array_equal(runs[0]["params"], runs[1]["params"])
    with pytest.raises(ValueError, match=r"59 labels.*60 cells"):
        bs.run_chains_host(data, [5], 2, 1, 0.2, 0.01, fixed_assignment=assign[:-1])
    # the file, as dpmmIO.load_txt reads it: an assignment.txt of the script, or blank-separated numbers
    table, plain = str(tmp_path / "assignment.txt"), str(tmp_path / "plain.txt")
    with open(table, "w") as f:
        f.write("chain\tAssignment\nmean\t%s\n" % " ".join(str(x) for x in assign))
    with open(plain, "w") as f:
        f.write(" ".join(str(x) for x in assign))
    assert bs.load_assignment(table) == list(assign) == bs.load_assignment(plain)


def test_script_device_errors_refusals(tmp_path):
    """--sampler device-errors takes -eup and -fa, and refuses -r, -ls and -sc by their names before a device is opened"""
    from tests.test_bnpc_cpu import run_script
    inp = os.path.join(GOLD, "bnpcs.fixture.BinaryMatrix.tsv")
    base = [inp, "--sampler", "device-errors", "--no_plots", "-o", str(tmp_path / "o"), "--bnpc_libs", str(tmp_path / "nowhere")]
    for extra, words in ((["-r", "5"], ("--runtime",)), (["-ls", "1.05"], ("--lugsail",)), (["-sc"], ("--single_chains",))):
        r = run_script(base + extra)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (extra, r.stderr)
        assert "--error_update_prob" not in r.stderr and "hip" not in r.stderr.lower()


def test_rule_file_names_the_sampler():
    rule = os.path.join(os.path.dirname(GOLD), "..", "workflow", "rules", "CellClustering.gpu.smk")
    text = open(rule).read()
    assert "--sampler device-errors" in text and "--sampler device-sm" in text and "--sampler device -smp 0" in text
