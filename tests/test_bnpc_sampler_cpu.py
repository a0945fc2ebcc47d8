"""CPU: the numpy twin of BnpC's sampler (longsom_amd.bnpc_sampler) held to the reference's own methods.

tests/golden/bnpcs.states.npz holds what CRP.py's methods return in given states (tools/make_bnpc_sampler_goldens.py ran them, unmodified).
The twin multiplies counts and uses matrix products where the reference adds per cell, so a value that is a sum of n terms is compared
with the bound  |a - b| <= (n + 4) 2^-52 sum |term|:  n roundings of a reordered sum, and a few ulp of log in the terms themselves."""
import os

import numpy as np
import pytest

from longsom_amd import bnpc, bnpc_sampler as bs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("uniform_neg", "quarter_given", "uniform_given", "quarter_neg")
ULP = 2.0 ** -52


def bound(n, mag):
    return (n + 4) * ULP * mag


@pytest.fixture(scope="module")
def states():
    with np.load(os.path.join(GOLD, "bnpcs.states.npz")) as z:
        return {k: z[k] for k in z.files}


def load_case(states, name):
    g = {k.split(".", 1)[1]: v for k, v in states.items() if k.startswith(name + ".")}
    model = bs.Model(g["data"], float(g["FN"]), float(g["FP"]), tuple(g["pp"]), tuple(g["ap"]))
    return g, model, bs.State(g["labels"], g["theta"], float(g["alpha"]))


def same_partition(a, b):
    return len(set(zip(a, b))) == len(set(a)) == len(set(b))


# ---- the stream ------------------------------------------------------------------------------------------------------------------
def philox_scalar(key, ctr):
    """Philox4x32-10 in plain Python integers"""
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    c = list(ctr)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def test_philox_known_answers():
    """Random123's published vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), 0, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xFFFFFFFF,) * 4, 0xFFFFFFFFFFFFFFFF, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd))]
    for ctr, key, want in kat:
        assert tuple(philox_scalar(key, ctr)) == want
        assert tuple(int(w) for w in bs.philox(key, *ctr)) == want


def test_philox_twin_equals_scalar():
    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 2 ** 32, (200, 4), dtype=np.uint64)
    key = 0x0123456789ABCDEF
    got = bs.philox(key, ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3])
    for i in range(len(ctr)):
        assert [int(w[i]) for w in got] == philox_scalar(key, [int(x) for x in ctr[i]])


def test_uniforms_lie_strictly_inside_the_unit_interval():
    lo = np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF], np.uint32); hi = np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    u = bs.to_double(lo, hi)
    assert u.min() > 0 and u.max() < 1 and u[0] == 2.0 ** -53 and u[3] == 1 - 2.0 ** -53
    a, b = bs.doubles(5, np.arange(100000), 2, bs.P_CHOICE)
    assert 0 < min(a.min(), b.min()) and max(a.max(), b.max()) < 1
    assert abs(a.mean() - 0.5) < 0.01 and abs(b.mean() - 0.5) < 0.01


def test_truncnorm_logpdf_equals_scipy():
    """[TMIN, TMAX] holds the location, so the mass is at least 0.47 and its log is well conditioned; z^2 / 2 reaches 50 at sd 0.1: a few
    ulp of 50 is the error to expect, 1e-12 bounds it"""
    from scipy.stats import truncnorm
    rng = np.random.default_rng(4)
    for sd in bs.PROPOSAL_SD:
        loc = np.concatenate([[bs.TMIN32, np.float32(0.5), bs.TMAX32], rng.random(200).astype(np.float32)]).astype(np.float32)
        x = np.clip(rng.random(len(loc)), bs.TMIN, bs.TMAX).astype(np.float32)
        a, b = (bs.TMIN - loc) / sd, (bs.TMAX - loc) / sd
        want = truncnorm.logpdf(x, a, b, loc=loc, scale=sd)
        assert np.abs(bs.truncnorm_logpdf(x, loc, sd) - want).max() <= 1e-12


def test_variates_follow_their_laws():
    from scipy import stats
    idx = np.arange(20000)
    for a, b in ((1, 1), (0.25, 1.25), (50.25, 30.25)):
        x, err = bs.beta_variate(9, a, b, idx, 0, bs.P_BIRTH)
        assert err == 0 and stats.kstest(x, stats.beta(a, b).cdf).pvalue > 1e-4
    u, _ = bs.doubles(9, idx, 0, bs.P_MH)
    for old in (bs.TMIN32, np.float32(0.5), bs.TMAX32):
        x = bs.truncnorm_variate(u, old, 0.25).astype(np.float64)
        a, b = (bs.TMIN - old) / 0.25, (bs.TMAX - old) / 0.25
        assert stats.kstest(x, stats.truncnorm(a, b, loc=old, scale=0.25).cdf).pvalue > 1e-4


# ---- the methods against the reference's -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_constants(states, name):
    g, model, st = load_case(states, name)
    assert np.abs(model.mix - g["mix"]).max() <= 4 * ULP
    assert (model.g0, model.g1) == tuple(g["dp_gamma"]) and model.alpha0 == float(g["alpha0"])
    sizes = np.append(np.arange(1, model.N + 1), st.alpha)
    assert np.array_equal(np.append(0, bs.crp_prior(sizes, model.N, st.alpha)), g["crp_prior"])


@pytest.mark.parametrize("name", CASES)
def test_new_cluster_posterior(states, name):
    g, model, st = load_case(states, name)
    got = model.new_cluster_ll() + (np.log(st.alpha) - np.log(model.N - 1 + st.alpha))
    t1, t0 = np.log(model.mix[1] * (1 - model.FN) + model.mix[0] * model.FP), np.log(model.mix[1] * model.FN + model.mix[0] * (1 - model.FP))
    mag = model.pop1 * abs(t1) + model.pop0 * abs(t0) + abs(np.log(st.alpha)) + abs(np.log(model.N - 1 + st.alpha))
    assert (np.abs(got - g["new_post"]) <= bound(model.pop1 + model.pop0 + 2, mag)).all()
    assert (model.pop1 + model.pop0 == 0).any(), "the case holds an all-missing cell"


@pytest.mark.parametrize("name", CASES)
def test_lpost_single_and_normalisation(states, name):
    g, model, _ = load_case(states, name)
    seen_death = False
    for i in range(model.N):
        st = bs.State(g["labels"], g["theta"], float(g["alpha"]))
        st.sizes[st.labels[i]] -= 1
        live = st.live()
        k = len(live)
        seen_death |= k < g["lpost"].shape[1]
        assert np.array_equal(live, g["lpost_ids"][i, :k]) and (g["lpost_ids"][i, k:] == -1).all()
        got = bs.lpost_single(model, st, i, live)
        L1, L0 = bs.log_tables(st.theta[live], model.FN, model.FP)
        mag = np.abs(L1) @ model.one_f[i] + np.abs(L0) @ model.zero_f[i] + np.abs(np.log(st.sizes[live])) + abs(np.log(model.N - 1 + st.alpha))
        assert (np.abs(got - g["lpost"][i, :k]) <= bound(model.pop1[i] + model.pop0[i] + 2, mag)).all()
        # _normalize_log_probs of the reference's own input: K + 1 exponentials, a log1p and an exp of a value of size |log p|
        want = g["probs"][i, :k + 1]
        p = bs.normalize_log_probs(np.append(g["lpost"][i, :k], g["new_post"][i]))
        assert (np.abs(p - want) <= bound(k + 1, want * np.maximum(1.0, np.abs(np.log(want))))).all()
    assert seen_death, "the case holds a one-cell cluster"


@pytest.mark.parametrize("name", CASES)
def test_log_A(states, name):
    g, model, st = load_case(states, name)
    n1, n0 = bs.counts(model, st)
    live = st.live()
    assert ((n1[live] + n0[live]).sum(axis=0) == 0).any(), "the case holds an all-missing column"
    A, mag = bs.log_A(model, g["mh_new"], st.theta[live], n1[live], n0[live], g["mh_sd"], terms=True)
    n = 2 * st.sizes[live][:, None] + 6
    assert (np.abs(A - g["mh_A"]) <= bound(n, mag)).all()


@pytest.mark.parametrize("name", CASES)
def test_likelihood_and_prior(states, name):
    g, model, st = load_case(states, name)
    ll, mag = bs.likelihood(model, st.labels, st.theta[st.live()])
    assert abs(ll - float(g["ll_full"])) <= bound(int(model.pop1.sum() + model.pop0.sum()), mag)
    crp, bsum = bs.prior_parts(model, st)
    a = float(bs.alpha_logpdf(model, st.alpha))
    live = st.live()
    terms = np.concatenate([[a], np.log(st.sizes[live]), np.full(len(live), np.log(model.N - 1 + st.alpha)),
                            [] if model.uniform else bs.beta_logpdf(st.theta[live], model.p, model.q).ravel()])
    assert np.isfinite(float(g["lprior_full"]))
    assert abs(a + crp + bsum - float(g["lprior_full"])) <= bound(len(terms), np.abs(terms).sum())


# ---- the twin's run ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    with np.load(os.path.join(GOLD, "bnpcs.fixture.npz")) as z:
        return z["data"], z["truth"]


def test_the_run_recovers_the_planted_partition(planted):
    data, truth = planted
    assert data.shape == (60, 40) and np.array_equal(truth, np.arange(60) % 3)
    res = bs.run_chains_host(data, [1, 2], 300, 100, 0.1, 0.01)
    for r in res:
        assert r["assignments"].shape == (301, 60) and r["params"].shape[0] == 201 and r["variate_errors"] == 0
        assert r["assignments"].min() >= 0 and r["assignments"].max() < 60
    cat = bnpc.concat_chains(res)
    est = bnpc.posterior_estimate_host(cat["assignments"], cat["params"], data, cat["DP_alpha"], cat["FN"], cat["FP"])
    assert same_partition(est["assignment"], truth)


def test_the_same_seeds_give_the_same_bytes(planted):
    data, _ = planted
    a = bs.run_chains_host(data, [5, 6], 12, 4, 0.1, 0.01, pp=(0.25, 0.25))
    b = bs.run_chains_host(data, [5, 6], 12, 4, 0.1, 0.01, pp=(0.25, 0.25))
    for ra, rb in zip(a, b):
        for k in ("assignments", "params", "DP_alpha", "ML", "MAP", "FN", "FP"):
            assert ra[k].tobytes() == rb[k].tobytes()
    assert not np.array_equal(a[0]["assignments"], a[1]["assignments"])
    assert np.array_equal(a[1]["assignments"], bs.run_chains_host(data, [6], 12, 4, 0.1, 0.01, pp=(0.25, 0.25))[0]["assignments"])


def test_the_start_is_the_reference_s(planted):
    """init(mode='random'): labels compacted to 0 .. K-1, parameters clipped uniforms on the live rows and zero elsewhere; DP_a at the
    prior's mean, which for a negative -ap is sqrt(N) + 1"""
    data, _ = planted
    model = bs.Model(data, 0.1, 0.01)
    st = bs.initial_state(model, 3)
    k = st.labels.max() + 1
    assert np.array_equal(np.unique(st.labels), np.arange(k)) and 20 < k < 60
    assert (st.theta[:k] >= np.float32(bs.TMIN)).all() and (st.theta[:k] <= np.float32(bs.TMAX)).all() and not st.theta[k:].any()
    assert st.alpha == np.sqrt(60) + 1
    assert bs.Model(data, 0.1, 0.01, dpa=(0.001, 5.0)).alpha0 == 5.001


def test_refusals(planted):
    data, _ = planted
    with pytest.raises(ValueError, match="65536"):
        bs.Model(np.zeros((65536, 1)), 0.1, 0.01)
    with pytest.raises(ValueError, match="0, 1 or NaN"):
        bs.Model(np.full((3, 3), 2.0), 0.1, 0.01)
    with pytest.raises(ValueError, match="burn_in"):
        bs.run_chains_host(data, [1], 5, 6, 0.1, 0.01)


def test_script_names_what_the_device_sampler_does_not_do(tmp_path):
    """--sampler device refuses each move it lacks with a message that names the flag, before any device is opened"""
    from tests.test_bnpc_cpu import run_script
    inp = os.path.join(GOLD, "bnpcs.fixture.BinaryMatrix.tsv")
    base = [inp, "--sampler", "device", "--no_plots", "-o", str(tmp_path / "o"), "--bnpc_libs", str(tmp_path / "nowhere")]
    for extra, words in ((["-smp", "0.33"], ("--split_merge_prob", "-smp 0")), ([], ("--split_merge_prob", "-smp 0")),
                         (["-smp", "0", "-eup", "0.25"], ("--error_update_prob", "-eup 0")), (["-smp", "0", "-eup", "0", "-fa", "x.txt"], ("--fixed_assignment",)),
                         (["-smp", "0", "-eup", "0", "-r", "5"], ("--runtime",)), (["-smp", "0", "-eup", "0", "-ls", "1.05"], ("--lugsail",)),
                         (["-smp", "0", "-eup", "0", "-sc"], ("--single_chains",))):
        r = run_script(base + extra)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (extra, r.stderr)
    assert not (tmp_path / "o").exists()
