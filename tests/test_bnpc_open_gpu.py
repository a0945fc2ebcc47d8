"""Chains of open length on the device: lsg_bnpcs_extend, lsg_bnpcs_psrf (csrc/bnpc_sampler.hip: k_bnpcs_restride, k_bnpcs_psrf) and the
Lugsail and Runtime stop rules of longsom_amd.bnpc_sampler.run_chains, which tests/test_bnpc_open_cpu.py holds to the reference on the twin.

A chain's draws are a function of (seed, step, purpose), so a run that is extended must be, bit for bit, the run a create of the final
length makes: that is what the extension tests compare.  The PSRF kernel sums ML - ML[first] in double as the twin does, in another
order: the two may differ by some n 2^-53 of a sum whose terms are of the deviations' own size, far inside the 1e-9 the PSRF is held to."""
import os

import numpy as np
import pytest

from longsom_amd import bnpc_sampler as bs
from tests.test_bnpc_cpu import run_script
from tests.test_bnpc_open_cpu import RUN, SCRIPTS, SEEDS, WIDE, Clock, same_psrf, value_cases
from tests.test_bnpc_sampler_cpu import GOLD
from tests.test_bnpc_sampler_gpu import FIXTURE_TSV, random_data

pytestmark = pytest.mark.gpu

KEYS = ("assignments", "params", "DP_alpha", "ML", "MAP", "FN", "FP", "sm_moves", "error_moves", "variate_errors", "burn_in")


def same_chains(a, b, keys=KEYS):
    for x, y in zip(a, b):
        for k in keys:
            assert np.asarray(x[k]).dtype == np.asarray(y[k]).dtype and np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    assert len(a) == len(b)


@pytest.fixture(scope="module")
def small():
    with np.load(os.path.join(GOLD, "bnpcpsrf.runs.npz")) as z:
        return z["data"]


# ---- lsg_bnpcs_psrf -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chains", [1, 3, 16])
def test_psrf_statistics_equal_twin(engine, n_chains):
    """every series of the goldens (lengths 8 .. 4097, the constant one), n_chains at a time: chain c holds its series in the records that
    end at `last`, so first differs per chain wherever the lengths do"""
    pool = [s[b:] for chains, _ in value_cases().values() for s, b in chains]
    assert {8, 9, 10, 15, 16, 35, 36, 100, 1023, 1024, 1025, 4097} <= {len(x) for x in pool} and any(x.std() == 0 for x in pool)
    model = bs.Model(np.array([[1.0], [0.0]]), 0.2, 0.01)
    room = 4097 + 40
    engine.bnpcs_create(model, list(range(1, n_chains + 1)), room - 1, 64)
    worst, finite, infinite, differ = 0.0, 0, 0, 0
    for g in range(0, len(pool), n_chains):
        group = [pool[(g + c * 7) % len(pool)] if c else pool[g] for c in range(n_chains)]
        last = max(len(x) for x in group) + g % 37                    # not always at the start of the records
        first = [last - len(x) for x in group]
        for c, x in enumerate(group):
            engine.bnpcs_test_set_ml(c, first[c], x)
        stats = engine.bnpcs_psrf(first, last)
        twin = np.array([bs.ml_stats(x, 0) for x in group])
        assert np.array_equal(stats[:, 0], twin[:, 0]) and np.abs(stats[:, 1] - twin[:, 1]).max() <= 1e-9
        got, want = bs.psrf_of_stats(stats), bs.psrf_of_stats(twin)
        assert same_psrf(got, want), (g, got, want)
        differ += len(set(first)) > 1
        if np.isfinite(want):
            worst, finite = max(worst, abs(got - want) / want), finite + 1
        else:
            infinite += 1
    print("chains %d: %d finite values, %d inf, largest relative deviation %.3g" % (n_chains, finite, infinite, worst))
    assert finite and infinite and (differ or n_chains == 1)
    engine.bnpcs_destroy()


def test_psrf_over_the_golden_cases_equals_the_reference(engine):
    """the goldens' own cases, burn-ins and all: the device's statistics give the reference's value"""
    model = bs.Model(np.array([[1.0], [0.0]]), 0.2, 0.01)
    for name, (chains, want) in value_cases().items():
        last = max(len(s) for s, _ in chains)                         # one `last` for all chains: every series ends there
        engine.bnpcs_create(model, list(range(len(chains))), last - 1, 64)
        for c, (s, _) in enumerate(chains):
            engine.bnpcs_test_set_ml(c, last - len(s), s)
        got = bs.psrf_of_stats(engine.bnpcs_psrf([last - len(s) + b for s, b in chains], last))
        print(name, "reference", want, "device", got)
        assert same_psrf(got, want), name
    engine.bnpcs_destroy()


def test_psrf_and_extend_refusals(engine):
    engine.bnpcs_destroy()
    with pytest.raises(Exception, match="lsg_bnpcs_extend"):
        engine.bnpcs_extend(5)                                        # before a create
    model = bs.Model(np.array([[1.0, 0.0], [0.0, np.nan]]), 0.2, 0.01)
    engine.bnpcs_create(model, [1, 2], 20, 64)
    for c in range(2):
        st = bs.initial_state(model, c + 1)
        engine.bnpcs_set_state(c, st.labels, st.theta, st.alpha)
    for add in (0, -3):
        with pytest.raises(Exception, match="lsg_bnpcs_extend"):
            engine.bnpcs_extend(add)
    with pytest.raises(Exception, match=r"lsg_bnpcs_extend.*2147483\d\d\d steps"):
        engine.bnpcs_extend(2 ** 31 - 10)                             # the steps it would reach are named
    assert engine.bnpcs_run(0, 12, 0) == 12
    assert engine.bnpcs_psrf([0, 3], 12)[:, 0].tolist() == [12, 9] and engine.bnpcs_psrf([12, 12], 12)[:, 0].tolist() == [0, 0]
    for first, last in (([0, 0], 13), ([0, 13], 12), ([-1, 0], 12), ([0, 0], -1)):
        with pytest.raises(Exception, match="lsg_bnpcs_psrf"):
            engine.bnpcs_psrf(first, last)
    with pytest.raises(Exception, match="lsg_bnpcs_test_set_ml"):
        engine.bnpcs_test_set_ml(0, 15, np.zeros(7))                  # past the room
    engine.bnpcs_extend(1)
    engine.bnpcs_test_set_ml(0, 15, np.zeros(7))
    engine.bnpcs_destroy()


# ---- lsg_bnpcs_extend -----------------------------------------------------------------------------------------------------------------------
def shape_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "tiny":
        return np.array([[1.0], [0.0]])
    if name == "holes":
        data = random_data(rng, 20, 65)
        data[7] = np.nan                                              # an all-missing cell
        data[:, 64] = np.nan                                          # an all-missing column, the only one of the second word
        return data
    return random_data(rng, 65, 130)


def drive(engine, model, seeds, arena_rows, create, plan, extend_when_full=0):
    """create with `create` steps, then the plan: an int n makes n records, ("extend", k) extends.  extend_when_full: the first time the arena
    fills, extend by that much BEFORE the fetch.  Returns everything the device recorded, and the number of fetches a full arena forced."""
    engine.bnpcs_create(model, seeds, create, arena_rows)
    engine.bnpcs_set_split_merge(0.33, 0.75, 0.25, 3)
    engine.bnpcs_set_error_learning(0.5, *WIDE)
    for c, seed in enumerate(seeds):
        st = bs.initial_state(model, seed)
        engine.bnpcs_set_state(c, st.labels, st.theta, st.alpha)
    rows, done, taken, forced = [[] for _ in seeds], 0, 0, 0

    def take():
        nonlocal taken
        labels, scalars, arena = engine.bnpcs_fetch()
        for c in range(len(seeds)):
            at = 0
            for s in range(taken, done):
                k = int(scalars[c, s, 3])
                rows[c].append(arena[c, at:at + k].copy())
                at += k
        taken = done
        return labels, scalars

    for op in plan:
        if isinstance(op, tuple):
            engine.bnpcs_extend(op[1])
            continue
        target = done + op
        while done < target:
            done += engine.bnpcs_run(done, target - done, 0)
            if done < target:
                if extend_when_full:
                    engine.bnpcs_extend(extend_when_full)
                    extend_when_full = 0
                forced += 1
                take()
    labels, scalars = take()
    rates, counts = engine.bnpcs_fetch_error_rates()
    out = dict(labels=labels, scalars=scalars, moves=engine.bnpcs_fetch_moves(), rates=rates, counts=counts, errors=engine.bnpcs_errors().copy(),
               rows=[np.concatenate([r.ravel() for r in rr]) for rr in rows], states=[engine.bnpcs_get_state(c) for c in range(len(seeds))])
    engine.bnpcs_destroy()
    return out, forced


@pytest.mark.parametrize("name", ["tiny", "holes", "two_words"])
def test_an_extended_run_is_the_longer_run(engine, name):
    data = shape_case(name)
    model = bs.Model(data, 0.2, 0.01, (0.25, 0.25), error_prob=0.5, error_priors=WIDE)
    seeds = [3, 4, 5, 6]
    arena = max(model.N, 3)                                           # a step's rows always fit, two steps' rarely: fetches fall inside the run
    whole, forced = drive(engine, model, seeds, arena, 10, [11])
    assert forced > 0 and whole["labels"].shape == (4, 11, model.N) and (whole["scalars"][:, :, 3] >= 1).all()
    assert whole["moves"].any() or name == "tiny"
    grown, _ = drive(engine, model, seeds, arena, 3, [4, ("extend", 5), 5, ("extend", 2), 2])
    early, forced = drive(engine, model, seeds, arena, 3, [("extend", 5), 9, 2], extend_when_full=2)      # before any step; then with a full arena and a step pending
    assert forced > 0
    for other in (grown, early):
        for k in ("labels", "scalars", "moves", "rates", "counts", "errors"):
            assert other[k].shape == whole[k].shape and other[k].tobytes() == whole[k].tobytes(), k
        for c in range(4):
            assert other["rows"][c].tobytes() == whole["rows"][c].tobytes()
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(other["states"][c], whole["states"][c]))


# ---- the stop rules ---------------------------------------------------------------------------------------------------------------------------
def test_lugsail_on_the_device(engine, small):
    seen = []
    stop = bs.Lugsail(1.2, extend=20, report=lambda n, v: seen.append((n, v)))
    out = bs.run_chains(engine, small, SEEDS, None, None, 0.2, 0.01, arena_rows=40, stop=stop, **RUN)
    checks = out[0]["PSRF"]
    records = len(out[0]["ML"])
    print("checks", checks)
    assert stop.first_steps == 10 and [n for n, _ in checks] == [11 + 20 * k for k in range(len(checks))] and records == checks[-1][0] and seen == checks
    assert all(v > 1.2 for _, v in checks[:-1]) and checks[-1][1] <= 1.2 and len(checks) >= 2
    for r in out:
        assert r["burn_in"] == records // 2 + 1 and r["params"].shape[0] == records - r["burn_in"] and r["PSRF"] == checks and r["PSRF_cutoff"] == 1.2
        assert r["assignments"].shape == (records, 30) and r["MAP"].shape == (records,)
    for n, v in checks:
        assert same_psrf(bs.lugsail_psrf([(r["ML"][:n], n // 2) for r in out]), v)
    whole = bs.run_chains(engine, small, SEEDS, records - 1, 0, 0.2, 0.01, **RUN)
    for r, w in zip(out, whole):
        assert r["params"].tobytes() == w["params"][r["burn_in"]:].tobytes()
        w["params"], w["burn_in"] = r["params"], r["burn_in"]
    same_chains(out, whole)


@pytest.mark.parametrize("times,batch,records,burn_in,reads", SCRIPTS)
def test_runtime_on_the_device(engine, small, times, batch, records, burn_in, reads):
    clock = Clock(times)
    out = bs.run_chains(engine, small, SEEDS, None, None, 0.2, 0.01, stop=bs.Runtime(10, 4, clock, batch), **RUN)
    assert clock.reads == reads and all(len(r["ML"]) == records and r["burn_in"] == burn_in and r["params"].shape[0] == records - burn_in for r in out)
    same_chains(out, bs.run_chains(engine, small, SEEDS, records - 1, burn_in, 0.2, 0.01, **RUN))
    with pytest.raises(ValueError, match="no step"):
        bs.run_chains(engine, small, SEEDS, None, None, 0.2, 0.01, stop=bs.Runtime(10, 4, Clock((0, 11)), batch), **RUN)


def test_a_refused_extension_ends_the_run_with_an_error(engine, small, monkeypatch):
    from longsom_amd._lib import LsgError

    def refuse(add):
        raise LsgError("lsg_bnpcs_extend failed (rc=-2): no room")
    monkeypatch.setattr(engine, "bnpcs_extend", refuse)
    with pytest.raises(RuntimeError, match=r"after 11 steps the PSRF is inf.*no room"):
        bs.run_chains(engine, small, SEEDS, None, None, 0.2, 0.01, stop=bs.Lugsail(1.2, extend=20), **RUN)


def test_device_open_without_a_rule_is_device_errors(small):
    """--sampler device-open with neither -ls nor -r returns --sampler device-errors' chains"""
    from datetime import datetime
    from longsom_amd import cli
    runs = []
    for sampler in ("device-errors", "device-open"):
        a = cli._bnpc_parser().parse_args(["in.tsv", "--sampler", sampler, "-n", "3", "-s", "25", "--seed", "5", "-v", "0"])
        a.time = [datetime.now()]
        cli._device_sampler_refusals(a)
        runs.append(cli._device_chains(a, small))
    assert runs[0][0]["error_moves"].sum() > 0 and len(runs[0][0]["ML"]) == 26 and "PSRF" not in runs[1][0]
    same_chains(runs[0], runs[1])


def test_script_device_open(tmp_path):
    out = str(tmp_path / "out")
    r = run_script([FIXTURE_TSV, "--sampler", "device-open", "-ls", "1.2", "-s", "7", "-n", "3", "--seed", "1", "--no_plots", "-o", out, "-v", "2",
                    "--bnpc_libs", str(tmp_path / "nowhere")])
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("\tPSRF at ")]
    print(r.stdout)
    assert len(lines) >= 2 and lines[0].startswith("\tPSRF at 11:\tinf") and lines[1].startswith("\tPSRF at 211:\t") and "until PSRF < 1.2000" in r.stdout
    assert float(lines[-1].split("\t")[-1]) <= 1.2 and all(float(l.split("\t")[-1]) > 1.2 for l in lines[:-1])
    for f in ("assignment.txt", "errors.txt", "genotypes_posterior_mean.tsv"):
        assert os.path.exists(os.path.join(out, f)), f
