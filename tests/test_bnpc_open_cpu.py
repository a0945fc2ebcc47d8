"""CPU: the chains of open length (longsom_amd.bnpc_sampler's Lugsail and Runtime stop rules) and the lugsail batch-means PSRF.

tests/golden/bnpcpsrf.values.npz holds what the reference's utils.get_lugsail_batch_means_est returns on listed series, and
bnpcpsrf.runs.npz two runs of its MCMC.run((cutoff, 0), ...) (tools/make_bnpc_psrf_goldens.py ran both, unmodified).

The tolerance of a PSRF, 1e-9 relative: the reference forms a batch mean's deviation from the raw values, so its rounding is at most
b^1.5 2^-53 |mean| / sd relative to the deviation's own size: 6e-10 for n <= 4097 (b = 64) and |mean| / sd <= 1e4.  The twin sums
x - x[first], which carries none of it.  Both conditions are asserted on the goldens' series."""
import os

import numpy as np
import pytest

from longsom_amd import bnpc_sampler as bs
from tests.test_bnpc_sampler_cpu import GOLD

WIDE = (0.01, 0.01, 0.2, 0.1)
LENGTHS = (8, 9, 10, 15, 16, 35, 36, 100, 1023, 1024, 1025, 4097)
RUN = dict(pp=(0.25, 0.25), dpa_prob=0.25, sm_prob=0.33, error_prob=0.25, error_priors=WIDE)      # the model of the goldens' runs
SEEDS = [11, 12, 13]


def value_cases():
    with np.load(os.path.join(GOLD, "bnpcpsrf.values.npz")) as z:
        names = sorted({k.rsplit(".", 1)[0] for k in z.files})
        return {n: ([(z["%s.s%d" % (n, i)], int(z["%s.b%d" % (n, i)])) for i in range(int(z[n + ".n"]))], float(z[n + ".psrf"])) for n in names}


@pytest.fixture(scope="module")
def values():
    return value_cases()


@pytest.fixture(scope="module")
def runs():
    with np.load(os.path.join(GOLD, "bnpcpsrf.runs.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def host_lugsail(runs):
    """one Lugsail run of the twin on the goldens' 30 x 12 data, and the Steps run of its length without burn-in"""
    seen = []
    out = bs.run_chains_host(runs["data"], SEEDS, None, None, 0.2, 0.01, stop=bs.Lugsail(1.05, report=lambda n, v: seen.append((n, v))), **RUN)
    records = len(out[0]["ML"])
    return out, bs.run_chains_host(runs["data"], SEEDS, records - 1, 0, 0.2, 0.01, **RUN), seen


def same_psrf(got, want):
    return np.isinf(got) if np.isinf(want) else abs(got - want) <= 1e-9 * want


def test_twin_equals_the_reference_on_listed_series(values):
    assert {"len%d" % n for n in LENGTHS} <= set(values) and {"constant", "below1", "mixed", "rho0.99"} <= set(values)
    worst = 0.0
    for name, (chains, want) in values.items():
        for s, b in chains:
            kept = s[b:]
            assert kept.size <= 4097 and (kept.std() == 0 or abs(kept.mean()) / kept.std(ddof=1) <= 1e4), name
        got = bs.lugsail_psrf(chains)
        print(name, [len(s) - b for s, b in chains], "reference", want, "twin", got)
        assert same_psrf(got, want), name
        if np.isfinite(want):
            worst = max(worst, abs(got - want) / want)
    print("largest relative deviation %.3g" % worst)
    assert np.isinf(values["len8"][1]) and np.isinf(values["constant"][1]) and np.isinf(values["short_one"][1]) and values["below1"][1] < 1
    assert len({b for _, b in values["len100"][0]}) > 1


def test_twin_equals_the_reference_on_its_own_runs(runs):
    for name, first in (("ls105", 10), ("ls101", 49)):
        cutoff, ML = float(runs[name + ".cutoff"]), runs[name + ".ML"]
        steps, want = runs[name + ".psrf_steps"], runs[name + ".psrf_values"]
        assert bs.Lugsail(cutoff).first_steps == first and steps[0] == first + 1 and (np.diff(steps) == 200).all() and ML.shape == (3, steps[-1])
        for k, (n, v) in enumerate(zip(steps, want)):
            got = bs.lugsail_psrf([(m[:n], n // 2) for m in ML])
            print(name, n, "reference", v, "twin", got)
            assert same_psrf(got, v) and (got <= cutoff) == (v <= cutoff) == (k == len(steps) - 1)
        # the shapes the rule leaves behind (MCMC.py:173-177)
        burn_in = int(runs[name + ".burn_in"])
        assert burn_in == steps[-1] // 2 + 1 and (runs[name + ".params_shape"][:, 0] == steps[-1] - burn_in).all() and (runs[name + ".assign_shape"][:, 0] == steps[-1]).all()


def test_statistics_and_their_combination():
    rng = np.random.default_rng(3)
    x = -1e4 + rng.standard_normal(50)
    n, mean, var, tau, tau3 = bs.ml_stats(x, 10)
    kept = x[10:]
    assert n == 40 and abs(mean - kept.mean()) < 1e-9 and abs(var - kept.var(ddof=1)) < 1e-9
    bm = kept[:36].reshape(6, 6).mean(axis=1)
    assert abs(tau - 6 / 5 * np.square(bm - kept.mean()).sum()) < 1e-9
    bm = kept.reshape(20, 2).mean(axis=1)
    assert abs(tau3 - 2 / 19 * np.square(bm - kept.mean()).sum()) < 1e-9
    assert np.array_equal(bs.ml_stats(x, 50), np.zeros(5)) and bs.ml_stats(x, 45)[0] == 5
    assert bs.psrf_of_stats([[8, 0, 1, 1, 1]]) == np.inf and bs.psrf_of_stats([[9, 0, 0, 0, 0]]) == np.inf        # too short; variance 0
    assert bs.psrf_of_stats([[9, 0, 1.0, 0.0, 100.0]]) == np.inf                                                    # a negative quotient
    assert bs.psrf_of_stats([[9, 0, 2.0, 2.0, 2.0], [10, 0, 2.0, 2.0, 2.0]]) == 1.0                                # n = round(9.5) = 10, T_L = s


def test_lugsail_on_the_host(host_lugsail):
    out, whole, seen = host_lugsail
    stop = bs.Lugsail(1.05)
    checks = out[0]["PSRF"]
    records = len(out[0]["ML"])
    print("checks", checks)
    assert (records - stop.first_steps - 1) % 200 == 0 and records == stop.first_steps + 1 + 200 * (len(checks) - 1)
    assert [n for n, _ in checks] == [stop.first_steps + 1 + 200 * k for k in range(len(checks))] and seen == checks
    assert all(v > 1.05 for _, v in checks[:-1]) and checks[-1][1] <= 1.05
    for r, w in zip(out, whole):
        assert r["burn_in"] == records // 2 + 1 and r["params"].shape[0] == records - r["burn_in"] and r["PSRF"] == checks and r["PSRF_cutoff"] == 1.05
        # the extension invariant: the extended chain is the chain of that length
        for k in ("ML", "MAP", "DP_alpha", "FN", "FP", "assignments", "sm_moves", "error_moves"):
            assert np.array_equal(r[k], w[k]), k
        assert np.array_equal(r["params"], w["params"][r["burn_in"]:]) and r["variate_errors"] == w["variate_errors"]
    for n, v in checks:
        assert same_psrf(bs.lugsail_psrf([(r["ML"][:n], n // 2) for r in out]), v)


def test_lugsail_refusals(runs):
    with pytest.raises(ValueError, match="cutoff"):
        bs.Lugsail(1.0)
    with pytest.raises(ValueError, match="extend"):
        bs.Lugsail(1.1, extend=0)
    with pytest.raises(ValueError, match="stop"):
        bs.run_chains_host(runs["data"], [1], None, None, 0.2, 0.01, stop=1.05)

    class NoRoom(bs._HostRun):
        def extend(self, add):
            raise MemoryError("no room")

    run = NoRoom(bs.Model(runs["data"], 0.2, 0.01, (0.25, 0.25)), [5, 6], [bs.initial_state(bs.Model(runs["data"], 0.2, 0.01, (0.25, 0.25)), s) for s in (5, 6)],
                 0.0, (0.75, 0.25), 3, False)
    with pytest.raises(RuntimeError, match=r"after 11 steps the PSRF is inf.*no room"):
        bs._drive(run, None, None, bs.Lugsail(1.05))


class Clock:
    """a scripted clock: returns the listed times one after the other"""

    def __init__(self, times):
        self.times, self.reads = list(times), 0

    def __call__(self):
        self.reads += 1
        return self.times.pop(0)


# end 10, burn-in ends at 4: (the clock's readings, batch) -> (records, burn_in, readings)
SCRIPTS = (((0, 1, 5, 9, 11), 4, 17, 9, 5),       # four batches; the third is the first to start at or after 4: kept from record 9
           ((4, 10, 10.5), 3, 7, 1, 3),           # a batch that starts AT the burn-in's end is kept, one that starts AT the end still runs
           ((0, 2, 3, 3.5, 6, 12), 1, 6, 5, 6))   # batches of one step: room grows from 1 step on


@pytest.mark.parametrize("times,batch,records,burn_in,reads", SCRIPTS)
def test_runtime_counts_on_the_host(runs, times, batch, records, burn_in, reads):
    clock = Clock(times)
    out = bs.run_chains_host(runs["data"], [5, 6], None, None, 0.2, 0.01, stop=bs.Runtime(10, 4, clock, batch), **RUN)
    assert clock.reads == reads
    whole = bs.run_chains_host(runs["data"], [5, 6], records - 1, burn_in, 0.2, 0.01, **RUN)
    for r, w in zip(out, whole):
        assert len(r["ML"]) == records == len(r["assignments"]) and r["burn_in"] == burn_in and r["params"].shape[0] == records - burn_in
        assert all(np.array_equal(r[k], w[k]) for k in ("ML", "MAP", "FN", "FP", "assignments", "params", "sm_moves"))


def test_runtime_that_keeps_nothing(runs):
    with pytest.raises(ValueError, match="no step"):
        bs.run_chains_host(runs["data"], [5], None, None, 0.2, 0.01, stop=bs.Runtime(10, 4, Clock((0, 3, 11)), 2), **RUN)
    with pytest.raises(ValueError, match="no step"):
        bs.run_chains_host(runs["data"], [5], None, None, 0.2, 0.01, stop=bs.Runtime(10, 4, Clock((11,)), 2), **RUN)
    with pytest.raises(ValueError, match="batch"):
        bs.Runtime(10, 4, Clock(()), 0)


def parse(extra):
    from datetime import datetime
    from longsom_amd import cli
    a = cli._bnpc_parser().parse_args(["in.tsv", "--sampler", "device-open"] + extra)
    a.time = [datetime(2026, 1, 1, 12, 0, 0)]
    return cli, a


def test_arguments_map_to_a_stop_rule():
    from datetime import datetime
    cli, a = parse(["-ls", "1.05"])
    cli._device_sampler_refusals(a)
    stop, text = cli._device_stop_rule(a)
    assert isinstance(stop, bs.Lugsail) and stop.cutoff == 1.05 and stop.extend == 200 and stop.report is None and text == "until PSRF < 1.0500"
    cli, a = parse(["-ls", "1.05", "-v", "2"])
    assert cli._device_stop_rule(a)[0].report is not None
    cli, a = parse(["-r", "5", "-ls", "1.05", "-s", "77", "-b", "0.2"])               # -r wins over -ls, both over -s
    cli._device_sampler_refusals(a)
    stop, text = cli._device_stop_rule(a, clock=lambda: 0)
    assert isinstance(stop, bs.Runtime) and stop.end == datetime(2026, 1, 1, 12, 5, 0) and stop.burn_in_end == datetime(2026, 1, 1, 12, 1, 0) and text == "for 5 mins"
    cli, a = parse(["-s", "77", "-fa", "x.txt", "-eup", "0.3"])
    cli._device_sampler_refusals(a)                                                     # what device-errors takes, device-open takes
    assert cli._device_stop_rule(a) == (None, "for 77 steps")
    cli, a = parse(["-ls", "1"])
    with pytest.raises(SystemExit, match="--lugsail 1 "):
        cli._device_sampler_refusals(a)
    for sampler in ("device", "device-sm", "device-errors"):                            # the others still turn both away
        a = cli._bnpc_parser().parse_args(["in.tsv", "--sampler", sampler, "-smp", "0", "-eup", "0", "-ls", "1.05"])
        with pytest.raises(SystemExit, match="--lugsail"):
            cli._device_sampler_refusals(a)


def test_script_device_open_refusals(tmp_path):
    from tests.test_bnpc_cpu import run_script
    inp = os.path.join(GOLD, "bnpcs.fixture.BinaryMatrix.tsv")
    base = [inp, "--sampler", "device-open", "--no_plots", "-o", str(tmp_path / "o"), "--bnpc_libs", str(tmp_path / "nowhere")]
    for extra, words in ((["-sc"], ("--single_chains",)), (["-ls", "1"], ("--lugsail 1",))):
        r = run_script(base + extra)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (extra, r.stderr)
        assert "hip" not in r.stderr.lower()


def test_rule_file_and_docs_name_device_open():
    root = os.path.join(os.path.dirname(GOLD), "..")
    text = open(os.path.join(root, "workflow", "rules", "CellClustering.gpu.smk")).read()
    assert "--sampler device-open" in text and "-ls" in text and "lugsail" in text
    assert "lugsail" in open(os.path.join(root, "INTEGRATION.md")).read()
