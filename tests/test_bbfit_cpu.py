"""CPU: the numpy twin of the beta-binomial fit (longsom_amd/bbfit.py) against the reference's own row extraction (a fixture made by
tools/make_bbfit_goldens.py from scripts/PoN/BetaBinEstimation.py), plain Python counts, the likelihood's root at 50 digits
(mpmath) and scipy's optimiser; the four statuses; the output file; the shim's parser.

Tolerance of the fit: 1e-7 relative in all four numbers - VGAM's own `epsilon`, the precision to which the reference itself fixes
them.  The generated inputs (tests/support/bbfit_cases.py) are conditioned so that the twin comes within 1e-10 of the root."""
import io
import os

import numpy as np
import pytest

from longsom_amd import bbfit, cli, tsvio
from tests.support import bbfit_cases as cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bbfit")


def fixture_rows():
    return tsvio.parse_counts_tsv(os.path.join(GOLD, "counts.tsv"), ["chr1", "chr2"])[:3]


def test_rows_kept_equal_the_reference_list_in_order():
    _, refs, counts = fixture_rows()
    v = bbfit.site_counts(refs, counts)
    keep = bbfit.kept(v[0], v[2], v[3], v[5])
    want = np.loadtxt(os.path.join(GOLD, "sites.expected.tsv"), skiprows=1, dtype=np.int64)
    assert 100 < len(want) < len(refs)
    assert np.array_equal(np.stack([v[0], v[1], v[3], v[4]], axis=1)[keep], want)
    # the fixture's edges: rows at exactly 0.10 and 0.15 are in the table and not in the list
    at_cc = (v[0] * 10 == v[2]) & (v[0] > 0)
    at_bc = (v[3] * 100 == v[5] * 15) & (v[3] > 0)
    assert at_cc.sum() >= 4 and at_bc.sum() >= 8 and not keep[at_cc].any() and not keep[at_bc].any()
    assert set(refs.tolist()) >= set(b"ACGTNRa") and not keep[np.isin(refs, list(b"NRa"))].any()


def test_n_and_o_planes_are_not_summed():
    """a table prints six alleles: counts of N and O never reach the reference's sums"""
    c = np.zeros((1, 42), np.uint32)
    c[0, 0], c[0, 1] = 100, 50
    c[0, 2], c[0, 10] = 45, 90                       # A (the REF)
    c[0, 8], c[0, 9], c[0, 16], c[0, 17] = 3, 2, 6, 4      # N, O
    v = bbfit.site_counts(b"A", c)
    assert [int(x[0]) for x in v] == [0, 50, 50, 0, 100, 100]


def test_histograms_equal_a_plain_count():
    rng = np.random.default_rng(5)
    n = 500
    counts = np.zeros((n, 42), np.uint32)
    refs = np.frombuffer(bytes(rng.choice(list(b"ACTGN"), n).astype(np.uint8)), np.uint8)
    counts[:, 0] = rng.integers(5, 300, n)
    counts[:, 1] = rng.integers(5, 60, n)
    counts[:, 2:8] = rng.integers(0, 3, (n, 6)) * (rng.random((n, 6)) < 0.2)
    counts[:, 10:16] = rng.integers(0, 9, (n, 6)) * (rng.random((n, 6)) < 0.2)
    counts[:, 8:10] = 7
    cap = 1024
    hist, seen, kept = bbfit.histograms(refs, counts, cap)
    want = np.zeros((6, cap), np.int64)
    n_kept = 0
    for i in range(n):
        dp, nc = int(counts[i, 0]), int(counts[i, 1])
        alt_cc = sum(int(counts[i, 2 + s]) for s in range(6) if "ACTGID"[s] != chr(refs[i]))
        alt_bc = sum(int(counts[i, 10 + s]) for s in range(6) if "ACTGID"[s] != chr(refs[i]))
        if alt_cc / float(nc) < 0.10 and alt_bc / float(dp) < 0.15:
            n_kept += 1
            for h, val in enumerate((alt_cc, nc - alt_cc, nc, alt_bc, dp - alt_bc, dp)):
                want[h, val] += 1
    assert seen == n and kept == n_kept and 50 < n_kept < n
    assert np.array_equal(hist.astype(np.int64), want)
    with pytest.raises(ValueError, match="capacity 200"):
        bbfit.histograms(refs, counts, 200)


def test_thinning_keeps_a_share_and_is_decided_before_the_filter():
    _, refs, counts = fixture_rows()
    n = len(refs)
    assert bbfit.thin(n, 0, 0, 1992).all() and bbfit.thin(n, 0, n, 1992).all()
    t = bbfit.thin(n, 3, 100, 1992)
    assert 60 < t.sum() < 140 and not np.array_equal(t, bbfit.thin(n, 4, 100, 1992)) and not np.array_equal(t, bbfit.thin(n, 3, 100, 7))
    hist, seen, kept = bbfit.histograms(refs, counts, 1024, table=3, sample_n=100, seed=1992)
    full, _, _ = bbfit.histograms(refs[t], counts[t], 1024)
    assert seen == t.sum() and np.array_equal(hist, full) and kept == int(hist[5].sum())
    assert bbfit.sample_size(500000, 7) == round(500000 / 7) and bbfit.sample_size(0, 7) == 0 and bbfit.sample_size(5, 2) == 2


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_solve_against_the_root_at_50_digits(name):
    hist = cases.shape_hist(name)
    est, infos = bbfit.solve(hist)
    assert [i["status"] for i in infos] == [bbfit.CONVERGED] * 2 and all(i["iterations"] < 30 for i in infos)
    root = cases.shape_roots(name)
    err = cases.rel(est, root)
    print(name, est, root, err, infos)
    assert err < 1e-10, "the inputs are conditioned for the twin to come within 1e-10"
    assert err <= 1e-7


def test_scipy_on_the_betaln_form_agrees():
    from scipy.optimize import minimize
    from scipy.special import betaln
    x, n = cases.draw(**cases.SHAPES["bases"])
    k = x / n.astype(np.float64) < 0.15
    x, n = x[k], n[k]
    hist = cases.shape_hist("bases")
    est, _ = bbfit.solve(hist)

    def nll(theta):
        a, b = np.exp(theta)
        return -float(np.sum(betaln(x + a, n - x + b) - betaln(a, b)))
    r = minimize(nll, np.log([0.5, 50.0]), method="Nelder-Mead", options=dict(xatol=1e-9, fatol=1e-12, maxiter=4000))
    assert r.success
    # Nelder-Mead's own tolerance: xatol 1e-9 in the log-parameters, on a likelihood whose ridge is flat - 1e-5 relative is what it holds
    assert cases.rel(np.exp(r.x), est[2:]) < 1e-5
    assert nll(np.log(est[2:])) <= r.fun + 1e-9 * abs(r.fun)


def test_statuses():
    cap = 4096
    sc = cases.status_cases(cap)
    zero, binom, empty = sc["zero"], sc["binomial"], sc["empty"]
    good = np.zeros((3, cap), np.uint64)
    good[:, :1024] = cases.shape_hist("cells")[:3]
    for hist, status in ((zero, bbfit.NO_FINITE_MAXIMUM), (binom, bbfit.NO_FINITE_MAXIMUM), (empty, bbfit.NO_DATA)):
        est, infos = bbfit.solve(np.concatenate([hist, good]))
        assert infos[0]["status"] == status and infos[1]["status"] == bbfit.CONVERGED, infos
        with pytest.raises(bbfit.FitFailed, match="cell counts"):
            bbfit.require_converged(infos)
    est, infos = bbfit.solve(np.concatenate([good, empty]))
    assert np.isnan(est[2]) and np.isnan(est[3])
    with pytest.raises(bbfit.FitFailed, match="base counts.*no row was kept"):
        bbfit.require_converged(infos)
    est, infos = bbfit.solve(np.concatenate([good, good]), max_iter=1)
    assert [i["status"] for i in infos] == [bbfit.ITERATION_CAP] * 2 and [i["iterations"] for i in infos] == [1, 1]
    with pytest.raises(bbfit.FitFailed, match="iteration cap"):
        bbfit.require_converged(infos)


def test_estimates_text_round_trips_through_the_rules_reader():
    import pandas as pd
    est = [0.21356677091082193, 104.95163748636298, 0.2474528917555431, 162.03696139428595]
    text = bbfit.estimates_text(est)
    assert text.split("\n")[0] == "alpha1\tbeta1\talpha2\tbeta2" and text.count("\n") == 2
    d = pd.read_csv(io.StringIO(text), sep="\t").squeeze().to_dict()                # get_BetaBinEstimates of rules/PoN.smk
    # (pandas' default float parser is not the round-trip one: it reads within an ulp or two, for the reference's file as for this one)
    assert cases.rel([d[k] for k in ("alpha1", "beta1", "alpha2", "beta2")], est) < 5e-16
    assert [float(x) for x in text.split("\n")[1].split("\t")] == est
    # ... and it is the file pandas writes (BetaBinEstimation.py:214-217)
    buf = io.StringIO()
    pd.DataFrame([est], columns=["alpha1", "beta1", "alpha2", "beta2"]).to_csv(buf, index=False, sep="\t")
    assert buf.getvalue() == text


def test_the_shim_accepts_the_reference_command_line():
    from tests.test_rules_cpu import parser_of
    p = parser_of(cli.betabin_estimation)
    a = p.parse_args(["--in_tsv", "files.txt", "--outfile", "BetaBinEstimates.txt"])
    assert (a.n_sites, a.seed, a.device) == (500000, 1992, 0)                       # BetaBinEstimation.py:158-159
    a = p.parse_args(["--in_tsv", "files.txt", "--outfile", "out.txt", "--n_sites", "0", "--seed", "7", "--device", "1"])
    assert (a.n_sites, a.seed, a.device) == (0, 7, 1)
    shim = os.path.join(os.path.dirname(GOLD), "..", "..", "workflow", "scripts_gpu", "PoN", "BetaBinEstimation.py")
    assert "cli.betabin_estimation()" in open(shim).read()
    q = parser_of(cli.pon_chain)
    a = q.parse_args(["--normals", "n.tsv", "--ref", "r.fa", "--outdir", "o", "--fit"])
    assert a.fit and a.alpha1 is None and (a.fit_n_sites, a.fit_seed) == (0, 1992)
