"""GPU: the count kernels at the edges of their packed counters.  The directed piles of tests/support/pile_cases.py (proved on the CPU
by tests/test_count_edges_cpu.py) put exactly 256 / 257 entries into a tile or a window (narrow 16-bit rows up to 256: 256 x 255 =
65 280) and exactly 4095 / 4096 entries of quality 255 into one barcode's run (pileup.hip tm_add: quality sum 20 bits, 4095 x 255 =
1 044 225 of 1 048 575; forward count 12 bits, 4095 of 4095; tw_add: the duplicates of symbol class 7, 4094 of 4095; one entry more and
the job is k_tm_walk_wide's), and a sweep draws qualities from the whole byte.  Every case is counted in every form - a plain load and
k_tm_walk, the fused gather-count and a re-count of its store, the direct count (path 4), tile-phased events (path 5), windows (path 6)
and the wrong-claim restart - and every row must equal the events-level oracle's integer for integer; the step-1 call reads the saturated
rows back (call.hip's narrow-row read, the deep sites' tails at n = 4095 / 4096) and must print what oracle/calling_oracle.py prints,
and the beta-binomial fit's pass (bbfit.hip, the other reader of narrow rows) must bin what its numpy twin bins.
Under LSG_TIMING every plan says how many jobs went to the wide walk and how long the longest packed job is (store.hip plan_finish):
the 4095 cases sit ON the border - no wide job, a packed job of 4095 entries - in every form."""
import re

import numpy as np
import pytest

from longsom_amd._lib import CountParams
from tests.support import pile_cases as pc
from tests.test_count_gpu import run_both
from tests.test_fused_gpu import expected_direct_path, fused_vs_oracle, oracle_rows
from tests.test_fuzz_gpu import step1_vs_oracle

pytestmark = pytest.mark.gpu

PLAN = re.compile(r"\[lsg\] plan: (\d+) jobs, (\d+) multi-job tiles, (\d+) wide, longest packed job (\d+) entries")
# a one-barcode pile must still make rows and be called: no gate on cells
CALL = dict(min_ac_cells=1, min_ac_reads=3, min_cells=1, min_cell_types=1, alpha1=0.21356677091082193, beta2=162.03696139428595)


def params(min_bq):
    return CountParams.longsom_defaults(min_bq=min_bq, min_dp=1, min_cc=1)


def plans(capfd):
    return [tuple(int(x) for x in m.groups()) for m in PLAN.finditer(capfd.readouterr().err)]


def check_plans(case, got, at_least):
    """every plan the form made: (jobs, multi-job tiles, wide, longest packed job)"""
    assert len(got) >= at_least, got
    if case.plan is None:
        return
    wide, longest = case.plan
    for jobs, multi, w, n in got:
        assert w in wide, (case.name, got)
        assert n == longest if case.kind == "limit" else 0 < n <= longest, (case.name, got)


def bbfit_vs_twin(engine, n_ct, cap=8192):
    """the beta-binomial fit's pass over the resident rows (bbfit.hip reads narrow and wide units) against its numpy twin over the fetched ones"""
    from longsom_amd import bbfit
    want = np.zeros((6, cap), np.uint64)
    engine.bbfit_reset(cap)
    for ct in range(n_ct):
        _, refs, counts = engine.fetch_counts(ct)
        h, seen, kept = bbfit.histograms(refs, counts, cap, ct, 0, 1992)
        want += h
        assert engine.bbfit_accumulate(ct, table=ct) == (seen, kept)
    assert np.array_equal(engine.bbfit_fetch(), want)


def all_forms(engine, case, n_ct, p, capfd, call=True):
    ct_of = case.celltype_of(n_ct)
    capfd.readouterr()
    rows, cols = run_both(engine, case.rec, case.lens, case.refs, ct_of, n_ct, p)            # a plain load and k_tm_walk
    assert rows[0] > 0
    check_plans(case, plans(capfd), 1)
    if call:
        step1_vs_oracle(engine, case.lens, case.refs, n_ct, CALL)
        bbfit_vs_twin(engine, n_ct)
    capfd.readouterr()
    # the fused gather-count + a re-count of its store, the direct count, tile-phased events, windows, the wrong-claim restart: 8 loads
    assert fused_vs_oracle(engine, case.rec, case.lens, case.refs, ct_of, n_ct, p, expect_fused=n_ct <= 2) == (rows, cols)
    check_plans(case, plans(capfd), 8)
    if call:
        step1_vs_oracle(engine, case.lens, case.refs, n_ct, CALL)                            # ... over the rows of a load that kept no store
        bbfit_vs_twin(engine, n_ct)


def nothing_passes(engine, case, n_ct=2):
    """min_bq = 256: no quality reaches it - zero rows, and the load that keeps no store takes path 4"""
    p = params(256)
    ct_of = case.celltype_of(n_ct)
    assert run_both(engine, case.rec, case.lens, case.refs, ct_of, n_ct, p) == ([0] * n_ct, 0)
    assert expected_direct_path(engine, p, True, True, True) == 4
    saved = engine.load_settings()
    engine.set_count_at_load(p)
    engine.set_store_policy(engine.STORE_SKIP_WHEN_COUNTED)
    try:
        engine.load_reads(case.rec)
    finally:
        engine.restore_load_settings(saved)
    assert engine.layout_info()[0] == 4
    assert engine.pileup_count(p) == ([0] * n_ct, 0)
    want, want_cols = oracle_rows(case.rec, case.lens, case.refs, ct_of, n_ct, p)
    assert want_cols == 0 and all(len(w[0]) == 0 for w in want)
    for ct in range(n_ct):
        assert len(engine.fetch_counts(ct)[0]) == 0


ROWS, LIMIT, PAST = pc.row_cases(), pc.limit_cases(pc.JOB_LIMIT), pc.limit_cases(pc.JOB_LIMIT + 1)
name = lambda c: c.name


@pytest.mark.parametrize("case", ROWS, ids=name)
def test_rows_at_the_narrow_threshold(engine, case, monkeypatch, capfd):
    """256 entries: 16-bit rows whose quality sums reach 65 280 beside a full neighbouring half-word; 257: 32-bit rows"""
    monkeypatch.setenv("LSG_TIMING", "1")
    for min_bq in (255, 20):
        all_forms(engine, case, 2, params(min_bq), capfd)
    nothing_passes(engine, case)


@pytest.mark.parametrize("case", LIMIT, ids=name)
def test_packed_job_at_its_limit(engine, case, monkeypatch, capfd):
    """4095 entries of quality 255 in one job: every field of the packed counters at its last value, no job for the wide walk"""
    monkeypatch.setenv("LSG_TIMING", "1")
    for min_bq in (255, 20):
        all_forms(engine, case, 2, params(min_bq), capfd)
    all_forms(engine, case, 3, params(255), capfd, call=False)                               # three cell types: two passes, no fused path
    nothing_passes(engine, case)


@pytest.mark.parametrize("case", PAST, ids=name)
def test_one_entry_past_the_limit(engine, case, monkeypatch, capfd):
    """4096 entries: the job is the wide walk's, and no packed job is longer than 4095"""
    monkeypatch.setenv("LSG_TIMING", "1")
    for min_bq in (255, 20):
        all_forms(engine, case, 2, params(min_bq), capfd)
    all_forms(engine, case, 3, params(255), capfd, call=False)
    nothing_passes(engine, case)


@pytest.fixture(scope="module")
def sweep():
    return pc.sweep_case()


@pytest.mark.parametrize("min_bq", [0, 1, 93, 128, 200, 255])
def test_quality_sweep(engine, sweep, min_bq):
    """qualities uniform in 0..255 against thresholds on both sides of 128 (the compares of a quality byte must be unsigned)"""
    rec, lens, refs, ct_of = sweep
    p = params(min_bq)
    rows, cols = run_both(engine, rec, lens, refs, ct_of, 2, p)
    assert sum(rows) > 0
    assert fused_vs_oracle(engine, rec, lens, refs, ct_of, 2, p) == (rows, cols)
