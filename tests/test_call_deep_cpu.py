"""CPU: the inputs of test_call_deep_gpu.py.  The fixture tests/golden/call_deep/tails.json (tools/make_call_deep_goldens.py) holds,
per parameter set and tail, pairs (k, n) with the exact beta-binomial upper tail, its 4-decimal rounding as an integer, the class the
call stage puts the pair in and the distance to a rounding tie.  Checked here: the pairs cover every class, no value is nearer than
1e-6 to a tie (the device and scipy both carry about 4e-10 at n = 150 000), scipy - the reference's own arithmetic - rounds every pair
to the fixture's integer, and the host mirror of the call stage's task counting gives the counts the GPU test expects."""
import collections

import pytest

from tests.support import call_deep_cases as cases

COMBOS = [(p, t) for p in cases.PARAM_SETS for t in cases.TAILS]


def test_classification_mirror():
    assert cases.classify(64, 2047) == "table/thread/lower" and cases.classify(65, 2047) == "table/lanes8/lower"
    assert cases.classify(1024, 2047) == "table/lanes8/lower" and cases.classify(1025, 2047) == "table/lanes8/upper"
    assert cases.classify(64, 2048) == "task/thread/lower" and cases.classify(65, 2048) == "task/lanes8/lower"
    assert cases.classify(1985, 2048) == "task/thread/upper" and cases.classify(1984, 2048) == "task/lanes8/upper"
    assert cases.classify(2048, 2048) == "task/thread/upper" and cases.tail_terms(2048, 2048) == 1
    assert cases.classify(1024, 30000) == "task/lanes8/lower" and cases.classify(1025, 30000) == "task/wave/lower"
    assert cases.classify(3977, 5000) == "task/lanes8/upper" and cases.classify(3976, 5000) == "task/wave/upper"
    assert cases.classify(1025, 2050) == "task/wave/lower" and cases.classify(1026, 2050) == "task/wave/upper"
    assert cases.classify(2500, 5000) == "task/wave/lower" and cases.classify(2501, 5000) == "task/wave/upper"
    assert cases.tail_work(0, 10) == 0 and cases.tail_work(11, 10) == 0 and not cases.tail_in_table(11, 10)


@pytest.mark.parametrize("pset,tail", COMBOS)
def test_fixture_covers_every_class_and_threshold(pset, tail):
    rows = cases.load()[pset][tail]
    have = {(e["k"], e["n"]) for e in rows}
    assert have >= set(cases.pairs_for(pset, tail)), "a listed pair (or its replacement) is missing"
    for (ps, t, old), new in cases.REPLACED.items():
        assert cases.classify(*old) == cases.classify(*new)
    assert len(cases.REPLACED) * 20 <= len(COMBOS) * len(cases.PAIRS)
    per_class = collections.Counter(e["class"] for e in rows)
    for cls in cases.CLASSES:
        assert per_class[cls] >= 2, (cls, per_class[cls])
    for e in rows:
        assert e["class"] == cases.classify(e["k"], e["n"]) and 1 <= e["k"] <= e["n"] <= 150000
    thr = {e["threshold"]: e for e in rows if e["threshold"] is not None}
    assert sorted(thr) == sorted(cases.THRESHOLD_VALUES)
    for v, e in thr.items():
        assert e["r4"] == v and cases.THRESHOLD_N[0] <= e["n"] <= cases.THRESHOLD_N[1]
    if pset == "wide":                                      # the set exists for upper-side sums with a value
        assert all(1 <= e["r4"] <= 9999 for e in rows if e["class"].endswith("upper") and e["n"] >= 2048 and e["k"] < e["n"] - 5), \
            [e for e in rows if e["class"].endswith("upper") and not 1 <= e["r4"] <= 9999]


@pytest.mark.parametrize("pset,tail", COMBOS)
def test_tie_margin_recomputed(pset, tail):
    """every pair up to 5000 terms from pmf(0), and the three deepest of n = 150 000 in one pass"""
    a, b = cases.ab(pset, tail)
    rows = cases.load()[pset][tail]
    assert all(e["tie"] >= cases.TIE_MARGIN for e in rows)
    by_n = collections.defaultdict(list)
    for e in rows:
        if e["k"] <= 5000 or (e["n"] == 150000 and pset == "wide" and tail == "reads") or (e["n"] == 150000 and pset == "defaults" and tail == "cells"):
            by_n[e["n"]].append(e)
    assert sum(len(v) for v in by_n.values()) >= len(rows) - 8
    for n, es in by_n.items():
        ex = cases.exact_tails(n, [e["k"] for e in es], a, b)
        for e in es:
            r4, tie = cases.rounded_and_tie(ex[e["k"]])
            assert r4 == e["r4"] and tie >= cases.TIE_MARGIN and abs(tie - e["tie"]) <= 1e-12, (e, r4, tie)
            assert abs(float(ex[e["k"]]) - e["exact"]) <= 1e-15


@pytest.mark.parametrize("pset,tail", COMBOS)
def test_scipy_rounds_to_the_fixture(pset, tail):
    """the oracle's own expression (oracle/calling_oracle.py: round(betabinom.sf(k - 0.1, n, a, b), 4)) on every pair"""
    from scipy.stats import betabinom
    a, b = cases.ab(pset, tail)
    for e in cases.load()[pset][tail]:
        p = round(betabinom.sf(e["k"] - 0.1, e["n"], a, b), 4)
        assert int(round(p * 1e4)) == e["r4"], (e, p)


def test_the_peaked_pair_needs_the_reanchor():
    """the geometry tests/support/call_deep_cases.py states for (75002, 150000) under the set 'peaked', from group_tail<64>'s own
    chunking, and the pair's fixture entry"""
    from scipy.stats import betabinom
    a, b = cases.ab("peaked", "reads")
    k, n = cases.PEAKED_PAIRS[0]
    assert cases.classify(k, n) == "task/wave/upper"
    terms = cases.tail_terms(k, n)
    chunk = (terms + 63) // 64
    start = k + 63 * chunk                                              # the last lane's first term
    assert chunk > 1024 and start + 1024 <= n
    assert betabinom.logpmf(start, n, a, b) < -745.2                    # exp() of it is 0.0
    assert betabinom.logpmf(start + 1024, n, a, b) > -700               # the re-anchor is a normal double
    assert betabinom.cdf(start + 1023, n, a, b) < 1e-12                 # what lies before it does not count
    for tail in cases.TAILS:
        rows = {(e["k"], e["n"]): e for e in cases.load()["peaked"][tail]}
        assert set(rows) == set(cases.PEAKED_PAIRS) and all(e["tie"] >= cases.TIE_MARGIN for e in rows.values())
        assert rows[(k, n)]["r4"] == 10000 == int(round(round(betabinom.sf(k - 0.1, n, a, b), 4) * 1e4))
    r4, tie = cases.rounded_and_tie(cases.exact_tails(n, [k], a, b)[k])
    assert (r4, tie >= cases.TIE_MARGIN) == (10000, True)


def test_site_tasks_mirror():
    """light / heavy task counts of single sites, counted by hand from call.hip's counting pass"""
    A, C_, T, I = 0, 1, 2, 4
    row = cases.cand_row(A, [(C_, (64, 2048), (1, 5))])
    assert (int(row[0]), int(row[1]), int(row[10 + A]), int(row[10 + C_])) == (2048, 5, 1984, 64)
    assert cases.site_tasks([row], A) == (1, 0)                      # (64, 2048) one thread; (1, 5) from the table; no noise tail
    assert cases.site_tasks([cases.cand_row(A, [(C_, (65, 2048), (1, 5))])], A) == (0, 1)
    assert cases.site_tasks([cases.cand_row(A, [(C_, (1, 10), (1025, 30000))])], A) == (0, 1)
    assert cases.site_tasks([cases.cand_row(A, [(C_, (3, 100), (1, 5))])], A) == (0, 0)
    assert cases.site_tasks([cases.make_row(3000, 5, {A: 2990, I: 10}, {A: 4, I: 1})], A) == (1, 0)      # only the noise tail (10, 3000)
    assert cases.site_tasks([cases.make_row(3000, 4, {A: 2990, I: 10}, {A: 4, I: 1})], A) == (0, 0)      # NC below min_cells: not considered
    # three alts in each of two cell types, every pair off the table, + both noise tails: 14 tasks
    r = cases.make_row(3000, 2500, {A: 2700, C_: 60, T: 70, 3: 80, I: 90}, {A: 2000, C_: 10, T: 20, 3: 30, I: 40})
    assert cases.site_tasks([r, r], A) == (8, 6)
    assert cases.site_tasks([r, None], A) == (5, 3)
    # the reference base's own column is no alt
    assert cases.site_tasks([r], C_) == (2, 4)


def test_levels_for_the_chain_tests():
    """test_call_deep_gpu draws significant (<= 10), low (11..499) and non-significant (>= 500) tails off the table from the fixture"""
    for pset, tail in COMBOS:
        deep = [e["r4"] for e in cases.load()[pset][tail] if e["class"].startswith("task")]
        assert any(v <= 10 for v in deep) and any(10 < v < 500 for v in deep) and any(v >= 500 for v in deep)
