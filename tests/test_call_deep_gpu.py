"""GPU: the step-1 call (csrc/call.hip) at sites deeper than the tail table - the light and heavy tail tasks, group_tail on eight and on
64 lanes, the deferred sites' chains in k_call_finish, the wave-private task arenas and their refills, the second, larger-sized run and
the PASS list.  Values are compared with the exact integers of tests/golden/call_deep/tails.json (pairs at least 1e-6 from a rounding
tie: no tolerance), records with oracle/calling_oracle.step1 under the same parameters.  Count rows are installed; no pileup runs."""
import re

import numpy as np
import pytest

from longsom_amd import tsvio
from longsom_amd._lib import CallParams
from tests.support import call_deep_cases as cases
from tests.util import neg_zero

pytestmark = pytest.mark.gpu
A, C_, T, G, I, D = 0, 1, 2, 3, 4, 5
LETTER_SYM = {ord("A"): A, ord("C"): C_, ord("T"): T, ord("G"): G}
CALL_LINE = re.compile(r"\[lsg\] call: (\d+) sites in (\d+) tiles, light task slots (\d+) \(\+(\d+) of the first chunks\), heavy (\d+) \(\+(\d+)\), "
                       r"sites that waited for a tail (\d+), PASS (\d+)")


def call_params(pset, **kw):
    return CallParams.longsom_defaults(**dict(cases.ALL_SETS[pset], **kw))


def call_lines(capfd):
    """the library's '[lsg] call:' lines since the last look, as dicts"""
    names = ("sites", "tiles", "light", "light_first", "heavy", "heavy_first", "waited", "n_pass")
    return [dict(zip(names, map(int, m.groups()))) for m in CALL_LINE.finditer(capfd.readouterr().err)]


def install(engine, seqs, per_ct):
    engine.set_contigs([len(s) for s in seqs])
    for t, s in enumerate(seqs):
        engine.load_reference(t, s)
    engine.load_counts([p[0] for p in per_ct], [p[2] for p in per_ct])


# ---- a. every tail path, value by value -------------------------------------------------------------------------------------------
def single_tail_sites(pset):
    """[(row, {field: expected integer})]: one site per fixture pair and destination of a task - a candidate's p_bc, its p_cc, the
    site's noise_p_bc and noise_p_cc.  Reference base A, alt C; the tail that is not under test asks the table for (1, 10) / (1, 5)."""
    er, ec = cases.expected(pset, "reads"), cases.expected(pset, "cells")
    small_r = (1, 10)
    small_c = (1, 5)
    out = []
    for (k, n), v in er.items():
        out.append((cases.cand_row(A, [(C_, (k, n), small_c)]), {"p_bc": v, "p_cc": ec[small_c], "noise_p_bc": -1, "noise_p_cc": -1}, "reads", k, n))
        out.append((cases.make_row(n, 5, {A: n - k, I: k}, {A: 4, I: 1}), {"noise_p_bc": v, "noise_p_cc": ec[small_c]}, "noise reads", k, n))
    for (k, n), v in ec.items():
        out.append((cases.cand_row(A, [(C_, small_r, (k, n))]), {"p_bc": er[small_r], "p_cc": v, "noise_p_bc": -1, "noise_p_cc": -1}, "cells", k, n))
        out.append((cases.make_row(10, n, {A: 9, D: 1}, {A: n - k, D: k}), {"noise_p_bc": er[small_r], "noise_p_cc": v}, "noise cells", k, n))
    return out


@pytest.mark.parametrize("layout", ["one site per tile", "64 sites per tile"])
@pytest.mark.parametrize("pset", list(cases.ALL_SETS))
def test_every_tail_path_gives_the_exact_integer(engine, pset, layout):
    """3a: p_bc, p_cc, noise_p_bc and noise_p_cc of single-cell-type sites, each written by a task (or read from the table, for the
    pairs at n = 2047) of every class, equal round(exact, 4) * 1e4.  The set 'peaked' has the one pair at which a lane of
    group_tail<64> depends on its re-anchor (tests/support/call_deep_cases.py)."""
    sites = single_tail_sites(pset)
    pos = np.arange(len(sites), dtype=np.int64) * (64 if layout.startswith("one") else 1) + 10
    L = int(pos[-1]) + 64
    install(engine, [np.full(L, ord("A"), np.uint8)], [(pos, None, np.stack([s[0] for s in sites]))])
    n_sites, _ = engine.call_step1(call_params(pset))
    calls = engine.fetch_calls()
    assert n_sites == len(calls) == len(sites) and np.array_equal(calls["key"], pos)
    bad = []
    for c, (_, want, what, k, n) in zip(calls, sites):
        got = {"p_bc": int(c["p_bc"][0][0]), "p_cc": int(c["p_cc"][0][0]), "noise_p_bc": int(c["noise_p_bc"]), "noise_p_cc": int(c["noise_p_cc"])}
        for f, v in want.items():
            if got[f] != v:
                bad.append((what, f, (k, n), cases.classify(k, n), "got", got[f], "exact", v))
    assert not bad, "%d of %d values differ: %s" % (len(bad), 4 * len(sites), bad[:12])


@pytest.mark.parametrize("pset", list(cases.ALL_SETS))
def test_one_thread_tail_gives_the_same_integers(engine, pset):
    """3a: the same pairs through lsg_betabinom_sf4 (bb_upper_tail on one thread, re-anchored every 1024 terms).  The raw values'
    largest distance from the exact sum is printed, not asserted (DESIGN.md's call section keeps the figure)."""
    for tail in cases.TAILS:
        a, b = cases.ab(pset, tail)
        rows = cases.load()[pset][tail]
        k, n = [e["k"] for e in rows], [e["n"] for e in rows]
        got = engine.betabinom_sf4(k, n, a, b)
        r4, raw = engine.betabinom_sf(k, n, a, b)
        want = np.array([e["r4"] for e in rows])
        err = np.abs(raw - np.array([e["exact"] for e in rows]))
        j = int(err.argmax())
        print("call_deep %s/%s: largest |raw - exact| = %.3g at (k, n) = (%d, %d)" % (pset, tail, err[j], k[j], n[j]))
        assert np.array_equal(got, want) and np.array_equal(r4, want), [(k[i], n[i], int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0]]


# ---- b. deferred chains against the oracle ----------------------------------------------------------------------------------------
class Levels:
    """pairs of one parameter set by what the chains make of them: significant (<= 10), low (11..499), non-significant (>= 500);
    off the table ('deep') or in it ('tab'); the threshold pairs by their value"""
    def __init__(self, pset):
        self.pairs, self.thr = {}, {}
        for tail in cases.TAILS:
            for e in cases.load()[pset][tail]:
                lvl = "sig" if e["r4"] <= 10 else ("low" if e["r4"] < 500 else "non")
                self.pairs.setdefault((tail, "deep" if e["class"].startswith("task") else "tab", lvl), []).append((e["k"], e["n"]))
                if e["threshold"] is not None:
                    self.thr[(tail, e["threshold"])] = (e["k"], e["n"])
        # of the pairs that round to 0.0009 and 0.001 the one with more alt reads / cells is 'enough', the other 'too few': the
        # calls below set min_ac_reads / min_ac_cells between them
        self.enough = {t: max(self.thr[(t, 9)], self.thr[(t, 10)]) for t in cases.TAILS}
        self.few = {t: min(self.thr[(t, 9)], self.thr[(t, 10)]) for t in cases.TAILS}
        self.min_ac_reads, self.min_ac_cells = self.enough["reads"][0], self.enough["cells"][0]

    def draw(self, rng, tail, depth, lvl=None):
        opts = [v for (t, d, l), v in self.pairs.items() if t == tail and d == depth and (lvl is None or l == lvl)]
        flat = [p for v in opts for p in v]
        return flat[rng.integers(len(flat))]


def add_alt(row, ref, sym, kb, kc):
    """a further alt of kb reads in kc cells, taken off the reference allele's counts"""
    kb, kc = min(kb, int(row[10 + ref])), min(kc, int(row[2 + ref]))
    if kb > 0 and kc > 0:
        row[10 + sym] += kb; row[26 + sym] += kb; row[10 + ref] -= kb; row[26 + ref] -= kb
        row[2 + sym] += kc; row[2 + ref] -= kc
    return row


def add_noise(row, ref, sym, kb, kc):
    """kb inserted / deleted reads in kc cells, taken off the reference allele's counts (they stay in DP and NC)"""
    return add_alt(row, ref, sym, kb, kc)


def random_ct_row(rng, lv, ref, alt):
    shape = rng.choice(["tab"] * 5 + ["dp deep", "nc deep", "both deep", "shallow"])
    if shape == "shallow":                                                  # below min_cov / min_cells: not considered
        return cases.make_row(4, 3, {ref: 3, alt: 1}, {ref: 2, alt: 1})
    rd, cd = ("deep" if shape in ("dp deep", "both deep") else "tab"), ("deep" if shape in ("nc deep", "both deep") else "tab")
    row = cases.cand_row(ref, [(alt, lv.draw(rng, "reads", rd), lv.draw(rng, "cells", cd))])
    others = [s for s in (A, C_, T, G) if s not in (ref, alt)]
    if rng.random() < 0.25:
        add_alt(row, ref, others[0], int(rng.integers(1, 4)), 1)
    if rng.random() < 0.1:
        add_alt(row, ref, others[1], int(rng.integers(1, 4)), 1)
    if rng.random() < 0.3:
        add_noise(row, ref, I if rng.random() < 0.5 else D, int(rng.integers(1, 400)), int(rng.integers(1, 6)))
    return row


def random_site(rng, lv, ref, n_ct):
    """rows of one site (None: the cell type has no row); at least one row"""
    alts = [s for s in (A, C_, T, G) if s != ref]
    alt = alts[rng.integers(3)]
    kind = rng.random()
    rows = []
    for ct in range(n_ct):
        if rng.random() < 0.25:
            rows.append(None)
        elif kind < 0.12:                                                   # no candidate: reference reads and some noise, deep or not
            n = lv.draw(rng, "reads", "deep" if rng.random() < 0.5 else "tab")[1]
            rows.append(add_noise(cases.make_row(n, 40, {ref: n}, {ref: 40}), ref, I, int(rng.integers(0, 90)), int(rng.integers(1, 6))))
        else:
            rows.append(random_ct_row(rng, lv, ref, alt if rng.random() < 0.85 else alts[rng.integers(3)]))
    if all(r is None for r in rows):
        rows[rng.integers(n_ct)] = random_ct_row(rng, lv, ref, alt)
    return rows


def designed_sites(lv, ref):
    """sites whose chains run in k_call_finish (every one has a tail off the table), one per outcome of the chains; the names say
    what the oracle is expected to print - the test asserts their presence in the oracle's text, not here"""
    alt, alt2 = [s for s in (A, C_, T, G) if s != ref][:2]
    R, Cc = lv.enough["reads"], lv.enough["cells"]
    one = lambda rp, cp: cases.cand_row(ref, [(alt, rp, cp)])
    tab_c = max(lv.pairs[("cells", "tab", "sig")])                          # a table pair, significant
    tab_r = max(lv.pairs[("reads", "tab", "sig")])
    out = {
        "PASS": [one(R, Cc), None],
        "Low_reads": [one(lv.few["reads"], Cc), None],
        "Low_cells": [one(R, lv.few["cells"]), None],
        "Multi-allelic (cell type)": [add_alt(one(R, Cc), ref, alt2, 1, 1), None],
        "Low-Significance (0.0011 reads)": [one(lv.thr[("reads", 11)], Cc), None],
        "Low-Significance (0.0499 cells)": [None, one(R, lv.thr[("cells", 499)])],
        "Low-Significance (0.0011 cells)": [one(R, lv.thr[("cells", 11)]), None],
        "Low-Significance (0.0499 reads)": [one(lv.thr[("reads", 499)], Cc), None],
        "Non-Significant (0.05 reads)": [one(lv.thr[("reads", 500)], Cc), None],
        "Non-Significant (0.05 cells)": [None, one(R, lv.thr[("cells", 500)])],
        "0.001 in both tails": [one(lv.thr[("reads", 10)], lv.thr[("cells", 10)]), None],
        "DP deep, NC in the table": [one(lv.thr[("reads", 10)], tab_c), None],
        "NC deep, DP in the table": [one(tab_r, lv.thr[("cells", 10)]), None],
        "Multiple_cell_types": [one(R, Cc), one(R, Cc)],
        "Multi-allelic (site, alts differ)": [one(R, Cc), cases.cand_row(ref, [(alt2, R, Cc)])],
        "Cell_type_noise": [one(R, Cc), one(lv.thr[("reads", 11)], Cc)],
        "Noisy_site with a candidate": [add_noise(one(R, Cc), ref, I, R[1] - R[0], 1), None],
        "Noisy_site with a candidate (cells)": [one(R, Cc), add_noise(cases.make_row(10, lv.thr[("cells", 9)][1], {ref: 10}, {ref: lv.thr[("cells", 9)][1]}),
                                                                      ref, D, 1, lv.thr[("cells", 9)][0])],
    }
    for v in (9, 10, 11):                                                    # only the noise tail is deep: < 0.001 flags the site, 0.001 does not
        k, n = lv.thr[("reads", v)]
        out["noise only, reads round to %d" % v] = [None, add_noise(cases.make_row(n, 5, {ref: n}, {ref: 5}), ref, I, k, 1)]
        k, n = lv.thr[("cells", v)]
        out["noise only, cells round to %d" % v] = [add_noise(cases.make_row(10, n, {ref: 10}, {ref: n}), ref, D, 1, k), None]
    return out


def random_reference(rng, lens):
    seqs = []
    for L in lens:
        s, cur = [], rng.integers(0, 4)
        for _ in range(L):
            if rng.random() > 0.62:
                cur = rng.integers(0, 4)
            s.append("ACGT"[cur])
        seqs.append(np.frombuffer("".join(s).encode(), np.uint8).copy())
    return seqs


def per_ct_arrays(sites, n_ct):
    """sites: [(key, ref letter, rows)] -> per cell type (keys, refs, counts), ascending keys"""
    per_ct = []
    for ct in range(n_ct):
        sel = sorted((k, r, rows[ct]) for k, r, rows in sites if rows[ct] is not None)
        per_ct.append((np.asarray([s[0] for s in sel], np.int64), np.asarray([s[1] for s in sel], np.uint8),
                       np.stack([s[2] for s in sel]) if sel else np.zeros((0, cases.ROW_WORDS), np.uint32)))
    return per_ct


def oracle_lines(per_ct, names, ct_names, seqs, pset, **kw):
    from oracle import calling_oracle
    merged = tsvio.format_merged_tsv(per_ct, names, ct_names)
    header = [l + "\n" for l in merged.split("\n") if l.startswith("##")]
    want = neg_zero(calling_oracle.step1(merged, dict(zip(names, [s.tobytes().decode() for s in seqs])), info_lines=tsvio.STEP1_INFO_LINES,
                                         **dict(cases.PARAM_SETS[pset], **kw)))
    return header, [l for l in want.split("\n") if l and not l.startswith("##fileDate=")]


def step1_lines(calls, per_ct, names, ct_names, header):
    return [l for l in tsvio.format_step1_tsv(calls, per_ct, names, ct_names, header).split("\n") if l and not l.startswith("##fileDate=")]


def chain_case(pset, n_ct):
    """a few hundred sites over eight contigs (some shorter than a tile): 24 designed ones among random ones"""
    rng = np.random.default_rng(1000 + n_ct)
    lv = Levels(pset)
    lens = [197, 70, 6, 64, 129, 11, 65, 63]
    names = ["c%d" % i for i in range(len(lens))]
    seqs = random_reference(rng, lens)
    free = [(t, p) for t, L in enumerate(lens) for p in range(L)]
    take = sorted(rng.choice(len(free), size=int(0.55 * len(free)), replace=False).tolist())
    design_at = sorted(rng.choice(take, size=24, replace=False).tolist())
    sites, designed = [], {}
    for i in take:
        t, p = free[i]
        ref = LETTER_SYM[int(seqs[t][p])]
        if i in design_at:
            name, rows = list(designed_sites(lv, ref).items())[design_at.index(i)]
            rows = list(rows) + [None] * (n_ct - 2)
            designed[(names[t], p + 1)] = name
        else:
            rows = random_site(rng, lv, ref, n_ct)
        sites.append(((t << 32) | p, int(seqs[t][p]), rows))
    assert len(designed) == len(designed_sites(lv, A)) == 24
    kw = dict(min_ac_cells=lv.min_ac_cells, min_ac_reads=lv.min_ac_reads, min_cell_types=1)
    return seqs, names, sites, designed, per_ct_arrays(sites, n_ct), kw


def check_deferred_rows(want, sites, names, designed):
    """the oracle's rows of the sites whose chains ran in k_call_finish show every outcome of the chains"""
    deferred = {}
    tid_of = {n: i for i, n in enumerate(names)}
    rows_of = {k: (LETTER_SYM[r], rows) for k, r, rows in sites}
    for l in want:
        if l.startswith("#"):
            continue
        el = l.split("\t")
        rsym, rows = rows_of[(tid_of[el[0]] << 32) | (int(el[1]) - 1)]
        if sum(cases.site_tasks(rows, rsym)) > 0:
            deferred[(el[0], int(el[1]))] = el
    assert set(designed) <= set(deferred) and 40 <= len(deferred) <= len(sites) - 40, (len(deferred), len(sites))
    ct_filters = {f for el in deferred.values() for f in el[23].split(",")}
    assert ct_filters >= {"Non-Significant", "Low-Significance", "Multi-allelic", "Low_cells", "Low_reads", "PASS"}, ct_filters
    site_filters = {f for el in deferred.values() if el[4] != "." for f in el[5].split(",")}
    assert site_filters >= {"Multiple_cell_types", "Multi-allelic", "Cell_type_noise", "Noisy_site"}, site_filters
    no_cand = [el[5] for el in deferred.values() if el[4] == "."]
    assert "Noisy_site" in no_cand and "." in no_cand
    p_tokens = {tok for el in deferred.values() for col in (16, 17) for tok in re.split("[,|]", el[col])}
    p_tokens |= {el[col].split(";")[2] for el in deferred.values() for col in (20, 21)}
    assert p_tokens >= {"0.0009", "0.001", "0.0011", "0.0499", "0.05"}, sorted(p_tokens)[:40]
    # each designed site shows what its name says (in the oracle's text, which the device's equals)
    for key, name in designed.items():
        el = deferred[key]
        label = name.split(" (")[0].split(",")[0]
        if label in ("PASS", "Low_reads", "Low_cells", "Low-Significance", "Non-Significant"):
            assert label in el[23].split(","), (name, el[5], el[23])
        elif label == "Multi-allelic":
            assert "Multi-allelic" in el[5].split(","), (name, el[5], el[23])
        elif label in ("Multiple_cell_types", "Cell_type_noise"):
            assert label in el[5].split(","), (name, el[5], el[23])
        elif label.startswith("Noisy_site"):
            assert "Noisy_site" in el[5].split(",") and el[4] != ".", (name, el[5], el[20], el[21])
        elif label.startswith("noise only"):
            assert el[4] == "." and el[5] == ("Noisy_site" if name.endswith(" 9") else "."), (name, el[5], el[20], el[21])
        elif label == "0.001 in both tails":
            assert el[16] == "0.001" and el[17] == "0.001" and el[23] not in ("Low-Significance", "Non-Significant"), (name, el[16], el[17], el[23])


@pytest.mark.parametrize("n_ct", [2, 3, 4])
@pytest.mark.parametrize("pset", list(cases.PARAM_SETS))
def test_deferred_chains_match_the_oracle(engine, pset, n_ct):
    """3b: the filter chains k_call_finish runs for sites with a tail off the table (the same chains k_call_gather runs for the
    others), beside table-only lanes in the same tiles, at contig and tile edges"""
    seqs, names, sites, designed, per_ct, kw = chain_case(pset, n_ct)
    ct_names = ["T%d" % i for i in range(n_ct)]
    install(engine, seqs, per_ct)
    n_sites, _ = engine.call_step1(call_params(pset, **kw))
    calls = engine.fetch_calls()
    assert n_sites == len(calls) == len(sites)
    header, want = oracle_lines(per_ct, names, ct_names, seqs, pset, min_reads=5, min_cells=5, max_cell_types=1, **kw)
    got = step1_lines(calls, per_ct, names, ct_names, header)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not bad, "%d lines differ, the first:\n%s\n%s" % (len(bad), bad[0][0], bad[0][1])
    check_deferred_rows(want, sites, names, designed)


# ---- c, d. the arenas and the re-sized run: copies of ~200 patterns on a period-4 reference ----------------------------------------
PSET_LIB = "defaults"
_LIB = {}


def fourteen_tasks(ref, heavy):
    """two cell types, three alts each, every tail off the table, both noise tails: 14 tasks, all light (<= 64 terms) or all heavy"""
    alts = [s for s in (A, C_, T, G) if s != ref]
    bc, cc, nz = ((70, 80, 90), (65, 66, 67), (100, 40)) if heavy else ((60, 50, 40), (10, 20, 30), (30, 12))
    row = cases.make_row(3000, 2500, dict(zip(alts, bc)), dict(zip(alts, cc)))
    row[10 + ref] = row[26 + ref] = 3000 - sum(bc) - nz[0]; row[2 + ref] = 2500 - sum(cc) - nz[1]
    row[10 + I] = row[26 + I] = nz[0]; row[2 + I] = nz[1]
    assert cases.site_tasks([row, row], ref) == ((0, 14) if heavy else (14, 0))
    return [row, row.copy()]


def pattern_library(engine, capfd, monkeypatch):
    """about 200 site patterns of two cell types, each tied to a residue of its position mod 4 (reference ACGT repeated: the same
    reference base and context at every copy); their records come from one call whose text is compared with the oracle in
    test_pattern_records_match_the_oracle.  Also the number of k_call_gather's waves, read from the library's own line."""
    if _LIB:
        return _LIB
    rng = np.random.default_rng(4242)
    lv = Levels(PSET_LIB)
    pats = []
    for i in range(200):
        res = i % 4
        ref = LETTER_SYM[ord("ACGT"[res])]
        if i < 4:
            rows = fourteen_tasks(ref, heavy=False)
        elif i < 8:
            rows = fourteen_tasks(ref, heavy=True)
        elif i < 12:
            rows = [fourteen_tasks(ref, heavy=False)[0], fourteen_tasks(ref, heavy=True)[1]]
        elif i < 36:
            rows = list(list(designed_sites(lv, ref).values())[i - 12])
        elif i < 120:                                                        # table only
            alt = [s for s in (A, C_, T, G) if s != ref][i % 3]
            rows = [cases.cand_row(ref, [(alt, lv.draw(rng, "reads", "tab"), lv.draw(rng, "cells", "tab"))]) if rng.random() < 0.8 else None for _ in range(2)]
            if rows[0] is None and rows[1] is None:
                rows[0] = cases.make_row(50, 20, {ref: 50}, {ref: 20})
        else:
            rows = random_site(rng, lv, ref, 2)
        pats.append(rows)
    L = 64 * (len(pats) + 2)
    seq = np.frombuffer(("ACGT" * (L // 4)).encode(), np.uint8).copy()
    sites = [((64 * (i + 1) + 8 + i % 4), int(seq[i % 4]), rows) for i, rows in enumerate(pats)]
    per_ct = per_ct_arrays(sites, 2)
    kw = dict(min_ac_cells=lv.min_ac_cells, min_ac_reads=lv.min_ac_reads, min_cell_types=1)
    install(engine, [seq], per_ct)
    monkeypatch.setenv("LSG_TIMING", "1")
    capfd.readouterr()
    engine.call_step1(call_params(PSET_LIB, **kw))
    lines = call_lines(capfd)
    monkeypatch.delenv("LSG_TIMING")
    calls = engine.fetch_calls().copy()
    tasks = np.array([cases.site_tasks(rows, LETTER_SYM[ord("ACGT"[i % 4])]) for i, rows in enumerate(pats)])
    _LIB.update(pats=pats, calls=calls, per_ct=per_ct, seq=seq, kw=kw, lines=lines, tasks=tasks, lv=lv,
                rows=[np.stack([p[ct] if p[ct] is not None else np.zeros(cases.ROW_WORDS, np.uint32) for p in pats]) for ct in range(2)],
                present=[np.array([p[ct] is not None for p in pats]) for ct in range(2)])
    return _LIB


RECORD_FIELDS = [f for f in ("ref", "present", "considered", "has_cand", "n_alt", "alt", "ct_filter", "alt_bc", "alt_cc", "p_bc", "p_cc", "site_filter",
                             "cell_types_min", "sum_alts_bc", "sum_dp", "sum_alts_cc", "sum_nc", "noise_p_bc", "noise_p_cc", "up_ctx", "down_ctx")]


def copies(lib, pid, pos):
    """per-cell-type (keys, None, rows) of the sites pos[i] = a copy of pattern pid[i]"""
    assert np.array_equal(pos % 4, pid % 4)
    return [(pos[lib["present"][ct][pid]], None, lib["rows"][ct][pid[lib["present"][ct][pid]]]) for ct in range(2)]


def assert_copies(lib, calls, pid, pos):
    assert len(calls) == len(pos) and np.array_equal(calls["key"], pos)
    want = lib["calls"][pid]
    for f in RECORD_FIELDS:
        same = (calls[f] == want[f]).reshape(len(pos), -1).all(axis=1)
        assert same.all(), "%s differs at %d of %d sites, the first a copy of pattern %d (%s light / heavy tasks): %s, the pattern's %s" % (
            f, (~same).sum(), len(pos), pid[np.argmin(same)], lib["tasks"][pid[np.argmin(same)]], calls[f][np.argmin(same)], want[f][np.argmin(same)])


def test_pattern_records_match_the_oracle(engine, capfd, monkeypatch):
    """3c / 3d compare copies of these records: here the records themselves, as text, against the oracle; and the library's line
    reports the patterns' deferred sites and the waves' first chunks"""
    lib = pattern_library(engine, capfd, monkeypatch)
    header, want = oracle_lines(lib["per_ct"], ["chr1"], ["T0", "T1"], [lib["seq"]], PSET_LIB, min_reads=5, min_cells=5, max_cell_types=1, **lib["kw"])
    got = step1_lines(lib["calls"], lib["per_ct"], ["chr1"], ["T0", "T1"], header)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not bad, "%d lines differ, the first:\n%s\n%s" % (len(bad), bad[0][0], bad[0][1])
    assert len(lib["lines"]) == 1, lib["lines"]
    line = lib["lines"][0]
    assert line["sites"] == len(lib["pats"]) and line["waited"] == int((lib["tasks"].sum(axis=1) > 0).sum())
    assert line["light_first"] % cases.TASK_CHUNK == 0 and line["light_first"] // cases.TASK_CHUNK == line["heavy_first"] // cases.HEAVY_CHUNK > 0
    tl, th = lib["tasks"][:, 0], lib["tasks"][:, 1]
    assert tl.max() == 14 and th.max() == 14 and (lib["tasks"].sum(axis=1) == 0).sum() >= 60


def test_arenas_and_refills(engine, capfd, monkeypatch):
    """3c: three times as many tiles as gather waves, 1 to 64 sites each with 0 to 14 light and 0 to 14 heavy tasks a site: a wave
    comes to a tile with a partly used chunk, and a tile's request spans several chunks"""
    lib = pattern_library(engine, capfd, monkeypatch)
    waves = lib["lines"][0]["light_first"] // cases.TASK_CHUNK
    rng = np.random.default_rng(77)
    n_tiles = 3 * waves + 17
    size = np.where(rng.random(n_tiles) < 0.75, rng.integers(1, 5, n_tiles), np.where(rng.random(n_tiles) < 0.7, rng.integers(5, 33, n_tiles), 64))
    first = (64 - size) * rng.integers(0, 2, n_tiles)                        # the tile's sites sit at its start or at its end
    tile = np.repeat(np.arange(n_tiles, dtype=np.int64), size)
    lane = np.arange(size.sum()) - np.repeat(np.cumsum(size) - size, size) + np.repeat(first, size)
    pos = 64 * (tile + 1) + lane
    # patterns 0..11 ask for 14 tasks, 12..35 are the designed sites, 36..119 ask the table only, 120.. are random; pattern i belongs
    # to positions of residue i % 4.  A tenth of the tiles is busy (14 tasks at every site), elsewhere most sites ask for few or none
    m, u, res = len(pos), rng.random(len(pos)), pos % 4
    busy = np.repeat(rng.random(n_tiles) < 0.1, size)
    other = rng.integers(0, 26, m)
    pid = np.where(busy | (u < 0.05), 4 * rng.integers(0, 3, m), np.where(u < 0.6, 36 + 4 * rng.integers(0, 21, m),
                   np.where(other < 6, 12 + 4 * other, 120 + 4 * (other - 6)))) + res
    assert len(lib["pats"]) == 200 and pid.max() < 200
    seq = np.frombuffer(("ACGT" * (16 * (n_tiles + 2))).encode(), np.uint8).copy()
    install(engine, [seq], copies(lib, pid, pos))
    monkeypatch.setenv("LSG_TIMING", "1")
    capfd.readouterr()
    n_sites, _ = engine.call_step1(call_params(PSET_LIB, **lib["kw"]))
    lines = call_lines(capfd)
    monkeypatch.delenv("LSG_TIMING")
    assert n_sites == len(pos)
    assert len(lines) == 1, "the call ran %d times: the shared engine's task buffers were sized up" % len(lines)
    line = lines[0]
    assert line["tiles"] == n_tiles >= 3 * waves
    tasks = lib["tasks"][pid]
    assert line["waited"] == int((tasks.sum(axis=1) > 0).sum())
    per_tile = np.add.reduceat(tasks, np.cumsum(size) - size, axis=0)
    assert per_tile[:, 0].max() > 3 * cases.TASK_CHUNK and per_tile[:, 1].max() > 3 * cases.HEAVY_CHUNK      # one request over several chunks
    assert line["light"] > 0 and line["heavy"] > 0 and line["light"] % cases.TASK_CHUNK == 0 and line["heavy"] % cases.HEAVY_CHUNK == 0
    assert line["light"] + line["light_first"] >= tasks[:, 0].sum() and line["heavy"] + line["heavy_first"] >= tasks[:, 1].sum()
    assert_copies(lib, engine.fetch_calls(), pid, pos)


def test_resized_run(capfd, monkeypatch, engine):
    """3d: more tasks than the first sizing holds (one task per site + 1024 + three chunks per wave), by a third: the call runs a
    second time with the bound no site exceeds, in an engine of its own (the shared one keeps its small buffers)"""
    from longsom_amd.engine import Engine
    lib = pattern_library(engine, capfd, monkeypatch)
    waves = lib["lines"][0]["light_first"] // cases.TASK_CHUNK
    first_sizing_slack = 1024 + 3 * cases.TASK_CHUNK * waves
    n = int(np.ceil(4 / 3 * first_sizing_slack / (14 - 4 / 3))) + 64         # 14 n = 4/3 (n + slack)
    pos = 64 + np.arange(n, dtype=np.int64)
    pid = pos % 4                                                            # patterns 0..3: 14 light tasks
    assert (lib["tasks"][pid] == (14, 0)).all() and 14 * n > 1.3 * (n + first_sizing_slack)
    seq = np.frombuffer(("ACGT" * (n // 4 + 64)).encode(), np.uint8).copy()
    monkeypatch.setenv("LSG_TIMING", "1")
    with Engine(0) as eng:
        install(eng, [seq], copies(lib, pid, pos))
        capfd.readouterr()
        assert eng.call_step1(call_params(PSET_LIB, **lib["kw"]))[0] == n
        lines = call_lines(capfd)
        assert len(lines) == 2 and lines[0]["waited"] == lines[1]["waited"] == n, lines
        assert lines[0]["light"] + lines[0]["light_first"] > n + first_sizing_slack
        assert_copies(lib, eng.fetch_calls(), pid, pos)
        assert eng.call_step1(call_params(PSET_LIB, **lib["kw"]))[0] == n
        assert len(call_lines(capfd)) == 1
        assert_copies(lib, eng.fetch_calls(), pid, pos)


# ---- e. the PASS list -------------------------------------------------------------------------------------------------------------
EXPORT_LINE = re.compile(r"\[lsg\] export: kind 2 from the (PASS list|scan), (\d+) rows")


@pytest.mark.parametrize("n_pass", [1, 1025, cases.PASS_CAP, cases.PASS_CAP + 1])
def test_pass_list(engine, capfd, monkeypatch, n_pass):
    """3e: PASS candidates listed by k_call_gather (table depth) and by k_call_finish (one deep tail), sorted by one workgroup: one
    element per thread, two, the list's capacity, and one more - answered by the scan"""
    from tests.test_export_gpu import CF_PASS, SF_CANDIDATE, export
    rng = np.random.default_rng(n_pass)
    n = 2 * n_pass + 40
    pos = 8 + 7 * np.arange(n, dtype=np.int64)                               # nine or ten sites a tile
    is_pass = np.zeros(n, bool); is_pass[rng.choice(n, n_pass, replace=False)] = True
    deep = rng.random(n) < 0.5
    seq = np.frombuffer(("ACGT" * (int(pos[-1]) // 4 + 32)).encode(), np.uint8).copy()
    rows0 = np.zeros((n, cases.ROW_WORDS), np.uint32)
    for i in range(n):
        ref = LETTER_SYM[int(seq[pos[i]])]
        alt = [s for s in (A, C_, T, G) if s != ref][i % 3]
        dp = 2048 if deep[i] else 100
        rows0[i] = cases.cand_row(ref, [(alt, (dp // 2 if is_pass[i] else 1, dp), (10 if is_pass[i] else 1, 20))])
    with_ct1 = rng.random(n) < 0.5                                           # the other cell type: reference reads only
    rows1 = np.stack([cases.make_row(30, 10, {LETTER_SYM[int(seq[p])]: 30}, {LETTER_SYM[int(seq[p])]: 10}) for p in pos[with_ct1]])
    install(engine, [seq], [(pos, None, rows0), (pos[with_ct1], None, rows1)])
    monkeypatch.setenv("LSG_TIMING", "1")
    engine.call_step1(CallParams.longsom_defaults(min_cell_types=1))
    line = call_lines(capfd)[-1]
    assert line["n_pass"] == n_pass and line["waited"] == int(deep.sum())
    calls = engine.fetch_calls()
    keep = (calls["site_filter"] == SF_CANDIDATE) & (calls["ct_filter"] == CF_PASS).any(axis=1)
    assert np.array_equal(keep, is_pass)
    assert n_pass == 1 or 0 < (keep & deep).sum() < n_pass                   # both kernels appended
    want = calls[keep].tobytes()
    capfd.readouterr()
    assert export(engine, 2).tobytes() == want
    how = EXPORT_LINE.findall(capfd.readouterr().err)
    assert how == [("PASS list" if n_pass <= cases.PASS_CAP else "scan", str(n_pass))], how
    if n_pass == 1025:
        monkeypatch.setenv("LSG_NO_PASS_LIST", "1")
        assert export(engine, 2).tobytes() == want
        assert EXPORT_LINE.findall(capfd.readouterr().err) == [("scan", "1025")]
