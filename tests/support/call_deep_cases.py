"""Shared by test_call_deep_cpu.py, test_call_deep_gpu.py and tools/make_call_deep_goldens.py: the pairs (k, n) at which the step-1
call's beta-binomial tails leave the table, their classification as the call stage makes it, the exact tail as a 60-digit sum, and
count rows that put a pair into each of the tails a site has."""
import functools
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "call_deep", "tails.json")

# ---- the call stage's classification: host mirror of call.hip's tail_in_table, tail_work and tail_terms --------------------------
TAIL_NT = 2047                 # call.hip: TAIL_NT
LIGHT_MAX_TERMS = 64           # call.hip: tail_work(k, n) > 64 makes a task heavy
GROUP8_MAX_TERMS = 1024        # call.hip: GROUP8_MAX_TERMS
TASK_CHUNK, HEAVY_CHUNK = 64, 16
PASS_CAP = 4096


def tail_in_table(k, n):
    return n <= TAIL_NT and k <= n


def tail_work(k, n):
    if k == 0 or k > n:
        return 0
    return min(k, n - k + 1)


def tail_terms(k, n):
    return k if k <= n - k + 1 else n + 1 - k


def classify(k, n):
    """'table' or 'task' / 'thread' (<= 64 terms), 'lanes8' (65..1024) or 'wave' (>= 1025) / 'lower' (k <= n-k+1) or 'upper'"""
    where = "table" if tail_in_table(k, n) else "task"
    t = tail_terms(k, n)
    width = "thread" if tail_work(k, n) <= LIGHT_MAX_TERMS else ("lanes8" if t <= GROUP8_MAX_TERMS else "wave")
    side = "lower" if k <= n - k + 1 else "upper"
    return "%s/%s/%s" % (where, width, side)


CLASSES = ["%s/%s/%s" % (w, g, s) for w, g in (("table", "thread"), ("table", "lanes8"), ("task", "thread"), ("task", "lanes8"), ("task", "wave"))
           for s in ("lower", "upper")]

# ---- parameter sets: (alpha1, beta1) of the read-count tails, (alpha2, beta2) of the cell-count tails -----------------------------
PARAM_SETS = {
    "defaults": dict(alpha1=0.21356677091082193, beta1=104.95163748636298, alpha2=0.2474528917555431, beta2=162.03696139428595),
    "wide": dict(alpha1=1.7, beta1=2.3, alpha2=0.9, beta2=1.1),     # upper-side sums that are not 0.0000
}
TAILS = ("reads", "cells")
# A third set for one thing only: the re-anchor inside a lane's chunk of group_tail<64>.  With the two sets above a recurrence that is
# never re-anchored ends within 1e-12 of the re-anchored one; it differs where the pmf at the chunk's start is below the doubles'
# range and the mass lies more than 1024 terms further on.  A beta-binomial is at least as wide as its binomial, so this takes a peak
# of a few terms' width next to n: mean 149 936, sigma 8.4.  At (75002, 150000) the last lane sums [148838, 150000]: its start is 130
# sigma below the peak (log pmf -1684: 0.0 as a double), its re-anchor at 149862 nine sigma below (log pmf -32; the terms it skipped
# hold 2e-14), so the tail is 1 to 2e-14 (test_call_deep_cpu.py checks these figures).
PEAKED = dict(alpha1=1499360.0, beta1=640.0, alpha2=1499360.0, beta2=640.0)
PEAKED_PAIRS = [(75002, 150000), (1, 5), (1, 10)]
ALL_SETS = dict(PARAM_SETS, peaked=PEAKED)


def ab(pset, tail):
    p = ALL_SETS[pset]
    return (p["alpha1"], p["beta1"]) if tail == "reads" else (p["alpha2"], p["beta2"])


# ---- the pairs --------------------------------------------------------------------------------------------------------------------
_BORDER_K = (1, 3, 64, 65, 1024, 1025, 1984, 1985, 2047)
PAIRS = (
    [(k, 2047) for k in _BORDER_K] + [(k, 2048) for k in _BORDER_K] +            # table border
    [(2048, 2048)] +                                                             # one term, upper side
    [(1024, 30000), (1025, 30000), (3977, 5000), (3976, 5000)] +                 # eight lanes / wavefront
    [(1025, 2050), (1026, 2050)] +                                               # 1025 terms: 64-lane chunks with empty trailing lanes
    [(66, 2048), (71, 4000), (300, 5000), (1100, 100000), (3000, 150000)] +      # chunks that do not divide
    [(70000, 150000), (80000, 150000)] +                                         # a lane's chunk over 1024 terms
    [(2500, 5000), (2501, 5000), (3000, 5000), (30000, 70000), (40000, 70000), (68000, 70000)] +
    [(1500, 2047), (1100, 2047)] +                                               # a second and third table pair of eight lanes, upper side
    [(1, 5), (1, 10)]                                                            # the shallow companions of the single-tail sites
)
# pairs closer than TIE_MARGIN to a tie (distance in the comment): the neighbour of the same class takes their place, none is dropped
REPLACED = {("wide", "cells", (65, 2048)): (65, 2049),            # 9.5e-8
            ("wide", "cells", (1025, 30000)): (1025, 30001),      # 4.0e-7
            ("wide", "cells", (1, 10)): (1, 11),                  # 5.8e-7
            ("defaults", "cells", (66, 2048)): (66, 2049)}        # 8.4e-7
THRESHOLD_VALUES = (9, 10, 11, 499, 500)                     # round(p, 4) * 1e4 around the chains' constants 10 and 500
THRESHOLD_N = (2048, 8192)
TIE_MARGIN = 1e-6


def pairs_for(pset, tail):
    if pset == "peaked":
        return list(PEAKED_PAIRS)
    return [REPLACED.get((pset, tail, p), p) for p in PAIRS]


# ---- the exact tail ---------------------------------------------------------------------------------------------------------------
def exact_tails(n, ks, a, b, dps=60):
    """P(X >= k) for every k of ks, X ~ BetaBinomial(n, a, b): 1 - sum_{m<k} pmf(m) with the pmf's recurrence from pmf(0), in mpmath
    at `dps` digits (a, b are taken as the doubles they are).  One pass serves every k of the same n."""
    import mpmath
    with mpmath.workdps(dps):
        A, B, N = mpmath.mpf(a), mpmath.mpf(b), mpmath.mpf(n)
        pm = mpmath.exp(mpmath.loggamma(N + B) + mpmath.loggamma(A + B) - mpmath.loggamma(N + A + B) - mpmath.loggamma(B))
        want = sorted(set(ks))
        out, s, m = {}, mpmath.mpf(0), 0
        for k in want:                                   # s = sum_{j<m} pmf(j), pm = pmf(m)
            while m < k:
                s += pm
                pm = pm * ((N - m) * (m + A)) / ((m + 1) * (N - m - 1 + B))
                m += 1
            out[k] = 1 - s
        return {k: out[k] for k in ks}


def rounded_and_tie(p):
    """(round(p, 4) * 1e4 as an integer, distance of p to the nearest x.xxxx5) of an mpmath or float value, without rounding p first"""
    import mpmath
    with mpmath.workdps(60):
        x = mpmath.mpf(p) * 10000
        if x < 0:
            x = mpmath.mpf(0)
        fl = mpmath.floor(x)
        tie = abs(x - fl - mpmath.mpf("0.5")) / 10000
        return int(fl) + (1 if x - fl > mpmath.mpf("0.5") else 0), float(tie)


@functools.lru_cache(maxsize=None)
def load():
    """{pset: {tail: [{"k", "n", "exact", "r4", "class", "tie", "threshold"}]}}"""
    with open(FIXTURE) as f:
        return json.load(f)


def expected(pset, tail):
    """{(k, n): rounded integer}"""
    return {(e["k"], e["n"]): e["r4"] for e in load()[pset][tail]}


# ---- count rows (42 words: 0 DP, 1 NC, 2..9 CC, 10..17 BC, 18..25 BQ, 26..33 forward BC; alleles A C T G I D N O) ----------------------
ROW_WORDS = 42


def make_row(dp, nc, bc, cc):
    """bc, cc: {allele index: count}"""
    r = np.zeros(ROW_WORDS, np.uint32)
    r[0], r[1] = dp, nc
    for s, v in cc.items():
        r[2 + s] = v
    for s, v in bc.items():
        r[10 + s] = v; r[26 + s] = v
    return r


def cand_row(ref, alts):
    """one cell type's row with the candidates alts = [(allele, (kb, nb), (kc, nc))]: every alt's read pair shares nb, every cell pair
    nc; the reference allele takes what is left"""
    nb, nc = alts[0][1][1], alts[0][2][1]
    bc = {s: kb for s, (kb, _), _ in alts}; cc = {s: kc for s, _, (kc, _) in alts}
    bc[ref] = max(nb - sum(bc.values()), 0); cc[ref] = max(nc - sum(cc.values()), 0)
    return make_row(nb, nc, bc, cc)


def site_tasks(rows, rsym, min_cov=5, min_cells=5):
    """what k_call_gather's counting pass makes of one site: (light tasks, heavy tasks).  rows: one row per cell type or None;
    rsym: allele index of the reference base.  A site with any task is deferred to k_call_finish."""
    light = heavy = 0
    s_alts_bc = s_alts_cc = s_dp = s_nc = 0

    def ask(k, n):
        nonlocal light, heavy
        if not tail_in_table(k, n):
            if tail_work(k, n) > LIGHT_MAX_TERMS:
                heavy += 1
            else:
                light += 1

    for r in rows:
        if r is None:
            continue
        dp, nc = int(r[0]), int(r[1])
        if not (dp >= min_cov and nc >= min_cells):
            continue
        s_dp += dp; s_nc += nc
        for s in range(6):
            if s == rsym:
                continue
            b, c = int(r[10 + s]), int(r[2 + s])
            if s < 4 and b > 0:
                s_dp -= b; s_nc -= c
                ask(b, dp); ask(c, nc)
            else:
                s_alts_bc += b; s_alts_cc += c
    if s_alts_bc > 0:
        if s_dp >= 0:
            ask(s_alts_bc, s_dp)
        if s_nc >= 0 and s_alts_cc >= 0:
            ask(s_alts_cc, s_nc)
    return light, heavy
