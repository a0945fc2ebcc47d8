#!/usr/bin/env python3
"""Writes tests/golden/call_deep/tails.json: for every parameter set and tail of tests/support/call_deep_cases.py, the listed pairs
(k, n) and the threshold pairs (found here with scipy, n in 2048..8192, rounding to 0.0009, 0.001, 0.0011, 0.0499 and 0.05), each with
its exact value (60-digit mpmath sum), the rounded integer, the call stage's class and the distance to a 4-decimal rounding tie.
A pair closer than 1e-6 to a tie is left out and reported; the CPU test bounds how many may be.

    python tools/make_call_deep_goldens.py
"""
import json
import os
import sys

import numpy as np
from scipy.stats import betabinom

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.support import call_deep_cases as cases   # noqa: E402


def threshold_candidates(a, b, value, taken):
    """pairs whose scipy tail rounds to value / 1e4 and lies well off a tie, in ascending n (a generator: under the defaults the
    tail moves by more than 1e-4 from one k to the next near 0.05, and most n have no such k)"""
    lo, hi = cases.THRESHOLD_N
    for n in range(lo, hi + 1):
        base, k0 = 0.0, 0
        while k0 < n:                                                            # blocks of k, until the tail is below every value
            pm = betabinom.pmf(np.arange(k0, min(k0 + 512, n)), n, a, b)
            sf = 1.0 - (base + np.concatenate([[0.0], np.cumsum(pm)]))           # sf[j] = P(X >= k0 + j)
            x = sf[:-1] * 1e4
            for j in np.nonzero((np.rint(x) == value) & (np.abs(x - np.floor(x) - 0.5) > 0.1))[0]:
                if k0 + j >= 1 and (int(k0 + j), n) not in taken:
                    yield int(k0 + j), n
            if sf[-1] * 1e4 < value - 1:
                break
            base += float(pm.sum()); k0 += 512


def main():
    out, dropped = {}, []
    for pset in cases.ALL_SETS:
        out[pset] = {}
        for tail in cases.TAILS:
            a, b = cases.ab(pset, tail)
            pairs = cases.pairs_for(pset, tail)
            assert len(set(pairs)) == len(pairs), "a pair is listed twice"
            thr = {}
            for v in cases.THRESHOLD_VALUES if pset in cases.PARAM_SETS else ():
                for k, n in threshold_candidates(a, b, v, set(pairs) | set(thr)):                                                # the first whose EXACT value agrees and keeps the margin
                    r4, tie = cases.rounded_and_tie(cases.exact_tails(n, [k], a, b)[k])
                    if r4 == v and tie >= cases.TIE_MARGIN:
                        thr[(k, n)] = v
                        break
                else:
                    raise AssertionError("no exact pair for %d under %s/%s" % (v, pset, tail))
            by_n = {}
            for k, n in pairs + list(thr):
                by_n.setdefault(n, []).append(k)
            rows = []
            for n in sorted(by_n):
                ex = cases.exact_tails(n, by_n[n], a, b)
                for k in sorted(by_n[n]):
                    r4, tie = cases.rounded_and_tie(ex[k])
                    if tie < cases.TIE_MARGIN:
                        dropped.append((pset, tail, k, n, tie))
                        continue
                    rows.append({"k": k, "n": n, "exact": float(ex[k]), "r4": r4, "class": cases.classify(k, n), "tie": tie,
                                 "threshold": thr.get((k, n))})
            out[pset][tail] = rows
            print(pset, tail, len(rows), "pairs;", "thresholds", sorted(thr.items(), key=lambda kv: kv[1]), flush=True)
    for d in dropped:
        print("left out (tie margin): %s/%s (%d, %d) at %.3g" % d)
    os.makedirs(os.path.dirname(cases.FIXTURE), exist_ok=True)
    with open(cases.FIXTURE, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
