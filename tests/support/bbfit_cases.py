"""Shared by test_bbfit_cpu.py and test_bbfit_gpu.py: generated beta-binomial rows, their histograms, and the maximum-likelihood root
at 50 digits (mpmath.findroot of the gradient, started from the fit under test - the root is the likelihood's, not the fit's)."""
import functools

import numpy as np

from longsom_amd import bbfit

# (alpha, beta) near config.yaml's values; depths of the rows; rows drawn.  The third shape is the deep one (depths up to 70 000).
SHAPES = {
    "cells": dict(a=0.2136, b=105.0, lo=5, hi=40, rows=3000, seed=11),
    "bases": dict(a=0.2475, b=162.0, lo=5, hi=120, rows=3000, seed=12),
    "deep": dict(a=0.2475, b=162.0, lo=200, hi=70000, rows=800, seed=13),
}


def draw(a, b, lo, hi, rows, seed):
    """(x, n) of `rows` beta-binomial draws with depths uniform in [lo, hi]"""
    rng = np.random.default_rng(seed)
    n = rng.integers(lo, hi + 1, rows)
    x = rng.binomial(n, rng.beta(a, b, rows))
    return x.astype(np.int64), n.astype(np.int64)


def fit_hist(x, n, frac, capacity=None):
    """three histograms (x, n - x, n) of the rows with x / n < frac (the reference's filter on one pair), uint64 [3, capacity]"""
    k = x / n.astype(np.float64) < frac
    x, n = x[k], n[k]
    cap = capacity or bbfit.capacity_for(int(n.max()))
    return np.stack([np.bincount(v, minlength=cap) for v in (x, n - x, n)]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def shape_hist(name):
    """six histograms: the named shape as the cell counts' fit (filter 0.10) and as the base counts' (0.15)"""
    x, n = draw(**SHAPES[name])
    cap = bbfit.capacity_for(int(n.max()))
    return np.concatenate([fit_hist(x, n, 0.10, cap), fit_hist(x, n, 0.15, cap)])


def root50(hx, hy, hn, a0, b0):
    """the root of the likelihood's gradient at 50 digits, as two doubles"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    # sum_j T[j] / (v + j) with T[j] = #{value > j} is sum over the values u of hist[u] (psi(v + u) - psi(v)): one digamma per occupied bin
    T = [[(int(u), int(h[u])) for u in np.flatnonzero(h) if u > 0] for h in (hx, hy, hn)]

    def s1(t, v):
        p0 = mp.digamma(v)
        return mp.fsum(c * (mp.digamma(v + u) - p0) for u, c in t)

    def grad(a, b):
        c = s1(T[2], a + b)
        return s1(T[0], a) - c, s1(T[1], b) - c
    r = mp.findroot(grad, (mp.mpf(a0), mp.mpf(b0)), tol=mp.mpf(10) ** -80, maxsteps=60)
    return float(r[0]), float(r[1])


@functools.lru_cache(maxsize=None)
def shape_roots(name):
    """[alpha1, beta1, alpha2, beta2] of shape_hist(name) at 50 digits (started from the twin's answer)"""
    h = shape_hist(name)
    est, _ = bbfit.solve(h)
    return list(root50(h[0], h[1], h[2], est[0], est[1])) + list(root50(h[3], h[4], h[5], est[2], est[3]))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / np.abs(np.asarray(b, dtype=np.float64))))


def status_cases(cap=4096):
    """three-histogram inputs of the statuses that are not "converged": all alternative counts zero; binomial data with one common p
    and deep sites; no rows.  A binomial sample has a finite beta-binomial maximum when it happens to be over-dispersed, so the
    sample is one whose Pearson statistic lies below its degrees of freedom (stated here, from the data alone)."""
    rng = np.random.default_rng(8)
    big = rng.integers(2000, 4000, 400)
    x = rng.binomial(big, 0.05)
    p = x.sum() / big.sum()
    assert float(((x - big * p) ** 2 / (big * p * (1 - p))).sum()) < len(x) - 1
    n = np.random.default_rng(3).integers(5, 100, 400)
    return dict(zero=fit_hist(np.zeros(400, np.int64), n, 0.15, cap), binomial=fit_hist(x, big, 0.15, cap), empty=np.zeros((3, cap), np.uint64))


def write_normal(bam, fasta, barcodes_tsv, seed, n_reads=400, read_len=1500, contig_len=6000, n_cb=60, genome_seed=7):
    """A small normal whose fit exists.  The project's synthetic reads carry one common mismatch rate: after the reference's filter
    such counts are no more dispersed than a binomial's and the likelihood has no finite maximum.  Here every site has an error
    rate of its own, drawn from Beta(0.3, 60), so the alternative counts are beta-binomial by construction.  Reads of read_len
    bases at uniform starts on one contig, plain matches, quality 40, one of n_cb barcodes (two cell types, half each).  The genome
    and its sites' rates come from genome_seed (the same for every normal of a panel), the reads from seed."""
    from longsom_amd import hostio
    from tests.support import bamwrite
    rng = np.random.default_rng(genome_seed)
    ref = rng.integers(0, 4, contig_len)
    rate = rng.beta(0.3, 60.0, contig_len)
    rng = np.random.default_rng(seed)
    with open(fasta, "w") as f:
        f.write(">chr1\n" + "".join("ACGT"[b] for b in ref) + "\n")
    cbs = ["".join("ACGT"[b] for b in np.random.default_rng(1000 + i).integers(0, 4, 16)) for i in range(n_cb)]
    hostio.write_barcodes_tsv(barcodes_tsv, cbs, (np.arange(n_cb) % 2).astype(np.uint8), ["Epithelial", "Stromal"])
    starts = np.sort(rng.integers(1, contig_len - read_len, n_reads))
    records = []
    for i, st in enumerate(starts.tolist()):
        base = ref[st:st + read_len].copy()
        err = rng.random(read_len) < rate[st:st + read_len]
        base[err] = (base[err] + 1 + rng.integers(0, 3, int(err.sum()))) % 4
        records.append(dict(tid=0, pos=st, name="r%d" % i, flag=16 if i % 2 else 0, mapq=60, cigar="%dM" % read_len,
                            seq="".join("ACGT"[b] for b in base), qual=[40] * read_len, tags={"CB": cbs[int(rng.integers(n_cb))]}))
    bamwrite.write_bam(bam, [("chr1", contig_len)], records)
