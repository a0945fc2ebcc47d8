"""The beta-binomial fit of the panel-of-normals branch (scripts/PoN/BetaBinEstimation.py) without R: the alpha / beta of the step-1
calls and of SingleCellGenotype, fitted on the device from the resident count rows (csrc/bbfit.hip).  This module is the numpy twin
those kernels are held to, the reference's output file, and the file route over BaseCellCounter tables.

What the reference does.  Per row of a BaseCellCounter table (extract_sites_for_betabinom_estimation, :64-111): Alt_BC = the sum of
BC over the alleles that are not REF, Ref_BC = DP - Alt_BC, Alt_CC / Ref_CC the same over CC and NC; the row is
kept iff Alt_CC / float(NC) < 0.10 and Alt_BC / float(DP) < 0.15 (double division: 3 / 30 is not kept).  Two fits of
vglm(cbind(x, y) ~ 1, betabinomialff): (Alt_BC, Ref_BC) gives alpha2 / beta2, (Alt_CC, Ref_CC) gives alpha1 / beta1.
The script lists eight alleles (A C T G I D N O) but reads tables, and a BaseCellCounter table prints six (A C T G I D,
BaseCellCounter.py:300): counts of N and O never reach its sums and stay on the Ref side of DP - Alt.  The resident rows do carry
the N and O planes; the six printed alleles are what is summed here, so that a fit from resident rows is the fit from their table.

The arithmetic here.  With the tail counts A[j] = #{x_i > j}, B[j] = #{y_i > j}, C[j] = #{x_i + y_i > j} the log-likelihood is
    l(a, b) = sum_j A[j] log(a + j) + sum_j B[j] log(b + j) - sum_j C[j] log(a + b + j)  + a constant,
so the data of both fits are six value histograms (Alt_CC, Ref_CC, NC, Alt_BC, Ref_BC, DP: HIST_NAMES), which add over cell types,
normals and ranks.  The solve is Newton in (log a, log b):
    start   method of moments from the marginal moments of x and n: p = E x / E n, rho = ((Var x - p^2 Var n) / (p q) - E n) /
            (E n^2 - E n), s = 1 / rho - 1 with rho held in [1e-4, 0.9999], a = p s, b = q s, each held in [1e-6, 1e6]
    step    d = -H^-1 g of the log-parameters; where H is not negative definite (eigenvalues lmax >= 0, lmin) it is first shifted by
            lmax + 0.01 max(|lmin|, |lmax|) times the identity; d's larger component is held to 2; d is halved (at most 30 times)
            while l drops by more than 1e-10 |l|
    stop    both components of d below 1e-12 (the step is taken): converged; 100 iterations: the cap; an iterate outside
            [1e-8, 1e8]: no finite maximum (all alternative counts zero, or data no more dispersed than a binomial's)
Every sum over j is taken over the occupied part of its histogram alone.  The gradient's three sums cancel to nothing at the root: in
plain doubles their rounding leaves steps of about 1e-12, the size of the stop rule, so each term T[j] / (v + j) is carried as a
quotient and the quotient of its remainder and the sums are taken exactly (math.fsum here, pairs of doubles on the device).

Divergences from the reference, stated: (1) the answer is the maximum-likelihood estimate to the stop rule above, not the last
iterate of VGAM's Fisher scoring (epsilon 1e-7); (2) the default is every eligible site, not 500 000 sampled lines; (3) --n_sites
thins by a Philox stream of its own - row r of table t is kept iff uniform(seed; t, r) < sample_n / n_rows, decided before the
filter - where the reference seeks to random byte offsets with replacement.
"""
import math
import os
from typing import Sequence

import numpy as np

from . import bnpc_sampler

HIST_NAMES = ("Alt_CC", "Ref_CC", "NC", "Alt_BC", "Ref_BC", "DP")
FIT_NAMES = ("cell counts", "base counts")          # fit 0: histograms 0-2 -> alpha1, beta1; fit 1: histograms 3-5 -> alpha2, beta2
CONVERGED, ITERATION_CAP, NO_DATA, NO_FINITE_MAXIMUM = 0, 1, 2, 3
STATUS_TEXT = ("converged", "the iteration cap was reached", "no row was kept", "the likelihood has no finite maximum "
               "(all alternative counts are zero, or the data are no more dispersed than a binomial's)")
MAX_ITER, STEP_TOL, LO, HI = 100, 1e-12, 1e-8, 1e8
ALLELES = b"ACTGID"          # the alleles a table prints, in the rows' plane order

_SYM = np.full(256, -1, np.int64)
for _i, _c in enumerate(ALLELES):
    _SYM[_c] = _i


# ---- the rows ----------------------------------------------------------------------------------------------------------------------
def site_counts(refs, counts):
    """(Alt_CC, Ref_CC, NC, Alt_BC, Ref_BC, DP) as int64 arrays of count rows (uint32 [n, 42]: DP, NC, CC[8], BC[8], ...) and their
    REF bytes.  A REF outside the six printed letters sums all six (BetaBinEstimation.py:90-91)."""
    c = np.asarray(counts).reshape(-1, np.asarray(counts).shape[-1]).astype(np.int64)
    refs = np.frombuffer(refs, np.uint8) if isinstance(refs, (bytes, bytearray)) else np.asarray(refs, dtype=np.uint8)
    sym = _SYM[refs]
    rows = np.arange(len(c))
    dp, nc, cc, bc = c[:, 0], c[:, 1], c[:, 2:8], c[:, 10:16]
    own = lambda m: np.where(sym >= 0, m[rows, np.maximum(sym, 0)], 0)
    alt_cc, alt_bc = cc.sum(1) - own(cc), bc.sum(1) - own(bc)
    return alt_cc, nc - alt_cc, nc, alt_bc, dp - alt_bc, dp


def kept(alt_cc, nc, alt_bc, dp):
    """:101-104, Python's double division; a row with NC or DP zero stops the reference (ZeroDivisionError) and is an error here"""
    nc, dp = np.asarray(nc), np.asarray(dp)
    if np.any(nc == 0) or np.any(dp == 0):
        raise ValueError("a count row with DP or NC zero")
    return (np.asarray(alt_cc) / nc.astype(np.float64) < 0.10) & (np.asarray(alt_bc) / dp.astype(np.float64) < 0.15)


def sample_size(n_sites: int, n_tables: int) -> int:
    """:193 (Python's round)"""
    return int(round(n_sites / n_tables)) if n_sites > 0 and n_tables > 0 else 0


def thin(n_rows: int, table: int, sample_n: int, seed: int):
    """the rows of table `table` that --n_sites leaves: all where sample_n <= 0 or the table has no more rows than that"""
    if sample_n <= 0 or n_rows <= sample_n:
        return np.ones(n_rows, bool)
    r = np.arange(n_rows, dtype=np.uint64)
    w = bnpc_sampler.philox(seed, table, r & np.uint64(0xFFFFFFFF), r >> np.uint64(32), 0)
    return bnpc_sampler.to_double(w[0], w[1]) < sample_n / n_rows


def histograms(refs, counts, capacity: int, table: int = 0, sample_n: int = 0, seed: int = 1992):
    """one table's six histograms (uint64 [6, capacity]), the rows the thinning left and the rows kept of them"""
    v = site_counts(refs, counts)
    t = thin(len(v[0]), table, sample_n, seed)
    v = [x[t] for x in v]
    k = kept(v[0], v[2], v[3], v[5])
    hist = np.zeros((6, capacity), np.uint64)
    for h, x in zip(hist, v):
        x = x[k]
        if len(x) and int(x.max()) >= capacity:
            raise ValueError("value %d does not fit the histograms' capacity %d" % (int(x.max()), capacity))
        h += np.bincount(x, minlength=capacity).astype(np.uint64)
    return hist, int(t.sum()), int(k.sum())


# ---- the solve ---------------------------------------------------------------------------------------------------------------------
def tails(h):
    """tail counts T[j] = #{value > j} over the occupied part of a histogram, as doubles"""
    h = np.asarray(h, dtype=np.uint64)
    nz = np.flatnonzero(h)
    if not len(nz):
        return np.zeros(0)
    n = int(nz[-1])                                    # the largest value: T[j] = 0 from there on
    cs = np.cumsum(h[:n + 1].astype(np.int64))
    return (cs[-1] - cs[:n]).astype(np.float64)


def _moments(hx, hn):
    hx, hn = np.asarray(hx, dtype=np.float64), np.asarray(hn, dtype=np.float64)
    vx, vn = np.arange(len(hx), dtype=np.float64), np.arange(len(hn), dtype=np.float64)
    rows = math.fsum(hn)
    return rows, math.fsum(hx * vx), math.fsum(hx * vx * vx), math.fsum(hn * vn), math.fsum(hn * vn * vn)


def start(hx, hn):
    """the method-of-moments start (module docstring); None without rows"""
    rows, sx, sxx, sn, snn = _moments(hx, hn)
    if rows == 0 or sn == 0:
        return None
    ex, ex2, en, en2 = sx / rows, sxx / rows, sn / rows, snn / rows
    p = min(max(ex / en, 1e-6), 1.0 - 1e-6)
    q = 1.0 - p
    den = en2 - en
    rho = ((ex2 - ex * ex - p * p * (en2 - en * en)) / (p * q) - en) / den if den > 0 else 0.0
    if not rho > 1e-4:
        rho = 1e-4
    if rho > 0.9999:
        rho = 0.9999
    s = 1.0 / rho - 1.0
    return min(max(p * s, 1e-6), 1e6), min(max(q * s, 1e-6), 1e6)


def _sums(t, v, with_log=False):
    j = np.arange(len(t), dtype=np.float64)
    if with_log:
        return math.fsum(t * np.log(v + j))
    r = 1.0 / (v + j)
    return math.fsum(t * r * r)


def loglik(A, B, Cc, a, b):
    return _sums(A, a, True) + _sums(B, b, True) - _sums(Cc, a + b, True)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _quotients(t, v, v_lo=0.0):
    """t[j] / (v + v_lo + j) as unevaluated pairs of doubles (a quotient and the quotient of its remainder).  The gradient is a
    difference of such sums that cancels to nothing at the root: in plain doubles its rounding leaves steps of 1e-12 in the
    log-parameters, the size of the stop rule itself."""
    j = np.arange(len(t), dtype=np.float64)
    s, e = _two_sum(np.float64(v), j)
    e = e + v_lo
    q = t / s
    p, pe = _two_prod(q, s)
    return q, (((t - p) - pe) - q * e) / s


def gradient(A, B, Cc, a, b):
    """(dl/da, dl/db): each the exactly rounded sum (math.fsum) of the pairs of _quotients"""
    s, e = _two_sum(np.float64(a), np.float64(b))
    qa, qb, qc = _quotients(A, a), _quotients(B, b), _quotients(Cc, float(s), float(e))
    neg = [-qc[0], -qc[1]]
    return math.fsum(np.concatenate(list(qa) + neg)), math.fsum(np.concatenate(list(qb) + neg))


def solve_one(hx, hy, hn, max_iter: int = MAX_ITER):
    """one fit: (alpha, beta, info) with info = dict(iterations, status, last_step, grad_norm)"""
    info = dict(iterations=0, status=NO_DATA, last_step=0.0, grad_norm=0.0)
    st = start(hx, hn)
    if st is None:
        return float("nan"), float("nan"), info
    a, b = st
    A, B, Cc = tails(hx), tails(hy), tails(hn)
    info["status"] = ITERATION_CAP
    for it in range(1, max_iter + 1):
        a2, b2, c2 = _sums(A, a), _sums(B, b), _sums(Cc, a + b)
        l0 = loglik(A, B, Cc, a, b)
        ga, gb = gradient(A, B, Cc, a, b)
        g1, g2 = a * ga, b * gb
        h11, h22, h12 = a * a * (c2 - a2) + g1, b * b * (c2 - b2) + g2, a * b * c2
        disc = math.sqrt((h11 - h22) * (h11 - h22) + 4.0 * h12 * h12)
        lmax, lmin = 0.5 * (h11 + h22 + disc), 0.5 * (h11 + h22 - disc)          # H's eigenvalues
        if not lmax < 0:                               # not negative definite (a start far out on the ridge): shifted until it is
            shift = lmax + 0.01 * max(abs(lmin), abs(lmax))
            h11, h22 = h11 - shift, h22 - shift
        det = h11 * h22 - h12 * h12
        d1, d2 = -(h22 * g1 - h12 * g2) / det, -(h11 * g2 - h12 * g1) / det
        m = max(abs(d1), abs(d2))
        if m > 2.0:
            d1, d2, m = d1 * (2.0 / m), d2 * (2.0 / m), 2.0
        info.update(iterations=it, last_step=m, grad_norm=math.hypot(g1, g2))
        if not m == m:                                 # (a NaN: nothing finite to go on with)
            info["status"] = NO_FINITE_MAXIMUM
            break
        t = 1.0
        if m < STEP_TOL:
            a, b = a * math.exp(d1), b * math.exp(d2)
            info["status"] = CONVERGED
            break
        for _ in range(30):
            na, nb = a * math.exp(t * d1), b * math.exp(t * d2)
            if loglik(A, B, Cc, na, nb) >= l0 - 1e-10 * abs(l0):
                break
            t *= 0.5
        a, b = na, nb
        if not (LO <= a <= HI and LO <= b <= HI):
            info["status"] = NO_FINITE_MAXIMUM
            break
    return a, b, info


def solve(hist, max_iter: int = MAX_ITER):
    """both fits of six histograms: ([alpha1, beta1, alpha2, beta2], [info of the cell counts' fit, info of the base counts' fit])"""
    hist = np.asarray(hist)
    est, infos = [], []
    for f in range(2):
        a, b, info = solve_one(hist[3 * f], hist[3 * f + 1], hist[3 * f + 2], max_iter)
        est += [a, b]
        infos.append(info)
    return est, infos


class FitFailed(RuntimeError):
    pass


def require_converged(infos) -> None:
    """raises FitFailed naming the fit and the reason unless both fits converged"""
    for name, info in zip(FIT_NAMES, infos):
        if info["status"] != CONVERGED:
            raise FitFailed("the beta-binomial fit of the %s did not converge: %s (after %d iterations, last step %.3g, gradient norm %.3g)"
                            % (name, STATUS_TEXT[info["status"]], info["iterations"], info["last_step"], info["grad_norm"]))


# ---- the reference's file ------------------------------------------------------------------------------------------------------------
def estimates_text(est) -> str:
    """BetaBinEstimation.py:214-217: pandas' to_csv of one row of four floats (repr: the shortest text that reads back the same)"""
    return "alpha1\tbeta1\talpha2\tbeta2\n" + "\t".join(repr(float(x)) for x in est) + "\n"


def write_estimates(path: str, est) -> None:
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write(estimates_text(est))


# ---- the device route ---------------------------------------------------------------------------------------------------------------
def capacity_for(max_value: int) -> int:
    """bins that hold every value up to max_value, in whole 1024s"""
    return (int(max_value) + 1 + 1023) // 1024 * 1024


def device_solve(engine):
    """lsg_bbfit_solve over the engine's histograms; raises FitFailed unless both fits converged"""
    est, infos = engine.bbfit_solve()
    require_converged(infos)
    return est, infos


def fit_tables(engine, paths: Sequence[str], n_sites: int = 0, seed: int = 1992):
    """The file route: every BaseCellCounter table of `paths` parsed, installed (engine.load_counts) and accumulated with its own REF
    column - no FASTA is named.  Returns ([alpha1, beta1, alpha2, beta2], infos, rows seen, rows kept)."""
    from . import tsvio
    paths = list(paths)
    if not paths:
        raise FitFailed("no count table to fit")
    contigs = tsvio.contigs_of_tsv(paths)
    sample_n = sample_size(n_sites, len(paths))
    tables = []
    for p in paths:
        k, r, c = tsvio.parse_counts_tsv(p, contigs)[:3]
        tables.append((k, r, c))
    lens = np.ones(len(contigs), np.int64)
    top = 0
    for k, r, c in tables:
        if len(k):
            np.maximum.at(lens, (k >> 32).astype(np.int64), (k & 0xFFFFFFFF) + 1)
            top = max(top, int(c[:, :2].max()))
    engine.set_contigs(lens)
    engine.bbfit_reset(capacity_for(top))
    seen = kept_rows = 0
    for t, (k, r, c) in enumerate(tables):
        engine.load_counts([k], [c])
        s, kk = engine.bbfit_accumulate(0, ref=r, table=t, sample_n=sample_n, seed=seed)
        seen += s
        kept_rows += kk
    est, infos = device_solve(engine)
    return est, infos, seen, kept_rows
