"""BnpC's sampler (scripts/CellClustering/libs/CRP.py:17-410, libs/MCMC.py:200-388) for the model with fixed error rates: Gibbs assignment
sweeps, the Escobar-West concentration update and the parameter Metropolis-Hastings, all chains of a run at once.  The split-merge move,
the error-rate updates, --fixed_assignment, --runtime and --lugsail are not here.

run_chains        the sampler on the device (csrc/bnpc_sampler.hip, lsg_bnpcs_*)
run_chains_host   its twin in numpy: what the CPU tests hold to the reference's goldens, and the GPU tests compare the device against
Both return the reference's list of result dicts (assignments, params, DP_alpha, FN, FP, ML, MAP, burn_in): bnpc.concat_chains,
bnpc.save_chains and bnpc.posterior_estimate take it as it is.

The data are 0 / 1 / missing, so a cell is two bit masks (one, zero) and every likelihood is a sum over them:
  L1[k][m] = log(theta (1 - FN) + (1 - theta) FP),  L0[k][m] = log(theta FN + (1 - theta)(1 - FP))         (_calc_ll, CRP.py:197-212)
  ll(i, k) = sum_m one[i][m] L1[k][m] + zero[i][m] L0[k][m]
with theta float32 and (1 - theta) rounded to float32 before it meets a double, as numpy does it in the reference.  Per cluster the
parameter move and ML / MAP need only the counts n1[k][m], n0[k][m] of the cluster's cells.

THE STREAM.  The sampler does not reproduce numpy's Mersenne stream; it has its own, shared by the kernels and this twin.
  Generator   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85).  The key is the chain's 64-bit
              seed (low word, high word); the counter is (index, step, purpose | sub << 8, attempt).
  Double      from the words (w0, w1) of a block: ((w1 << 32 | w0) >> 12) + 0.5, times 2^-52: 52 drawn bits and the half unit make the
              53-bit mantissa, so the value is exact and never 0 or 1.  (w2, w3) give the block's second double the same way.
  Purposes    see P_* below.  `sub` carries a cell or a cluster id (< 65536).
THE VARIATES.
  Permutation   of the cells: ascending by (the 64-bit draw w1 << 32 | w0 of block (cell, step, P_PERM, 0), cell).
  Categorical   numpy's choice(p=...) rule: cdf = running sum of p, divided by its last element; the first slot whose cdf exceeds u wins.
                Clusters in ascending id, the new cluster last.  u: first double of block (cell, step, P_CHOICE, 0).
  Truncated normal on [TMIN, TMAX] around `old` with sd: a = (TMIN - old) / sd, b = (TMAX - old) / sd (the differences in float32, as
                numpy forms them), x = old + sd ndtri(ndtr(a) + u (ndtr(b) - ndtr(a))), cast to float32.  Its logpdf at x:
                -z^2 / 2 - log(2 pi) / 2 - log sd - log(ndtr(b) - ndtr(a)), z = (x - old) / sd (the difference in float32).
  Gamma(a)      Marsaglia-Tsang: a' = a (+ 1 if a < 1), d = a' - 1/3, c = 1 / sqrt(9 d).  Try t = 0 .. 63: (u1, u2) = the doubles of
                block (.., attempt 2 t), (u3, u4) of block (.., 2 t + 1); x = sqrt(-2 ln u1) cos(2 pi u2); v = (1 + c x)^3; accepted
                if v > 0 and ln u3 < x^2 / 2 + d - d v + d ln v; the value is d v, times u4^(1 / a) if a < 1.  After 64 refusals the
                value is a (the mean) and an error is counted.
  Beta(a, b)    x / (x + y) of Gamma(a) under purpose P and Gamma(b) under purpose P + 1; 0.5 if both are 0.
THE STEP (Chain.do_step, MCMC.py:320-337, with sm_prob = 0), step s >= 1:
  sweep   update_assignments_Gibbs (CRP.py:254-288) over the permuted cells.  A cell leaves its cluster; the log posterior of every live
          cluster (ll + log size - log(N - 1 + alpha)) and of a new one (get_lpost_single_new_cluster, :230-234) are normalised by
          _normalize_log_probs (:89-100, with its clip at log EPSILON) and one is drawn.  A new cluster takes the smallest free id
          (get_empty_cluster) and draws theta[m] ~ Beta(p + one[i][m], q + zero[i][m]) (_init_cl_params_new: a missing entry counts 0
          towards both), block (m, s, P_BIRTH | cell << 8, .), clipped to [TMIN, TMAX], float32.
  alpha   (u0, u1) = the doubles of block (0, s, P_DPA, 0).  If u0 < dpa_prob: update_DP_alpha (:386-410) as written: eta ~ Beta(alpha + 1,
          N) (P_ETA), w = (g0 + k - 1) / (N (g1 - ln eta)), the shape is g0 + k if u1 < w / (1 + w), else g0 + k - 1, and g1 - ln eta
          enters as numpy's *scale*: alpha = max(1 + EPSILON, Gamma(shape) (g1 - ln eta)) (P_ALPHA).
  move    MH_cluster_params / _get_log_A (:314-383) with trans_prob = False, per live cluster k and mutation m: (u, v) = the doubles of
          block (m, s, P_MH | k << 8, 0), sd = (0.1, 0.25, 0.5)[w0 % 3] of block (m, s, P_MH | k << 8, 1); the proposal is the truncated
          normal at u; it is declined iff ln v >= A.
  record  Chain.update_results (MCMC.py:242-282): ML, MAP, DP_alpha, FN, FP, the labels; from the first step after burn-in the theta rows
          of the live clusters in ascending id.
The start (CRP.init(mode='random'), :139-148, :176-180): label i = floor(N u) of block (i, 0, P_INIT_LABEL, 0), compacted to 0 .. K-1 in
ascending order; theta[k][m] = clip(u) of block (m, 0, P_INIT_THETA | k << 8, 0); alpha = the mean of scipy's gamma(*DP_a_gamma), whose
second number is a `loc`: g0 + g1, so a negative -ap gives (sqrt N, 1) and a start at sqrt N + 1.
"""
import numpy as np

EPSILON = np.finfo(np.float64).resolution          # CRP.py:11
LOG_EPSILON = np.log(EPSILON)
TMIN = 1e-5
TMAX = 1 - TMIN
TMIN32, TMAX32 = np.float32(TMIN), np.float32(TMAX)
PROPOSAL_SD = np.array([0.1, 0.25, 0.5])
GAMMA_TRIES = 64
MAX_CELLS = 65535                                 # the estimate keeps 16-bit labels

P_PERM, P_CHOICE, P_BIRTH, P_BIRTH_B, P_DPA, P_ETA, P_ETA_B, P_ALPHA, P_MH, P_INIT_LABEL, P_INIT_THETA = range(1, 12)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


# ---- the stream ----------------------------------------------------------------------------------------------------------------
def philox(key, c0, c1, c2, c3):
    """Philox4x32-10 of the counters (c0, c1, c2, c3), broadcast against each other, under the 64-bit key: four uint32 arrays"""
    key = int(key)
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _LO for c in (c0, c1, c2, c3)])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def to_double(lo, hi):
    x = (np.asarray(hi, dtype=np.uint64) << _S32 | np.asarray(lo, dtype=np.uint64)) >> np.uint64(12)
    return (x.astype(np.float64) + 0.5) * 2.0 ** -52


def doubles(key, index, step, purpose, attempt=0, sub=0):
    w = philox(key, index, step, np.asarray(purpose, dtype=np.uint64) | (np.asarray(sub, dtype=np.uint64) << np.uint64(8)), attempt)
    return to_double(w[0], w[1]), to_double(w[2], w[3])


class Margin:
    """the smallest distance of any decision from its edge: of u to a cdf edge, of a test to its threshold; and the clusters born"""

    def __init__(self):
        self.value = np.inf
        self.births = 0

    def see(self, d):
        d = np.asarray(d)
        if d.size:
            self.value = min(self.value, float(np.min(np.abs(d))))


# ---- the variates ----------------------------------------------------------------------------------------------------------------
def gamma_variate(key, shape, index, step, purpose, sub=0, margin=None):
    """Gamma(shape, 1) per element of the broadcast (shape, index, sub); returns (values, number of elements that ran out of tries)"""
    shape, index, sub = np.broadcast_arrays(np.asarray(shape, dtype=np.float64), np.asarray(index, dtype=np.uint64), np.asarray(sub, dtype=np.uint64))
    flat = shape.ravel()
    a1 = np.where(flat < 1, flat + 1, flat)
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = flat.copy()                                                # an element that runs out of tries keeps the mean
    todo = np.arange(flat.size)
    idx, sb = index.ravel(), sub.ravel()
    with np.errstate(all="ignore"):
        for t in range(GAMMA_TRIES):
            if not todo.size:
                break
            u1, u2 = doubles(key, idx[todo], step, purpose, 2 * t, sb[todo])
            u3, u4 = doubles(key, idx[todo], step, purpose, 2 * t + 1, sb[todo])
            x = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
            base = 1.0 + c[todo] * x
            v = base * base * base
            dd = d[todo]
            rhs = 0.5 * x * x + dd - dd * v + dd * np.log(np.where(v > 0, v, 1.0))
            lu = np.log(u3)
            ok = (v > 0) & (lu < rhs)
            if margin is not None:
                margin.see(base)
                margin.see((lu - rhs)[v > 0])
            g = dd * v
            small = flat[todo] < 1
            g = np.where(small, g * np.power(u4, 1.0 / np.where(small, flat[todo], 1.0)), g)
            out[todo[ok]] = g[ok]
            todo = todo[~ok]
    return out.reshape(shape.shape), int(todo.size)


def beta_variate(key, a, b, index, step, purpose, sub=0, margin=None):
    x, e1 = gamma_variate(key, a, index, step, purpose, sub, margin)
    y, e2 = gamma_variate(key, b, index, step, purpose + 1, sub, margin)
    s = x + y
    with np.errstate(all="ignore"):
        return np.where(s > 0, x / np.where(s > 0, s, 1.0), 0.5), e1 + e2


def _f32diff(bound32, x32):
    """(bound - x) as numpy forms it for a float32 array and a Python float: in float32"""
    return (bound32 - np.asarray(x32, dtype=np.float32)).astype(np.float64)


def truncnorm_mass(loc32, sd):
    from scipy.special import ndtr
    pa, pb = ndtr(_f32diff(TMIN32, loc32) / sd), ndtr(_f32diff(TMAX32, loc32) / sd)
    return pa, pb


def truncnorm_variate(u, old32, sd):
    from scipy.special import ndtri
    pa, pb = truncnorm_mass(old32, sd)
    return (np.asarray(old32, dtype=np.float64) + sd * ndtri(pa + u * (pb - pa))).astype(np.float32)


def truncnorm_logpdf(x32, loc32, sd):
    """log density at x of the normal(loc, sd) truncated to [TMIN, TMAX]"""
    pa, pb = truncnorm_mass(loc32, sd)
    z = (np.asarray(x32, dtype=np.float32) - np.asarray(loc32, dtype=np.float32)).astype(np.float64) / sd
    return -0.5 * z * z - 0.5 * np.log(2.0 * np.pi) - np.log(sd) - np.log(pb - pa)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def beta_mix_const(p, q):
    """CRP.__init__ (:42-44)"""
    from scipy.special import gamma
    mix0 = gamma(p) * gamma(q + 1) / gamma(p + q + 1)
    mix1 = gamma(p + 1) * gamma(q) / gamma(p + q + 1)
    return np.array([mix0, mix1]) / (mix0 + mix1)


def dp_gamma(n_cells, dpa):
    """DP_a_gamma (:51-54) and the start DP_a_prior.mean() (:55-56)"""
    g = (np.sqrt(n_cells), 1) if dpa[0] < 0 or dpa[1] < 0 else (dpa[0], dpa[1])
    return (float(g[0]), float(g[1])), float(g[0]) + float(g[1])


def log_tables(theta32, FN, FP):
    theta32 = np.asarray(theta32, dtype=np.float32)
    th, om = theta32.astype(np.float64), (np.float32(1) - theta32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.log(th * (1 - FN) + om * FP), np.log(th * FN + om * (1 - FP))


def beta_logpdf(x32, p, q):
    """scipy's beta(p, q).logpdf at float32 values (beta_gen._logpdf)"""
    from scipy.special import betaln, xlog1py, xlogy
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    return xlog1py(q - 1.0, -x) + xlogy(p - 1.0, x) - betaln(p, q)


class Model:
    """the fixed part of a run: the data as masks and the constants"""

    def __init__(self, data, FN, FP, pp=(1, 1), dpa=(-1, -1), dpa_prob=0.5, error_prior=None):
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[0] < 2 or data.shape[1] < 1:
            raise ValueError("the sampler needs a cells x mutations matrix of at least 2 x 1, got %r" % (data.shape,))
        if data.shape[0] > MAX_CELLS:
            raise ValueError("%d cells: the sampler takes fewer than 65536 (the estimate keeps 16-bit labels)" % data.shape[0])
        known = ~np.isnan(data)
        if not np.isin(data[known], (0, 1)).all():
            raise ValueError("the data must be 0, 1 or NaN")
        self.N, self.M = data.shape
        self.one, self.zero = data == 1, data == 0
        self.pop1, self.pop0 = self.one.sum(axis=1), self.zero.sum(axis=1)
        self.FN, self.FP = float(FN), float(FP)
        self.p, self.q = float(pp[0]), float(pp[1])
        self.uniform = self.p == self.q == 1
        self.mix = beta_mix_const(self.p, self.q)
        (self.g0, self.g1), self.alpha0 = dp_gamma(self.N, dpa)
        self.dpa_prob = float(dpa_prob)
        self.error_prior = 0.0 if error_prior is None else float(error_prior)      # the error rates' own prior terms in MAP (CRP_learning_errors.py:47-49)
        self.one_f, self.zero_f = self.one.astype(np.float64), self.zero.astype(np.float64)

    def new_cluster_ll(self):
        """get_lpost_single_new_cluster (:230-234) without CRP_prior[-1]: two popcounts times two logs"""
        return self.pop1 * np.log(self.mix[1] * (1 - self.FN) + self.mix[0] * self.FP) + self.pop0 * np.log(self.mix[1] * self.FN + self.mix[0] * (1 - self.FP))

    def masks64(self):
        """(one, zero) as [N][ceil(M / 64)] uint64, bit m % 64 of word m // 64"""
        W = (self.M + 63) // 64
        out = []
        for b in (self.one, self.zero):
            pad = np.zeros((self.N, W * 64), np.uint8)
            pad[:, :self.M] = b
            out.append(np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little").view(np.uint64)))
        return out


class State:
    """one chain: labels [N], sizes [N] (0 = a free id), theta [N][M] float32 (row = cluster id), alpha"""

    def __init__(self, labels, theta, alpha):
        self.labels = np.array(labels, dtype=np.int64)
        self.theta = np.array(theta, dtype=np.float32)
        self.alpha = float(alpha)
        self.sizes = np.bincount(self.labels, minlength=len(self.labels)).astype(np.int64)

    def live(self):
        return np.nonzero(self.sizes)[0]


def initial_state(model, seed):
    N, M = model.N, model.M
    u, _ = doubles(seed, np.arange(N), 0, P_INIT_LABEL)
    raw = np.minimum((u * N).astype(np.int64), N - 1)
    labels = np.unique(raw, return_inverse=True)[1]
    K = int(labels.max()) + 1
    theta = np.zeros((N, M), np.float32)
    ut, _ = doubles(seed, np.arange(M)[None, :], 0, P_INIT_THETA, 0, np.arange(K)[:, None])
    theta[:K] = np.clip(ut, TMIN, TMAX).astype(np.float32)
    return State(labels, theta, model.alpha0)


def crp_prior(sizes, N, alpha):
    """log_CRP_prior (:84-85)"""
    return np.log(np.asarray(sizes, dtype=np.float64)) - np.log(N - 1 + alpha)


def normalize_log_probs(probs):
    """_normalize_log_probs (:89-100)"""
    max_i = int(np.argmax(probs))
    rest = np.delete(probs, max_i) - probs[max_i]
    with np.errstate(under="ignore"):
        norm = probs - probs[max_i] - np.log1p(np.sum(np.exp(rest)))
        return np.exp(np.clip(norm, LOG_EPSILON, 0))


def lpost_single(model, st, cell, live=None, L=None):
    """get_lpost_single (:223-227) of a cell against the live clusters, ascending"""
    live = st.live() if live is None else live
    L1, L0 = log_tables(st.theta[live], model.FN, model.FP) if L is None else L
    return L1 @ model.one_f[cell] + L0 @ model.zero_f[cell] + crp_prior(st.sizes[live], model.N, st.alpha)


def gibbs_sweep(model, st, seed, step, margin=None):
    """update_assignments_Gibbs; returns the number of variates that ran out of tries"""
    N, M = model.N, model.M
    w = philox(seed, np.arange(N), step, P_PERM, 0)
    draw = w[1].astype(np.uint64) << _S32 | w[0].astype(np.uint64)
    order = np.lexsort((np.arange(N), draw))
    us, _ = doubles(seed, np.arange(N), step, P_CHOICE)
    L1, L0 = log_tables(st.theta, model.FN, model.FP)                 # rows of dead ids are never read
    new_ll = model.new_cluster_ll()
    lden = np.log(N - 1 + st.alpha)
    errors = 0
    for cell in order:
        old = st.labels[cell]
        st.sizes[old] -= 1
        live = np.nonzero(st.sizes)[0]
        post = L1[live] @ model.one_f[cell] + L0[live] @ model.zero_f[cell] + (np.log(st.sizes[live].astype(np.float64)) - lden)
        probs = normalize_log_probs(np.append(post, new_ll[cell] + (np.log(st.alpha) - lden)))
        cdf = np.cumsum(probs)
        cdf /= cdf[-1]
        pick = int(np.searchsorted(cdf, us[cell], side="right"))
        if margin is not None:
            margin.see(cdf[:-1] - us[cell])
        if pick >= len(live):
            if margin is not None:
                margin.births += 1
            slot = int(np.nonzero(st.sizes == 0)[0][0])               # get_empty_cluster: the smallest free id
            b, e = beta_variate(seed, model.p + model.one_f[cell], model.q + model.zero_f[cell], np.arange(M), step, P_BIRTH, cell, margin)
            errors += e
            st.theta[slot] = np.clip(b, TMIN, TMAX).astype(np.float32)
            L1[slot], L0[slot] = log_tables(st.theta[slot], model.FN, model.FP)
        else:
            slot = int(live[pick])
        st.labels[cell] = slot
        st.sizes[slot] += 1
    return errors


def alpha_update(model, st, seed, step, margin=None):
    """the draw that decides on it, and update_DP_alpha"""
    u0, u1 = doubles(seed, 0, step, P_DPA)
    if not float(u0) < model.dpa_prob:
        return 0
    k = int(np.count_nonzero(st.sizes))
    eta, e1 = beta_variate(seed, st.alpha + 1, float(model.N), 0, step, P_ETA, 0, margin)
    scale = model.g1 - np.log(float(eta))
    w = (model.g0 + k - 1) / (model.N * scale)
    pi_eta = w / (1 + w)
    if margin is not None:
        margin.see(float(u1) - pi_eta)
    g, e2 = gamma_variate(seed, model.g0 + k if float(u1) < pi_eta else model.g0 + k - 1, 0, step, P_ALPHA, 0, margin)
    st.alpha = max(1 + EPSILON, float(g) * scale)
    return e1 + e2


def counts(model, st):
    """n1, n0 [N][M]: per cluster id and mutation, the cells of the cluster that show 1 resp. 0"""
    n1 = np.zeros((model.N, model.M), np.int64); n0 = np.zeros((model.N, model.M), np.int64)
    np.add.at(n1, st.labels, model.one)
    np.add.at(n0, st.labels, model.zero)
    return n1, n0


def log_A(model, new32, old32, n1, n0, sd, terms=False):
    """_get_log_A (:347-383) with clip False from the cluster's counts"""
    nL1, nL0 = log_tables(new32, model.FN, model.FP)
    oL1, oL0 = log_tables(old32, model.FN, model.FP)
    new_ll, old_ll = n1 * nL1 + n0 * nL0, n1 * oL1 + n0 * oL0
    new_prior = old_prior = 0
    if not model.uniform:
        new_prior, old_prior = beta_logpdf(new32, model.p, model.q), beta_logpdf(old32, model.p, model.q)
    new_p, old_p = truncnorm_logpdf(new32, old32, sd), truncnorm_logpdf(old32, new32, sd)
    A = new_ll + new_prior - old_ll - old_prior + old_p - new_p
    if terms:
        mag = np.abs(n1 * nL1) + np.abs(n0 * nL0) + np.abs(n1 * oL1) + np.abs(n0 * oL0) + np.abs(new_prior) + np.abs(old_prior) + np.abs(old_p) + np.abs(new_p)
        return A, mag
    return A


def parameter_move(model, st, seed, step, margin=None):
    """update_parameters (:302-311) over the live clusters; margin sees |ln v - A| / max(1, |A|)"""
    live = st.live()
    n1, n0 = counts(model, st)
    m = np.arange(model.M)[None, :]
    u, v = doubles(seed, m, step, P_MH, 0, live[:, None])
    w = philox(seed, m, step, np.uint64(P_MH) | (live[:, None].astype(np.uint64) << np.uint64(8)), 1)
    sd = PROPOSAL_SD[w[0] % np.uint32(3)]
    old = st.theta[live]
    new = truncnorm_variate(u, old, sd)
    A = log_A(model, new, old, n1[live], n0[live], sd)
    lv = np.log(v)
    if margin is not None:
        margin.see((lv - A) / np.maximum(1.0, np.abs(A)))
    st.theta[live] = np.where(lv >= A, old, new)


def likelihood(model, labels, theta_rows):
    """get_ll_full (:237-238) from the counts: theta_rows [K][M] are the rows of the K distinct labels, ascending"""
    ids, inv = np.unique(labels, return_inverse=True)
    n1 = np.zeros((len(ids), model.M)); n0 = np.zeros((len(ids), model.M))
    np.add.at(n1, inv, model.one_f)
    np.add.at(n0, inv, model.zero_f)
    L1, L0 = log_tables(theta_rows[:len(ids)], model.FN, model.FP)
    terms = np.concatenate([(n1 * L1).ravel(), (n0 * L0).ravel()])
    return float(terms.sum()), float(np.abs(terms).sum())


def prior_parts(model, st):
    """(sum of CRP_prior over the live clusters, sum of the beta prior's logpdf over their parameters): get_lprior_full (:241-251) without
    the concentration's own term"""
    live = st.live()
    crp = float(np.sum(crp_prior(st.sizes[live], model.N, st.alpha)))
    bsum = 0.0 if model.uniform else float(np.sum(beta_logpdf(st.theta[live], model.p, model.q)))
    return crp, bsum


def alpha_logpdf(model, alpha):
    from scipy.stats import gamma
    with np.errstate(all="ignore"):
        return gamma(model.g0, model.g1).logpdf(np.asarray(alpha, dtype=np.float64))      # the second number is scipy's loc (:55)


def _empty_result(model, steps, burn_in):
    n = steps + 1
    return {"ML": np.zeros(n), "MAP": np.zeros(n), "DP_alpha": np.zeros(n), "FN": np.full(n, model.FN), "FP": np.full(n, model.FP),
            "assignments": np.zeros((n, model.N), dtype=int), "burn_in": burn_in, "_crp": np.zeros(n), "_beta": np.zeros(n), "_rows": []}


def _finish_result(model, r):
    """MAP from its parts (the scalar prior logpdf with scipy, over all steps at once) and the parameter blocks padded to one cluster count"""
    r["MAP"] = r["ML"] + alpha_logpdf(model, r["DP_alpha"]) + r.pop("_crp") + r.pop("_beta") + model.error_prior
    rows = r.pop("_rows")
    k_max = max(b.shape[0] for b in rows)
    params = np.zeros((len(rows), k_max, model.M), np.float32)
    for s, b in enumerate(rows):
        params[s, :b.shape[0]] = b
    r["params"] = params
    return r


def _check_run(steps, burn_in):
    if steps < 1 or not 0 <= burn_in <= steps:
        raise ValueError("steps must be at least 1 and burn_in within [0, steps], got %d and %d" % (steps, burn_in))


def run_chains_host(data, seeds, steps, burn_in, FN, FP, pp=(1, 1), dpa=(-1, -1), dpa_prob=0.5, error_prior=None, states=None):
    """The whole sampler in numpy.  seeds: one 64-bit seed per chain.  states: start there instead of at the random initialisation."""
    _check_run(steps, burn_in)
    model = Model(data, FN, FP, pp, dpa, dpa_prob, error_prior)
    out = []
    for c, seed in enumerate(seeds):
        st = initial_state(model, seed) if states is None else State(states[c].labels, states[c].theta, states[c].alpha)
        r = _empty_result(model, steps, burn_in)
        errors = 0
        for s in range(steps + 1):
            if s:
                errors += gibbs_sweep(model, st, seed, s)
                errors += alpha_update(model, st, seed, s)
                parameter_move(model, st, seed, s)
            live = st.live()
            r["ML"][s] = likelihood(model, st.labels, st.theta[live])[0]
            r["_crp"][s], r["_beta"][s] = prior_parts(model, st)
            r["DP_alpha"][s] = st.alpha
            r["assignments"][s] = st.labels
            if s >= burn_in:
                r["_rows"].append(st.theta[live].copy())
        r["variate_errors"] = errors
        out.append(_finish_result(model, r))
    return out


def run_chains(engine, data, seeds, steps, burn_in, FN, FP, pp=(1, 1), dpa=(-1, -1), dpa_prob=0.5, error_prior=None, states=None, arena_rows=0):
    """The same on the device, all chains in every kernel.  arena_rows: the parameter rows per chain the device holds between two fetches
    (0: enough for 64 kept steps of 64 clusters, at least N rows); a full arena only costs a fetch."""
    _check_run(steps, burn_in)
    model = Model(data, FN, FP, pp, dpa, dpa_prob, error_prior)
    seeds = [int(s) for s in seeds]
    start = [initial_state(model, s) for s in seeds] if states is None else states
    arena_rows = int(arena_rows) or max(model.N, 4096)
    engine.bnpcs_create(model, seeds, steps, arena_rows)
    try:
        for c, st in enumerate(start):
            engine.bnpcs_set_state(c, st.labels, st.theta, st.alpha)
        rows = [[] for _ in seeds]
        done = 0
        while done < steps + 1:
            n = engine.bnpcs_run(done, steps + 1 - done, burn_in)
            labels, scalars, arena = engine.bnpcs_fetch()
            for c in range(len(seeds)):
                at = 0
                for s in range(max(done, burn_in), done + n):
                    k = int(scalars[c, s, 3])
                    rows[c].append(arena[c, at:at + k].copy())
                    at += k
            done += n
        errors = engine.bnpcs_errors()
        out = []
        for c in range(len(seeds)):
            r = _empty_result(model, steps, burn_in)
            r["ML"], r["_crp"], r["_beta"], r["DP_alpha"] = scalars[c, :, 0].copy(), scalars[c, :, 1].copy(), scalars[c, :, 2].copy(), scalars[c, :, 4].copy()
            if model.uniform:
                r["_beta"][:] = 0.0
            r["assignments"] = labels[c].astype(int)
            r["_rows"] = rows[c]
            r["variate_errors"] = int(errors[c])
            out.append(_finish_result(model, r))
        return out
    finally:
        engine.bnpcs_destroy()


def chain_seeds(seed, n):
    """MCMC.run (MCMC.py:100-104): the chains' seeds as the reference draws them from --seed"""
    if seed > 0:
        np.random.seed(seed)
    return np.random.randint(0, 2 ** 32 - 1, n)
