"""BnpC's sampler (scripts/CellClustering/libs/CRP.py:17-410, libs/CRP_learning_errors.py, libs/MCMC.py:200-388): Gibbs assignment
sweeps, the non-conjugate split-merge move (CRP.py:417-820), the Escobar-West concentration update, the parameter Metropolis-Hastings
and the Metropolis-Hastings updates of the error rates, all chains of a run at once; --fixed_assignment is a start state and a flag;
--steps, --lugsail and --runtime are three stop rules over the same chains.  --single_chains is not here.

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
  Purposes    see P_* below.  `sub` carries a cell or a cluster id (< 65536); under the P_SM* purposes a scan number t (0 .. sm_steps, below
              2^22) or a row r (0 = the i side, 1 = the j side, 2 = the merged cluster), and where both are needed 4 t + r: 24 bits hold it.
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
THE STEP (Chain.do_step, MCMC.py:320-337), step s >= 1.  (u0, u1) = the doubles of block (0, s, P_SM, 0): if u0 < sm_prob the step makes the
split-merge move below in place of the sweep (with sm_prob = 0 no step does, and no draw of any other purpose moves); alpha, move and
record follow either one.
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
THE SPLIT-MERGE MOVE (update_assignments_split_merge, do_split_move, do_merge_move, run_rg_nc and what they call, CRP.py:417-820).
  Blocks of (0, s, P_SM, a): a = 0 (u0, u1) above; a = 1 (c0, c1) choose the clusters; a = 2 (a0, a1) choose the anchors; a = 3 its first
  double v decides the move.  With K live clusters: K = 1 forces a split, K = N a merge, else a split iff u1 < r0 / (r0 + r1) (choice(p=ratios)).
  split   the cluster: the first of the clusters with at least two cells, ascending, whose running share of their sizes exceeds c0.  The
          anchors: with n cells in it, ascending, i the floor(a0 n)-th and j the floor(a1 (n - 1))-th of the others.  size_data:
          log(size / N) - log size - log(size - 1), with the UNRESTRICTED size / N although one-cell clusters cannot be chosen (:454-456).
  merge   the clusters: i the first live one whose running share of the inverse sizes exceeds c0, j the same with c1 over the others.  The
          anchors: the floor(a0 n_i)-th cell of i, the floor(a1 n_j)-th of j.  size_data: log p_i + log p_j - log n_i - log n_j (:505-507).
  S       the other cells of the move in ascending id; n = |S| + 2.
  launch  _rg_init_split runs for BOTH moves, so a merge does not start from the original partition either: a cell of S goes to j iff
          ll_j > ll_i, its likelihood under "parameters" that are the anchor's own data with mix[0] for a missing entry.  Such a theta is
          0, 1 or mix[0]: six log constants times popcounts of mask intersections, added in the order (anchor 1, 0, missing) x (cell 1, 0).
          The rows r = 0, 1, 2 (the i side with i, the j side with j, all cells): theta[m] ~ Beta(p + n1, q + n0) of the row's cells' counts,
          block (m, s, P_SM_BETA | r << 8, .), clipped, float32.
  scan t  (t = 0 .. sm_steps - 1) _rg_scan_assign if S is not empty: the likelihoods of all cells of S under rows 0 and 1 are taken ONCE;
          the cells are walked in the order of ascending (64-bit draw of block (cell, s, P_SM_PERM | t << 8, 0), cell); the walked cell leaves,
          n_j = 1 + the others on the j side, n_i = n - n_j - 1, log_post = ll + log_CRP_prior([n_i, n_j], n, alpha) with the move's n and
          not N, normalised by _normalize_log (not _normalize_log_probs: no clip; its FloatingPointError fallback is [0, log EPSILON]), and
          choice([0, 1], p=exp(.)) with u the first double of block (cell, s, P_SM_CHOICE | t << 8, 0).  Then MH_cluster_params on rows 0 and 1
          with their cells' counts after the walk, and on row 2: (u, v) of block (m, s, P_SM_MH | (4 t + r) << 8, 0), sd by w0 % 3 of attempt 1.
  split   scan t = sm_steps of rows 0, 1 with trans_prob: the walk returns the sum of the chosen log probabilities (0 if S is empty);
          MH_cluster_params(trans_prob=True) clips A at 0 and a declined entry contributes log(-expm1(A)).  Then _get_log_A(parameters[the
          cluster], row 2, clip=True) summed, with fresh sds (w0 % 3 of block (m, s, P_SM_SD | 2 << 8, 0)).  A = (that - the scan's) +
          _get_lprior_ratio_split + _get_ll_ratio + _get_ltrans_prob_size_ratio_split, added in this order.  Refused when S is not empty
          and all of it ended on one side (np.unique(.).size == 1; an empty S has size 0 and is not refused); else accepted iff ln v < A.
          An accepted split leaves row 0 to the cluster and gives the j side the smallest free id with row 1.
  merge   scan t = sm_steps of row 2 with trans_prob.  _rg_get_split_prob: fresh sds for rows 0, 1 (P_SM_SD | r << 8); _get_log_A(parameters
          [cluster of the anchor], row r, clip=True) whose forward bounds are (0 - theta) / sd and (1 - theta) / sd, NOT TMIN / TMAX (the
          reverse bounds are), over the LAUNCH state's members of the side, not the original cluster's; then the walk in S's own order with
          the original clusters' parameters, which overwrites the assignment with the original one as it goes.  A = (that - the scan's) +
          _get_lprior_ratio_merge + _get_ll_ratio + _get_ltrans_prob_size_ratio_merge in this order; the second and third read the (now
          original) assignment together with the launch state's rows 0, 1.  log(|S| - 1) raises under MCMC.py:20's np.seterr for |S| of 0
          or 1, and the term falls back to -log N.  Accepted iff ln v < A: the cluster of i takes row 2 and the cells of j's.
  Where this differs from the reference in distribution only (never in the target): the cluster to split is drawn once from the clusters
  with two cells or more (the re-draw loop's own distribution); the anchors are a uniform ordered pair of distinct cells (what the
  acceptance ratio's - log n - log(n - 1) assumes; the reference's two swaps, :448-450, do not give it when obs_j_idx == 0); S is listed
  in ascending id; the merge pair is two sequential draws without replacement; the permutation is a rank by Philox keys.
THE ERROR-RATE UPDATE (CRP_errors_learning.update_error_rates / MH_error_rates, CRP_learning_errors.py:52-111; Chain.do_step, MCMC.py:339-342).
  State     per chain FP, FN (doubles).  They start at the prior means; the priors are truncnorm((0 - m) / sd, (1 - m) / sd, m, sd) for
            (FP_mean, FP_sd) and (FN_mean, FN_sd); the proposal sds of a rate are (0.5 sd, sd, 1.5 sd) of ITS prior sd (:26, :32).
  When      after the parameter move and before the record (MCMC.py:335-342), only when learning is on.  (u0, _) = the doubles of block
            (0, s, P_ERR, 0): if u0 < error_prob, the FP move and then the FN move, which sees the FP move's result (:52-55).
  A move    of rate e under purpose P_e (P_ERR_FP, P_ERR_FN): (u, v) = the doubles of block (0, s, P_e, 0); std = sds[w0 % 3] with w0 of block
            (0, s, P_e, 1); a = (0 - old) / std, b = (1 - old) / std, all in double; new = old + std ndtri(ndtr(a) + u (ndtr(b) - ndtr(a))).
            new_p_target: the log density of new under the normal(old, std) truncated to [0, 1]; old_p_target: that of old under the
            normal(new, std) truncated to [0, 1]; both, and the prior's log density, in the form -z^2 / 2 - log(2 pi) / 2 - log std -
            log(ndtr(b) - ndtr(a)).  A = new_ll + new_prior - old_ll - old_prior + old_p_target - new_p_target, added in this order (:106);
            accepted iff ln v < A.
  ll        get_ll_full_error(FP, FN) (:58-63) is the nansum over cells x mutations of log(par (1 - FN)^d FN^(1 - d) + (1 - par)(1 - FP)^(1 - d)
            FP^d): L1 for d = 1, L0 for d = 0 of log_tables, so it equals sum_k sum_m n1[k][m] L1'[k][m] + n0[k][m] L0'[k][m] over the live
            clusters with the tables taken under the trial rates: K x M terms from the counts.  old_ll is the likelihood under the current
            rates; after an accepted FP move it is that move's new_ll.
  After     an accepted move the chain's derived constants change (1 - FN, 1 - FP, the new cluster's two log terms, the six anchor logs) and
            its L1 / L0: the next sweep, split-merge move and parameter move of THAT chain read the new ones.
  record    FN[s], FP[s] per step (MCMC.py:256-257); MAP[s] gains FP_prior.logpdf(FP[s]) + FN_prior.logpdf(FN[s]) (get_lprior_full, :47-49),
            added on the host over all steps at once with scipy, as the concentration's term.  error_moves: FP accepted, declined, FN
            accepted, declined.
  Where this differs from the reference in distribution only: a `new` that rounding put at <= 0 or >= 1 is declined and counted in
  variate_errors (the reference would raise there under MCMC.py:20's np.seterr).
A FIXED ASSIGNMENT (CRP.init(assign=...), :121-128, :169-175; Chain.do_step with fix_assign, MCMC.py:321-333).  The labels are the file's, read
as dpmmIO.load_txt reads them (:101-112) and compacted to 0 .. K-1 in ascending order; theta[k][m] = clip(Beta(p + n1[k][m], q + n0[k][m])),
float32, of block (m, 0, P_INIT_ASSIGN | k << 8, .).  A step makes neither the sweep, nor the split-merge move, nor the concentration
update, and consumes no draw of theirs: only the parameter move and the error update run.  All chains start from the same labels and
differ by their seeds.
THE STOP RULES (dpmmIO._get_mcmc_termination, dpmmIO.py:158-169; MCMC.run, MCMC.py:79-123).  A chain's draws are a function of (seed, step,
purpose) alone, so a chain that is extended IS the longer chain: nothing below changes what any step does.
  steps     `steps` steps, the first `burn_in` of which keep no parameters.
  Lugsail   run_lugsail_chains (MCMC.py:138-177).  A first run of max(10, int(1 / (cutoff^2 - 1))) steps that keeps every step's parameters,
            step 0 included; then, with steps_run the records so far: PSRF = get_lugsail_batch_means_est over ML[steps_run // 2:] of every
            chain (utils.py:427-467; lugsail_psrf here, lsg_bnpcs_psrf on the device); (steps_run, PSRF) joins the result's "PSRF" list; at or
            below the cutoff the run ends, else the chains go on for `extend` (200) steps.  At the end burn_in = steps_run // 2 + 1, params =
            params[burn_in:] and "PSRF_cutoff" = cutoff.  An extension that is refused for room ends the run with an error.
            Where this differs from the reference: MCMC.extend_chain (:180-188) re-seeds numpy with the chain's seed before every extension,
            so its chains replay the random numbers of their start every 200 steps; these do not.
  Runtime   Chain_time (MCMC.py:395-440).  Steps in batches; the clock is read before each batch; no batch starts after `end`; the first step
            of the first batch that starts at or after `burn_in_end` is the first kept one, and step 0 never is; burn_in = the records minus
            the kept ones.  Where this differs from the reference: the chains run in lockstep, so all have the same length (the reference's
            run in processes of their own and end with different lengths), and the clock is read per batch, not per step.
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
P_SM, P_SM_PERM, P_SM_CHOICE, P_SM_BETA, P_SM_BETA_B, P_SM_MH, P_SM_SD = range(12, 19)
P_ERR, P_ERR_FP, P_ERR_FN, P_INIT_ASSIGN, P_INIT_ASSIGN_B = range(19, 24)
ERROR_SD_FACTORS = (0.5, 1.0, 1.5)                # CRP_learning_errors.py:26,32
SM_SWEEP, SM_SPLIT_DECLINED, SM_SPLIT_ACCEPTED, SM_MERGE_DECLINED, SM_MERGE_ACCEPTED = range(5)      # the codes of sm_moves
MAX_SM_STEPS = 1 << 20

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


def truncnorm_logpdf(x32, loc32, sd, lo32=None, hi32=None):
    """log density at x of the normal(loc, sd) truncated to [TMIN, TMAX], or to [lo, hi] where given"""
    if lo32 is None:
        pa, pb = truncnorm_mass(loc32, sd)
    else:
        from scipy.special import ndtr
        pa, pb = ndtr(_f32diff(np.float32(lo32), loc32) / sd), ndtr(_f32diff(np.float32(hi32), loc32) / sd)
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

    def __init__(self, data, FN, FP, pp=(1, 1), dpa=(-1, -1), dpa_prob=0.5, error_prior=None, error_prob=0.0, error_priors=None):
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
        # the error-rate update: its probability and (FP_mean, FP_sd, FN_mean, FN_sd); a chain whose rates move works on a copy (of_chain)
        self.error_prob = float(error_prob)
        self.error_priors = None if error_priors is None else tuple(float(x) for x in error_priors)
        self.learning = self.error_priors is not None and self.error_prob > 0

    def of_chain(self, FP=None, FN=None):
        """the model of one chain: the same data, rates of its own (error_update writes them)"""
        import copy
        m = copy.copy(self)
        if FP is not None:
            m.FP, m.FN = float(FP), float(FN)
        return m

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
    """one chain: labels [N], sizes [N] (0 = a free id), theta [N][M] float32 (row = cluster id), alpha, and the error rates FP, FN
    (None: the model's)"""

    def __init__(self, labels, theta, alpha, FP=None, FN=None):
        self.labels = np.array(labels, dtype=np.int64)
        self.theta = np.array(theta, dtype=np.float32)
        self.alpha = float(alpha)
        self.FP, self.FN = (None, None) if FP is None else (float(FP), float(FN))
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


def load_assignment(path):
    """dpmmIO.load_txt (:101-112): the first row's 'Assignment' of a tab-separated table, or a file of numbers separated by blanks"""
    import pandas as pd
    try:
        x = pd.read_csv(path, sep="\t", index_col=False).at[0, "Assignment"].split(" ")
    except (ValueError, KeyError, AttributeError):
        with open(path) as f:
            x = f.read().split(" ")
    return [int(v) for v in x]


def assigned_state(model, seed, assign):
    """CRP.init(assign=...) (:121-128) with _init_cl_params('assign') (:169-175)"""
    assign = np.asarray(assign)
    if assign.ndim != 1 or len(assign) != model.N:
        raise ValueError("the fixed assignment has %d labels, the data have %d cells" % (assign.size, model.N))
    labels = np.unique(assign, return_inverse=True)[1].reshape(-1)
    K = int(labels.max()) + 1
    st = State(labels, np.zeros((model.N, model.M), np.float32), model.alpha0)
    n1, n0 = counts(model, st)
    b, _ = beta_variate(seed, model.p + n1[:K], model.q + n0[:K], np.arange(model.M)[None, :], 0, P_INIT_ASSIGN, np.arange(K)[:, None])
    st.theta[:K] = np.clip(b, TMIN, TMAX).astype(np.float32)
    return st


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


def log_A(model, new32, old32, n1, n0, sd, terms=False, clip=False, unit_bounds=False):
    """_get_log_A (:347-383) from the cluster's counts.  unit_bounds: the forward density's bounds are (0 - old) / sd and (1 - old) / sd, as
    _rg_get_split_prob (:779-780) passes them; the reverse bounds stay TMIN / TMAX"""
    nL1, nL0 = log_tables(new32, model.FN, model.FP)
    oL1, oL0 = log_tables(old32, model.FN, model.FP)
    new_ll, old_ll = n1 * nL1 + n0 * nL0, n1 * oL1 + n0 * oL0
    new_prior = old_prior = 0
    if not model.uniform:
        new_prior, old_prior = beta_logpdf(new32, model.p, model.q), beta_logpdf(old32, model.p, model.q)
    new_p = truncnorm_logpdf(new32, old32, sd, 0.0, 1.0) if unit_bounds else truncnorm_logpdf(new32, old32, sd)
    old_p = truncnorm_logpdf(old32, new32, sd)
    A = new_ll + new_prior - old_ll - old_prior + old_p - new_p
    if clip:
        A = np.minimum(A, 0.0)
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


# ---- the split-merge move (CRP.py:417-820).  The functions take their draws as arguments: the run feeds them the Philox stream, the
# CPU tests the reference's own replayed draws. --------------------------------------------------------------------------------------
def anchor_logs(model):
    """the six values log(theta B_FN(x) + (1 - theta) B_FP(x)) can take when theta is an anchor's data with mix[0] for a missing entry
    (_rg_init_split, :557-560): [anchor 1, 0, missing][cell 1, 0]"""
    FN, FP, m0 = model.FN, model.FP, model.mix[0]
    return np.log(np.array([[1 - FN, FN], [FP, 1 - FP], [m0 * (1 - FN) + (1 - m0) * FP, m0 * FN + (1 - m0) * (1 - FP)]]))


def sm_anchor_ll(model, S, anchor):
    """_calc_ll(data[S], nan_to_num(data[anchor], nan=mix[0])): popcounts of mask intersections times the six constants, added in a fixed order"""
    S = np.asarray(S, dtype=np.int64)
    consts = anchor_logs(model)
    sides = (model.one[anchor], model.zero[anchor], ~(model.one[anchor] | model.zero[anchor]))
    ll = np.zeros(len(S)); mag = np.zeros(len(S)); cnt = np.zeros((len(S), 6), np.int64)
    for a, mask in enumerate(sides):
        for x, cells in enumerate((model.one, model.zero)):
            n = (cells[S] & mask).sum(axis=1)
            cnt[:, 2 * a + x] = n
            ll = ll + n * consts[a, x]
            mag = mag + n * abs(consts[a, x])
    return ll, mag, cnt


def sm_launch_assign(model, i, j, S, margin=None):
    """_rg_init_split's assignment (:551-561): 1 where the j anchor's data explain the cell better"""
    ll_i, mag_i, cnt_i = sm_anchor_ll(model, S, i)
    ll_j, mag_j, cnt_j = sm_anchor_ll(model, S, j)
    if margin is not None:
        differ = (cnt_i != cnt_j).any(axis=1)                         # equal counts give equal sums wherever they are added
        margin.see(((ll_j - ll_i) / np.maximum(1.0, mag_i + mag_j))[differ])
    return np.where(ll_j > ll_i, 1, 0).astype(np.int64)


def sm_row_counts(model, i, j, S, assign):
    """n1, n0 [3][M] of the rows' cells: S where assign is 0 and i, S where it is 1 and j, all of them"""
    S = np.asarray(S, dtype=np.int64)
    n1 = np.zeros((3, model.M), np.int64); n0 = np.zeros((3, model.M), np.int64)
    for r, cells in enumerate((np.append(S[assign == 0], i), np.append(S[assign == 1], j))):
        n1[r], n0[r] = model.one[cells].sum(axis=0), model.zero[cells].sum(axis=0)
    n1[2], n0[2] = n1[0] + n1[1], n0[0] + n0[1]
    return n1, n0


def sm_cell_ll(model, S, rows32):
    """_rg_get_ll (:635-638): [|S|][2], and the sums of the terms' magnitudes"""
    S = np.asarray(S, dtype=np.int64)
    L1, L0 = log_tables(rows32, model.FN, model.FP)
    return model.one_f[S] @ L1.T + model.zero_f[S] @ L0.T, model.one_f[S] @ np.abs(L1).T + model.zero_f[S] @ np.abs(L0).T


def normalize_log(probs):
    """_normalize_log (:104-116)"""
    max_i = int(np.argmax(probs))
    try:
        with np.errstate(divide="raise", over="ignore", under="ignore", invalid="raise"):
            return probs - probs[max_i] - np.log1p(np.sum(np.exp(np.delete(probs, max_i) - probs[max_i])))
    except FloatingPointError:
        return np.array([0, LOG_EPSILON]) if probs[0] > probs[1] else np.array([LOG_EPSILON, 0])


def sm_scan_assign(ll, assign, n, alpha, order, us=None, fixed=None, margin=None):
    """_rg_scan_assign (:609-632) with trans_prob over `order` (positions in S) with the uniforms us [|S|]; with `fixed` the walk of
    _rg_get_split_prob (:803-818), which assigns fixed[.] instead of drawing.  `assign` is changed in place.  Returns (the sum of the chosen
    log probabilities, the sum of their magnitudes)."""
    lden = np.log(n - 1 + alpha)
    prob = np.zeros(len(assign))
    on_j = int(assign.sum())
    for s in order:
        others = on_j - int(assign[s])
        n_j = others + 1                                              # nansum(rg_assignment) + 2 with -1 in the cell's place
        n_i = n - n_j - 1
        lp = normalize_log(ll[s] + (np.log(np.array([n_i, n_j], dtype=np.float64)) - lden))
        if fixed is None:
            p = np.exp(lp)
            cdf = np.cumsum(p)
            cdf /= cdf[-1]
            new = 0 if cdf[0] > us[s] else 1
            if margin is not None:
                margin.see(cdf[0] - us[s])
        else:
            new = int(fixed[s])
        assign[s] = new
        on_j = others + new
        prob[s] = lp[new]
    return float(prob.sum()), float(np.abs(prob).sum())


def sm_param_move(model, old32, new32, n1, n0, sd, lv, margin=None):
    """MH_cluster_params(trans_prob=True) (:314-342) of one row after its proposal: A clipped at 0, declined iff ln v >= A, a declined
    entry contributes log(-expm1(A)).  Returns (the row, the sum, the sum of magnitudes: an entry's own and those of A's terms, which a
    declined entry's log(-expm1(.)) passes on times its slope 1 / expm1(-A))."""
    A, mag = log_A(model, new32, old32, n1, n0, sd, terms=True)
    A = np.minimum(A, 0.0)
    decline = lv >= A
    if margin is not None:
        margin.see((lv - A) / np.maximum(1.0, np.abs(A)))
    with np.errstate(all="ignore"):
        T = np.where(decline, np.log(-np.expm1(np.where(decline, A, -1.0))), A)
        slope = np.where(decline, 1.0 / np.expm1(-np.where(decline, A, -1.0)), 1.0)
    return np.where(decline, old32, new32).astype(np.float32), float(T.sum()), float((np.abs(T) + mag * np.maximum(1.0, slope)).sum())


def sm_lprior_ratio(model, move, n, n_j, alpha, rows32, theta_orig):
    """_get_lprior_ratio_split (:695-713) / _merge (:736-754): rows32 are rows 0, 1 for a split and row 2 for a merge; theta_orig the
    parameters of the original cluster(s)"""
    from scipy.special import gammaln
    n_i = n - n_j
    sign = 1.0 if move == "split" else -1.0
    r = sign * (np.log(alpha) - gammaln(n))
    if n_i > 0:
        r += sign * gammaln(n_j)
    if n_j > 0:
        r += sign * gammaln(n_i)
    mag = abs(np.log(alpha)) + abs(gammaln(n)) + abs(gammaln(n_j)) + abs(gammaln(n_i))
    if not model.uniform:
        a, b = beta_logpdf(rows32, model.p, model.q), beta_logpdf(theta_orig, model.p, model.q)
        r += float(np.sum(a)) - float(np.sum(b))
        mag += float(np.abs(a).sum() + np.abs(b).sum())
    return float(r), float(mag)


def sm_ll_ratio(model, move, n1, n0, rows32):
    """_get_ll_ratio (:716-733) from the three rows' counts"""
    L1, L0 = log_tables(rows32, model.FN, model.FP)
    t = n1 * L1 + n0 * L0
    ll = t.sum(axis=1)
    r = ll[0] + ll[1] - ll[2] if move == "split" else ll[2] - ll[0] - ll[1]
    return float(r), float(np.abs(t).sum())


def sm_size_ratio_split(ltrans_prob_size, other_sizes, n, n_j):
    """_get_ltrans_prob_size_ratio_split (:757-764)"""
    n_i = n - n_j
    norm = np.sum(1 / np.append(np.asarray(other_sizes, dtype=np.float64), [n_i, n_j]))
    return float(np.log(1 / n_i / norm) + np.log(1 / n_j / norm) - ltrans_prob_size)


def sm_size_ratio_merge(size_data, N, n_S):
    """_get_ltrans_prob_size_ratio_merge (:767-774): log(|S| - 1) raises for |S| of 0 or 1 and the term falls back"""
    rev = -np.log(N) - np.log(n_S - 1) if n_S > 1 else -np.log(N)
    return float(rev - size_data)


def sm_split_size_data(sizes, live, cl):
    """do_split_move's ltrans_prob_size (:454-456): the unrestricted share of the cluster"""
    size = int(sizes[cl])
    return float(np.log(size / float(sizes[live].sum())) - np.log(size) - np.log(size - 1))


def sm_merge_size_data(sizes, live, cl_i, cl_j):
    """do_merge_move's cluster_size_data (:505-507); the inverse sizes are added in the order of the ids"""
    inv = 1 / sizes[live].astype(np.float64)
    total = np.cumsum(inv)[-1]
    return float((np.log(1 / float(sizes[cl_i]) / total) + np.log(1 / float(sizes[cl_j]) / total)) - (np.log(float(sizes[cl_i])) + np.log(float(sizes[cl_j]))))


def sm_choose_split(sizes, live, c0):
    """the cluster to split: the first of those with two cells or more whose running share of their sizes exceeds c0"""
    cand = live[sizes[live] >= 2]
    cdf = np.cumsum(sizes[cand]).astype(np.float64) / float(sizes[cand].sum())
    return int(cand[min(int(np.searchsorted(cdf, c0, side="right")), len(cand) - 1)])


def sm_choose_merge(sizes, live, c0, c1):
    """the clusters to merge: two sequential draws without replacement from the inverse sizes"""
    inv = 1 / sizes[live].astype(np.float64)
    cdf = np.cumsum(inv)
    ji = min(int(np.searchsorted(cdf / cdf[-1], c0, side="right")), len(live) - 1)
    rest = np.delete(np.arange(len(live)), ji)
    cdf2 = np.cumsum(inv[rest])
    jj = int(rest[min(int(np.searchsorted(cdf2 / cdf2[-1], c1, side="right")), len(rest) - 1)])
    return int(live[ji]), int(live[jj])


def sm_apply(st, move, cl_i, cl_j, j, S, assign, rows32):
    """an accepted move on the state (:465-477, :513-520): rows32 are rows 0, 1 for a split (cl_j the free id) and row 2 for a merge"""
    if move == "split":
        st.theta[cl_i], st.theta[cl_j] = rows32[0], rows32[1]
        st.labels[np.append(np.asarray(S, dtype=np.int64)[np.asarray(assign) == 1], j)] = cl_j
    else:
        st.theta[cl_i] = rows32
        st.labels[st.labels == cl_j] = cl_i
    st.sizes[:] = np.bincount(st.labels, minlength=len(st.labels))


def _sm_mh_draws(seed, step, M, scan, row):
    m = np.arange(M)
    sub = 4 * scan + row
    u, v = doubles(seed, m, step, P_SM_MH, 0, sub)
    w = philox(seed, m, step, np.uint64(P_SM_MH) | (np.uint64(sub) << np.uint64(8)), 1)
    return u, np.log(v), PROPOSAL_SD[w[0] % np.uint32(3)]


def _sm_fresh_sd(seed, step, M, row):
    w = philox(seed, np.arange(M), step, np.uint64(P_SM_SD) | (np.uint64(row) << np.uint64(8)), 0)
    return PROPOSAL_SD[w[0] % np.uint32(3)]


def split_merge_move(model, st, seed, step, ratios=(0.75, 0.25), scans=3, margin=None):
    """update_assignments_split_merge (:417-431) on the state, under the stream.  Returns the outcome: code (as in sm_moves), clusters
    (i, j: for a split j is the smallest free id), anchors, A, terms [4], mags [4] (the sums of magnitudes behind the terms), counts [4]
    (their numbers of terms), lv (ln v), errors."""
    N, M = model.N, model.M
    live = st.live()
    K = len(live)
    _, u_kind = doubles(seed, 0, step, P_SM, 0)
    c0, c1 = doubles(seed, 0, step, P_SM, 1)
    a0, a1 = doubles(seed, 0, step, P_SM, 2)
    v, _ = doubles(seed, 0, step, P_SM, 3)
    lv = float(np.log(v))
    if K == 1:
        split = True
    elif K == N:
        split = False
    else:
        edge = ratios[0] / (ratios[0] + ratios[1])
        split = bool(u_kind < edge)
        if margin is not None:
            margin.see(float(u_kind) - edge)
    if split:
        cl_i = sm_choose_split(st.sizes, live, float(c0))
        size_data = sm_split_size_data(st.sizes, live, cl_i)
        cl_j = int(np.nonzero(st.sizes == 0)[0][0])                   # get_empty_cluster, should the split be accepted
        cells = np.nonzero(st.labels == cl_i)[0]
        n = len(cells)
        ii = min(int(float(a0) * n), n - 1)
        jj = min(int(float(a1) * (n - 1)), n - 2)
        jj += jj >= ii
        i, j = int(cells[ii]), int(cells[jj])
        orig_rows = st.theta[[cl_i]]
    else:
        cl_i, cl_j = sm_choose_merge(st.sizes, live, float(c0), float(c1))
        size_data = sm_merge_size_data(st.sizes, live, cl_i, cl_j)
        cells_i, cells_j = np.nonzero(st.labels == cl_i)[0], np.nonzero(st.labels == cl_j)[0]
        i = int(cells_i[min(int(float(a0) * len(cells_i)), len(cells_i) - 1)])
        j = int(cells_j[min(int(float(a1) * len(cells_j)), len(cells_j) - 1)])
        cells = np.sort(np.concatenate([cells_i, cells_j]))
        n = len(cells)
        orig_rows = st.theta[[cl_i, cl_j]]
    S = cells[(cells != i) & (cells != j)]
    n_S = len(S)
    # run_rg_nc (:527-544): the launch state
    assign = sm_launch_assign(model, i, j, S, margin)
    n1, n0 = sm_row_counts(model, i, j, S, assign)
    b, errors = beta_variate(seed, model.p + n1, model.q + n0, np.arange(M)[None, :], step, P_SM_BETA, np.arange(3)[:, None], margin)
    rows = np.clip(b, TMIN, TMAX).astype(np.float32)

    def scan_assign(t):
        if n_S == 0:
            return 0.0, 0.0                                           # _rg_scan_split (:571-572)
        w = philox(seed, S, step, np.uint64(P_SM_PERM) | (np.uint64(t) << np.uint64(8)), 0)
        order = np.lexsort((S, w[1].astype(np.uint64) << _S32 | w[0].astype(np.uint64)))
        us, _ = doubles(seed, S, step, P_SM_CHOICE, 0, t)
        ll, _ = sm_cell_ll(model, S, rows[:2])
        return sm_scan_assign(ll, assign, n, st.alpha, order, us, None, margin)

    def move_row(t, r, n1, n0):
        u, lvs, sd = _sm_mh_draws(seed, step, M, t, r)
        rows[r], total, mag = sm_param_move(model, rows[r], truncnorm_variate(u, rows[r], sd), n1[r], n0[r], sd, lvs, margin)
        return total, mag

    for t in range(scans):
        scan_assign(t)
        n1, n0 = sm_row_counts(model, i, j, S, assign)
        for r in range(3):
            move_row(t, r, n1, n0)
    terms, mags, counts = np.zeros(4), np.zeros(4), np.zeros(4, np.int64)
    per_row = 2 * n * M + 6 * M                                       # what one row's M values of A are sums of, at most
    if split:
        # _do_rg_split_MH (:641-653), _get_trans_prob_ratio_split (:668-682)
        prob_cl, mag_cl = scan_assign(scans)
        n1, n0 = sm_row_counts(model, i, j, S, assign)
        (p0, m0), (p1, m1) = move_row(scans, 0, n1, n0), move_row(scans, 1, n1, n0)
        GS_split = prob_cl + (p0 + p1)
        sd = _sm_fresh_sd(seed, step, M, 2)
        A_rev, mag_rev = log_A(model, orig_rows[0], rows[2], n1[2], n0[2], sd, terms=True, clip=True)
        terms[0], mags[0], counts[0] = float(A_rev.sum()) - GS_split, mag_cl + m0 + m1 + float(mag_rev.sum()), n_S + 3 * per_row
        n_j = int(assign.sum()) + 1
        terms[1], mags[1] = sm_lprior_ratio(model, "split", n, n_j, st.alpha, rows[:2], orig_rows)
        terms[2], mags[2] = sm_ll_ratio(model, "split", n1, n0, rows)
        terms[3] = sm_size_ratio_split(size_data, np.delete(st.sizes[live], np.searchsorted(live, cl_i)), n, n_j)
        refused = n_S > 0 and len(np.unique(assign)) == 1
    else:
        # _do_rg_merge_MH (:656-665), _get_trans_prob_ratio_merge (:685-692), _rg_get_split_prob (:777-820)
        GS_merge, mag_m = move_row(scans, 2, n1, n0)
        GS_split, mag_s = 0.0, 0.0
        for r in range(2):
            sd = _sm_fresh_sd(seed, step, M, r)
            A_r, mag_r = log_A(model, orig_rows[r], rows[r], n1[r], n0[r], sd, terms=True, clip=True, unit_bounds=True)
            GS_split += float(A_r.sum()); mag_s += float(mag_r.sum())
        original = (st.labels[S] == cl_j).astype(np.int64)
        if n_S:
            ll, _ = sm_cell_ll(model, S, orig_rows)
            pa, mag_a = sm_scan_assign(ll, assign, n, st.alpha, np.arange(n_S), None, original, None)
            GS_split += pa; mag_s += mag_a
        terms[0], mags[0], counts[0] = GS_split - GS_merge, mag_m + mag_s, n_S + 3 * per_row
        n1, n0 = sm_row_counts(model, i, j, S, assign)                # the original clusters' cells by now
        n_j = int(assign.sum()) + 1
        terms[1], mags[1] = sm_lprior_ratio(model, "merge", n, n_j, st.alpha, rows[2], orig_rows)
        terms[2], mags[2] = sm_ll_ratio(model, "merge", n1, n0, rows)
        terms[3] = sm_size_ratio_merge(size_data, N, n_S)
        refused = False
    counts[1], counts[2], counts[3] = 4 + 3 * M, 6 * M, 8
    mags[3] = abs(terms[3]) + 4 * np.log(N) + abs(size_data)
    A = ((terms[0] + terms[1]) + terms[2]) + terms[3]
    accept = not refused and lv < A
    if split:
        code = SM_SPLIT_ACCEPTED if accept else SM_SPLIT_DECLINED
    else:
        code = SM_MERGE_ACCEPTED if accept else SM_MERGE_DECLINED
    if accept:
        sm_apply(st, "split" if split else "merge", cl_i, cl_j, j, S, assign, rows[:2] if split else rows[2])
    return {"code": code, "clusters": (cl_i, cl_j), "anchors": (i, j), "A": float(A), "terms": terms, "mags": mags, "counts": counts, "lv": lv,
            "refused": bool(refused), "errors": int(errors)}


def sm_bound_of_A(out):
    """the bound on |A - A'| between two evaluations of the move's acceptance ratio: (n + 4) 2^-52 sum |term| per term"""
    return float(np.sum((out["counts"] + 4) * 2.0 ** -52 * out["mags"]))


def takes_split_merge(seed, step, sm_prob):
    """Chain.do_step's first draw (MCMC.py:322)"""
    return bool(sm_prob > 0 and float(doubles(seed, 0, step, P_SM, 0)[0]) < sm_prob)


# ---- the error-rate update (CRP_learning_errors.py:47-111) ----------------------------------------------------------------------------
def unit_truncnorm_logpdf(x, loc, sd):
    """log density at x of the normal(loc, sd) truncated to [0, 1], all in double"""
    from scipy.special import ndtr
    pa, pb = ndtr((0.0 - loc) / sd), ndtr((1.0 - loc) / sd)
    z = (np.asarray(x, dtype=np.float64) - loc) / sd
    return -0.5 * z * z - 0.5 * np.log(2.0 * np.pi) - np.log(sd) - np.log(pb - pa)


def error_ll(model, st, FP, FN):
    """get_ll_full_error (:58-63) from the counts of the live clusters: (the sum, the sum of the terms' magnitudes)"""
    live = st.live()
    n1, n0 = counts(model, st)
    L1, L0 = log_tables(st.theta[live], FN, FP)
    terms = np.concatenate([(n1[live] * L1).ravel(), (n0[live] * L0).ravel()])
    return float(terms.sum()), float(np.abs(terms).sum())


def error_log_A(model, st, rate, new, sd):
    """the terms of MH_error_rates' A (:86-106) for the proposal `new` of `rate` ('FP' or 'FN') made with the proposal sd `sd`, from the
    state's current rates"""
    e = 0 if rate == "FP" else 1
    FP, FN = (model.FP, model.FN) if st.FP is None else (st.FP, st.FN)
    old = (FP, FN)[e]
    mean, psd = model.error_priors[2 * e], model.error_priors[2 * e + 1]
    new_ll, new_mag = error_ll(model, st, new if e == 0 else FP, FN if e == 0 else new)
    old_ll, old_mag = error_ll(model, st, FP, FN)
    new_prior, old_prior = float(unit_truncnorm_logpdf(new, mean, psd)), float(unit_truncnorm_logpdf(old, mean, psd))
    new_p, old_p = float(unit_truncnorm_logpdf(new, old, sd)), float(unit_truncnorm_logpdf(old, new, sd))
    A = new_ll + new_prior - old_ll - old_prior + old_p - new_p
    return {"new": float(new), "old": float(old), "new_ll": new_ll, "old_ll": old_ll, "ll_mag": (new_mag, old_mag), "new_prior": new_prior, "old_prior": old_prior,
            "prior": new_prior - old_prior, "new_p": new_p, "old_p": old_p, "A": float(A)}


def error_bound_of_A(model, out):
    """the bound on |A - A'| between two evaluations of A: (n + 4) 2^-52 sum |term| for each likelihood (n: the observed entries), and a few
    ulp of the six scalar terms, each of which is itself a sum of four"""
    n_obs = int(model.pop1.sum() + model.pop0.sum())
    scalars = abs(out["new_prior"]) + abs(out["old_prior"]) + abs(out["new_p"]) + abs(out["old_p"])
    return float((n_obs + 4) * 2.0 ** -52 * (out["ll_mag"][0] + out["ll_mag"][1]) + 64 * 2.0 ** -52 * (scalars + 40.0))


def error_update(model, st, seed, step, margin=None):
    """Chain.do_step's draw (MCMC.py:339) and update_error_rates (:52-55) on the state; the model is the chain's own (Model.of_chain): its
    rates follow the state's.  Returns None where the draw says no update, else {'FP': ..., 'FN': ...}: error_log_A's terms with pick (the
    sd's index), lv (ln v) and code (1 accepted, 0 declined, -1 declined because rounding put the proposal on an end).  margin sees the
    draw's distance from error_prob."""
    from scipy.special import ndtr, ndtri
    if st.FP is None:
        st.FP, st.FN = model.FP, model.FN
    u0, _ = doubles(seed, 0, step, P_ERR)
    if margin is not None:
        margin.see(float(u0) - model.error_prob)
    if not float(u0) < model.error_prob:
        return None
    out = {}
    for e, (rate, purpose) in enumerate((("FP", P_ERR_FP), ("FN", P_ERR_FN))):
        u, v = doubles(seed, 0, step, purpose)
        pick = int(philox(seed, 0, step, purpose, 1)[0] % np.uint32(3))
        psd = model.error_priors[2 * e + 1]
        sd = (psd * 0.5, psd, psd * 1.5)[pick]
        old = (st.FP, st.FN)[e]
        pa, pb = ndtr((0.0 - old) / sd), ndtr((1.0 - old) / sd)
        new = float(old + sd * ndtri(pa + float(u) * (pb - pa)))
        inside = 0.0 < new < 1.0
        o = error_log_A(model, st, rate, new if inside else old, sd)
        o.update(new=new, pick=pick, lv=float(np.log(v)))
        accept = inside and o["lv"] < o["A"]
        o["code"] = 1 if accept else 0 if inside else -1
        if accept:
            if e == 0:
                st.FP = new
            else:
                st.FN = new
            model.FP, model.FN = st.FP, st.FN
        out[rate] = o
    return out


def error_prior_logpdf(model, FP, FN):
    """FP_prior.logpdf(FP) + FN_prior.logpdf(FN) (get_lprior_full, CRP_learning_errors.py:47-49) with scipy, over arrays"""
    from scipy.stats import truncnorm
    fm, fs, nm, ns = model.error_priors
    return truncnorm((0 - fm) / fs, (1 - fm) / fs, fm, fs).logpdf(np.asarray(FP, dtype=np.float64)) + truncnorm((0 - nm) / ns, (1 - nm) / ns, nm, ns).logpdf(np.asarray(FN, dtype=np.float64))


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
            "assignments": np.zeros((n, model.N), dtype=int), "burn_in": burn_in, "_crp": np.zeros(n), "_beta": np.zeros(n), "_rows": [],
            "sm_moves": np.zeros(n, np.int8), "error_moves": np.zeros(4, np.int64)}


def _finish_result(model, r):
    """MAP from its parts (the scalar prior logpdfs with scipy, over all steps at once) and the parameter blocks padded to one cluster count.
    The error rates' own terms: the priors' log densities at the recorded rates where they are learned, else the run's one number."""
    error_prior = error_prior_logpdf(model, r["FP"], r["FN"]) if model.learning else model.error_prior
    r["MAP"] = r["ML"] + alpha_logpdf(model, r["DP_alpha"]) + r.pop("_crp") + r.pop("_beta") + error_prior
    rows = r.pop("_rows")
    k_max = max(b.shape[0] for b in rows)
    params = np.zeros((len(rows), k_max, model.M), np.float32)
    for s, b in enumerate(rows):
        params[s, :b.shape[0]] = b
    r["params"] = params
    return r


# ---- the stop rules: run_BnpC.py's -s, -ls and -r (dpmmIO._get_mcmc_termination, dpmmIO.py:158-169) ---------------------------------------
_NEVER = 2 ** 31 - 1                                                  # the first kept step of a run that keeps none yet


class Lugsail:
    """--lugsail: run until the lugsail batch-means PSRF of the chains' ML, over the second half of their records, is at most `cutoff`
    (MCMC.run, MCMC.py:85-90; run_lugsail_chains, :138-177).  The first run has max(10, int(1 / (cutoff^2 - 1))) steps; after every check
    above the cutoff the chains go on for `extend` steps.  report(steps_run, psrf) is called at every check."""

    def __init__(self, cutoff, extend=200, report=None):
        cutoff, extend = float(cutoff), int(extend)
        if not cutoff > 1:
            raise ValueError("lugsail cutoff %r: it must be above 1 (the first run has int(1 / (cutoff^2 - 1)) steps, which 1 divides by zero)" % (cutoff,))
        if extend < 1:
            raise ValueError("lugsail extend must be at least 1, got %d" % extend)
        self.cutoff, self.extend, self.report = cutoff, extend, report
        self.first_steps = max(10, int(1 / (cutoff ** 2 - 1)))


class Runtime:
    """--runtime: steps in batches of `batch` until clock() passes `end`; the clock is read before each batch, no batch starts after `end`,
    and the first step of the first batch that starts at or after `burn_in_end` is the first kept one (Chain_time, MCMC.py:395-440, which
    reads the clock before each step).  clock() returns what compares with end and burn_in_end: datetimes, or numbers."""

    def __init__(self, end, burn_in_end, clock, batch=50):
        if int(batch) < 1:
            raise ValueError("runtime batch must be at least 1, got %r" % (batch,))
        self.end, self.burn_in_end, self.clock, self.batch = end, burn_in_end, clock, int(batch)


def ml_stats(series, first, last=None):
    """n, the mean, the sample variance (ddof 1), tau(b) and tau(b // 3) of series[first:last] (get_tau_lugsail, utils.py:464-467; b =
    int(n ** 0.5)): what lsg_bnpcs_psrf returns per chain.  The sums are of x - x[first], in two passes."""
    x = np.asarray(series, dtype=np.float64)[first:last]
    n = x.size
    if n < 1:
        return np.zeros(5)
    pivot = x[0]
    x = x - pivot
    mean = x.sum() / n
    var = float(np.square(x - mean).sum() / (n - 1)) if n > 1 else 0.0
    taus = [0.0, 0.0]
    if n >= 9:
        b = int(n ** 0.5)
        for k, size in enumerate((b, b // 3)):
            a = n // size
            taus[k] = size / (a - 1) * float(np.square(x[:a * size].reshape(a, size).sum(axis=1) / size - mean).sum())
    return np.array([n, pivot + mean, var, taus[0], taus[1]])


def psrf_of_stats(stats):
    """get_lugsail_batch_means_est (utils.py:427-461) from the chains' five statistics [C][5] (ml_stats, lsg_bnpcs_psrf): inf where a chain
    has fewer than 9 values, and where the reference's FloatingPointError is (MCMC.py:20's np.seterr: a mean variance of 0, a negative
    quotient under the root)"""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 5)
    if (stats[:, 0] < 9).any():
        return np.inf
    T_L = np.mean(2 * stats[:, 3] - stats[:, 4])
    s = np.mean(stats[:, 2])
    n = np.round(np.mean(stats[:, 0]))
    sigma_L = ((n - 1) * s + T_L) / n
    if s == 0 or not sigma_L / s >= 0:
        return np.inf
    return float(np.sqrt(sigma_L / s))


def lugsail_psrf(chains):
    """utils.get_lugsail_batch_means_est of chains = [(series, burn_in), ...]"""
    return psrf_of_stats([ml_stats(series, burn_in) for series, burn_in in chains])


def _check_run(steps, burn_in, sm_prob=0.0, sm_ratios=(0.75, 0.25), sm_steps=3, stop=None):
    if stop is not None and not isinstance(stop, (Lugsail, Runtime)):
        raise ValueError("stop must be None (steps and burn_in hold), a Lugsail or a Runtime, got %r" % (stop,))
    if stop is None and (steps < 1 or not 0 <= burn_in <= steps):
        raise ValueError("steps must be at least 1 and burn_in within [0, steps], got %d and %d" % (steps, burn_in))
    if not 0 <= sm_prob <= 1 or len(sm_ratios) != 2 or min(sm_ratios) <= 0 or abs(sum(sm_ratios) - 1) > 1e-9 or not 0 <= sm_steps <= MAX_SM_STEPS:
        raise ValueError("sm_prob must lie in [0, 1], sm_ratios be two positive numbers that sum to 1 and sm_steps be in [0, %d], got %r, %r and %r"
                         % (MAX_SM_STEPS, sm_prob, tuple(sm_ratios), sm_steps))


def _error_model(data, FN, FP, pp, dpa, dpa_prob, error_prior, error_prob, error_priors):
    """the run's model; where the error rates are learned (error_prob > 0) the four numbers of their priors are needed, and the rates start
    at the priors' means, which FP and FN must then be"""
    if not 0 <= error_prob <= 1:
        raise ValueError("error_prob must lie in [0, 1], got %r" % (error_prob,))
    if error_prob > 0:
        if error_priors is None or len(error_priors) != 4 or not all(0 < float(x) < 1 for x in error_priors):
            raise ValueError("error_prob %g needs error_priors = (FP_mean, FP_sd, FN_mean, FN_sd), each inside (0, 1), got %r" % (error_prob, error_priors))
        if float(FP) != float(error_priors[0]) or float(FN) != float(error_priors[2]):
            raise ValueError("the learned error rates start at their priors' means: FP %r and FN %r were given, the means are %r and %r"
                             % (FP, FN, error_priors[0], error_priors[2]))
    return Model(data, FN, FP, pp, dpa, dpa_prob, error_prior, error_prob, error_priors if error_prob > 0 else None)


def _start_states(model, seeds, states, fixed_assignment):
    if fixed_assignment is not None:
        if states is not None:
            raise ValueError("give either states or fixed_assignment")
        return [assigned_state(model, s, fixed_assignment) for s in seeds]
    return [initial_state(model, s) for s in seeds] if states is None else states


def run_chains_host(data, seeds, steps, burn_in, FN, FP, pp=(1, 1), dpa=(-1, -1), dpa_prob=0.5, error_prior=None, states=None,
                    sm_prob=0.0, sm_ratios=(0.75, 0.25), sm_steps=3, error_prob=0.0, error_priors=None, fixed_assignment=None, stop=None):
    """The whole sampler in numpy.  seeds: one 64-bit seed per chain.  states: start there instead of at the random initialisation.
    stop: None (the run has `steps` steps, the first `burn_in` of which keep no parameters), a Lugsail or a Runtime, under which steps and
    burn_in are not read (pass None): see THE STOP RULES above.
    sm_prob, sm_ratios, sm_steps: run_BnpC.py's -smp, -smr, -sms; the result's sm_moves [steps + 1] says what each step did.
    error_prob, error_priors: -eup and (-FP_m, -FP_sd, -FN_m, -FN_sd): the result's FP / FN are then the rates of each step and error_moves
    the moves' counts (FP accepted, declined, FN accepted, declined).  fixed_assignment: -fa's labels [N]; the steps keep them."""
    _check_run(steps, burn_in, sm_prob, sm_ratios, sm_steps, stop)
    shared = _error_model(data, FN, FP, pp, dpa, dpa_prob, error_prior, error_prob, error_priors)
    run = _HostRun(shared, seeds, _start_states(shared, seeds, states, fixed_assignment), sm_prob, sm_ratios, sm_steps, fixed_assignment is not None)
    return _drive(run, steps, burn_in, stop)


class _HostRun:
    """the chains of run_chains_host under _drive: open(steps), advance(n, keep_from), stats(first), extend(add), results(burn_in)"""

    _PER_STEP = ("ML", "MAP", "DP_alpha", "FN", "FP", "assignments", "_crp", "_beta", "sm_moves")      # a result's records that hold a row per step

    def __init__(self, shared, seeds, start, sm_prob, sm_ratios, sm_steps, fixed):
        self.sm, self.fixed, self.done = (sm_prob, sm_ratios, sm_steps), fixed, 0
        self.chains = []
        for seed, s0 in zip(seeds, start):
            st = State(s0.labels, s0.theta, s0.alpha, s0.FP, s0.FN)
            self.chains.append({"seed": seed, "st": st, "model": shared.of_chain(st.FP, st.FN), "errors": 0})

    def open(self, steps):
        for ch in self.chains:
            ch["r"] = _empty_result(ch["model"], steps, 0)

    def extend(self, add):
        for ch in self.chains:
            r, more = ch["r"], _empty_result(ch["model"], add - 1, 0)
            for k in self._PER_STEP:
                r[k] = np.concatenate([r[k], more[k]])

    def advance(self, n, keep_from):
        sm_prob, sm_ratios, sm_steps = self.sm
        for ch in self.chains:
            seed, st, model, r = ch["seed"], ch["st"], ch["model"], ch["r"]
            errors = 0
            for s in range(self.done, self.done + n):
                if s:
                    if not self.fixed:
                        if takes_split_merge(seed, s, sm_prob):
                            move = split_merge_move(model, st, seed, s, sm_ratios, sm_steps)
                            errors += move["errors"]
                            r["sm_moves"][s] = move["code"]
                        else:
                            errors += gibbs_sweep(model, st, seed, s)
                        errors += alpha_update(model, st, seed, s)
                    parameter_move(model, st, seed, s)
                    if model.learning:
                        move = error_update(model, st, seed, s)
                        if move is not None:
                            for e, rate in enumerate(("FP", "FN")):
                                r["error_moves"][2 * e + (0 if move[rate]["code"] == 1 else 1)] += 1
                                errors += move[rate]["code"] == -1
                live = st.live()
                r["ML"][s] = likelihood(model, st.labels, st.theta[live])[0]
                r["_crp"][s], r["_beta"][s] = prior_parts(model, st)
                r["DP_alpha"][s] = st.alpha
                r["FP"][s], r["FN"][s] = model.FP, model.FN
                r["assignments"][s] = st.labels
                if s >= keep_from:
                    r["_rows"].append(st.theta[live].copy())
            ch["errors"] += int(errors)
        self.done += n

    def stats(self, first):
        return np.array([ml_stats(ch["r"]["ML"], first, self.done) for ch in self.chains])

    def results(self, burn_in):
        out = []
        for ch in self.chains:
            r = ch["r"]
            for k in self._PER_STEP:
                r[k] = r[k][:self.done]
            r["burn_in"], r["variate_errors"] = burn_in, ch["errors"]
            out.append(_finish_result(ch["model"], r))
        return out


class _DeviceRun:
    """the chains of run_chains under _drive.  The arena is emptied when it is full and at the end; a convergence check moves five numbers
    per chain to the host (engine.bnpcs_psrf)."""

    def __init__(self, engine, model, seeds, start, arena_rows, sm_prob, sm_ratios, sm_steps, fixed):
        self.engine, self.model, self.seeds, self.start, self.arena_rows = engine, model, seeds, start, arena_rows
        self.sm, self.fixed, self.done, self.taken, self.keep_from = (sm_prob, sm_ratios, sm_steps), fixed, 0, 0, _NEVER
        self.rows = [[] for _ in seeds]

    def open(self, steps):
        engine, model = self.engine, self.model
        sm_prob, sm_ratios, sm_steps = self.sm
        engine.bnpcs_create(model, self.seeds, steps, self.arena_rows)
        if sm_prob > 0:
            engine.bnpcs_set_split_merge(sm_prob, sm_ratios[0], sm_ratios[1], sm_steps)
        if model.learning:
            engine.bnpcs_set_error_learning(model.error_prob, *model.error_priors)
        if self.fixed:
            engine.bnpcs_set_fixed_assignment(True)
        for c, st in enumerate(self.start):
            engine.bnpcs_set_state(c, st.labels, st.theta, st.alpha)
            if st.FP is not None:
                engine.bnpcs_set_error_rates(c, st.FP, st.FN)

    def extend(self, add):
        self.engine.bnpcs_extend(add)

    def advance(self, n, keep_from):
        target = self.done + n
        self.keep_from = keep_from
        while self.done < target:
            self.done += self.engine.bnpcs_run(self.done, target - self.done, keep_from)
            if self.done < target:
                self._take()                                          # the arena is full

    def _take(self):
        """the records so far, and the parameter rows of the steps kept since the arena was last emptied"""
        labels, scalars, arena = self.engine.bnpcs_fetch()
        for c in range(len(self.seeds)):
            at = 0
            for s in range(max(self.taken, self.keep_from), self.done):
                k = int(scalars[c, s, 3])
                self.rows[c].append(arena[c, at:at + k].copy())
                at += k
        self.taken = self.done
        return labels, scalars

    def stats(self, first):
        return self.engine.bnpcs_psrf([first] * len(self.seeds), self.done)

    def results(self, burn_in):
        engine, model, n = self.engine, self.model, self.done
        labels, scalars = self._take()
        errors = engine.bnpcs_errors()
        moves = engine.bnpcs_fetch_moves() if self.sm[0] > 0 else None
        rates, rate_moves = engine.bnpcs_fetch_error_rates() if model.learning or any(st.FP is not None for st in self.start) else (None, None)
        out = []
        for c in range(len(self.seeds)):
            r = _empty_result(model, n - 1, burn_in)
            r["ML"], r["_crp"], r["_beta"], r["DP_alpha"] = scalars[c, :n, 0].copy(), scalars[c, :n, 1].copy(), scalars[c, :n, 2].copy(), scalars[c, :n, 4].copy()
            if model.uniform:
                r["_beta"][:] = 0.0
            r["assignments"] = labels[c, :n].astype(int)
            r["_rows"] = self.rows[c]
            r["variate_errors"] = int(errors[c])
            if moves is not None:
                r["sm_moves"] = moves[c, :n].copy()
            if rates is not None:
                r["FP"], r["FN"], r["error_moves"] = rates[c, :n, 0].copy(), rates[c, :n, 1].copy(), rate_moves[c].astype(np.int64)
            out.append(_finish_result(model, r))
        return out


def _drive(run, steps, burn_in, stop):
    """the three stop rules over a run (_HostRun, _DeviceRun)"""
    if stop is None:
        run.open(steps)
        run.advance(steps + 1, burn_in)
        return run.results(burn_in)
    if isinstance(stop, Lugsail):
        # MCMC.run (MCMC.py:85-90): the first run keeps every step's parameters; run_lugsail_chains (:138-177)
        run.open(stop.first_steps)
        run.advance(stop.first_steps + 1, 0)
        checks = []
        while True:
            steps_run = run.done
            psrf = psrf_of_stats(run.stats(steps_run // 2))
            checks.append((steps_run, psrf))
            if stop.report is not None:
                stop.report(steps_run, psrf)
            if psrf <= stop.cutoff:
                break
            try:
                run.extend(stop.extend)
            except (RuntimeError, MemoryError) as e:
                raise RuntimeError("the chains have not converged and cannot go on: after %d steps the PSRF is %.5f, above the cutoff %g, and %d more "
                                   "steps were refused: %s" % (steps_run, psrf, stop.cutoff, stop.extend, e)) from e
            run.advance(stop.extend, 0)
        burn_in = steps_run // 2 + 1
        out = run.results(burn_in)
        for r in out:
            r["params"] = r["params"][burn_in:]
            r["PSRF"], r["PSRF_cutoff"] = list(checks), stop.cutoff
        return out
    # Chain_time (MCMC.py:395-440), the chains in lockstep: the clock is read before each batch
    room = stop.batch
    run.open(room)
    run.advance(1, _NEVER)                                            # step 0 is never kept (update_results(0), :404)
    keep_from = _NEVER
    while True:
        now = stop.clock()
        if now > stop.end:
            break
        if keep_from == _NEVER and not now < stop.burn_in_end:
            keep_from = run.done
        if run.done + stop.batch > room + 1:
            add = max(stop.batch, room)                               # room doubles, so that the records are moved a logarithmic number of times
            try:
                run.extend(add)
            except (RuntimeError, MemoryError):
                add = run.done + stop.batch - room - 1
                run.extend(add)
            room += add
        run.advance(stop.batch, keep_from)
    if keep_from == _NEVER:
        raise ValueError("the runtime ended before the burn-in did: no step of %d is kept, so there is nothing to estimate from" % (run.done - 1))
    return run.results(keep_from)


def run_chains(engine, data, seeds, steps, burn_in, FN, FP, pp=(1, 1), dpa=(-1, -1), dpa_prob=0.5, error_prior=None, states=None, arena_rows=0,
               sm_prob=0.0, sm_ratios=(0.75, 0.25), sm_steps=3, error_prob=0.0, error_priors=None, fixed_assignment=None, stop=None):
    """The same on the device, all chains in every kernel.  arena_rows: the parameter rows per chain the device holds between two fetches
    (0: enough for 64 kept steps of 64 clusters, at least N rows); a full arena only costs a fetch."""
    _check_run(steps, burn_in, sm_prob, sm_ratios, sm_steps, stop)
    model = _error_model(data, FN, FP, pp, dpa, dpa_prob, error_prior, error_prob, error_priors)
    seeds = [int(s) for s in seeds]
    start = _start_states(model, seeds, states, fixed_assignment)
    run = _DeviceRun(engine, model, seeds, start, int(arena_rows) or max(model.N, 4096), sm_prob, sm_ratios, sm_steps, fixed_assignment is not None)
    try:
        return _drive(run, steps, burn_in, stop)
    finally:
        engine.bnpcs_destroy()


def chain_seeds(seed, n):
    """MCMC.run (MCMC.py:100-104): the chains' seeds as the reference draws them from --seed"""
    if seed > 0:
        np.random.seed(seed)
    return np.random.randint(0, 2 ** 32 - 1, n)
