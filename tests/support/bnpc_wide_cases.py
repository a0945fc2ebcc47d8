"""BnpC past 256 cells: the cases of tests/test_bnpc_wide_cpu.py and tests/test_bnpc_wide_gpu.py, and the numpy twin's answer to each.

Every per-chain kernel of csrc/bnpc_sampler.hip is one workgroup of 256 lanes, and once N, hi + 1 (the largest live id + 2) or K (the live
clusters) passes 256 a lane owns a run of ids in place of one; the estimate (csrc/bnpc.hip) has a bitmap of 2048 words, a prefix over 256
lanes and 64 x 64 pair tiles.  The cases here are the smallest that cross each of these widths.  The twin (longsom_amd.bnpc_sampler,
bnpc._Host) is run once per case and process (lru_cache) and its answer is shared, unchanged, by the CPU file, which asserts the conditions
a case must meet to test anything (a decision of the twin not within 1e-9 of its edge, a cluster born, a width crossed), and the GPU
file, which holds the device to it."""
import functools

import numpy as np

from longsom_amd import bnpc, bnpc_sampler as bs
from tests.test_bnpc_gpu import generated
from tests.test_bnpc_sampler_gpu import random_data, state_of

# ---- one sweep from a loaded state (step 1) ----------------------------------------------------------------------------------------------
SWEEP_CASES = ("singletons257", "random300", "gaps513", "singletons600")
SWEEP_SEEDS = (1, 2, 3, 4)
SWEEP_STEP = 1


def sweep_case(name):
    """(model, seed -> start state)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "singletons257":                                       # hi + 1 = 258: two slots per lane from the first cell on; K = 257 columns of LL
        model = bs.Model(random_data(rng, 257, 65), 0.1, 0.01)
        return model, lambda seed: state_of(np.random.default_rng(seed), model, np.arange(257))
    if name == "random300":                                           # hi + 1 passes 256 inside the sweep
        model = bs.Model(random_data(rng, 300, 130), 0.1, 0.01, (0.25, 0.25))
        return model, lambda seed: bs.initial_state(model, seed)
    if name == "gaps513":                                             # three slots per lane, most of them free ids; the last id is live
        model = bs.Model(random_data(rng, 513, 33), 0.1, 0.01)
        ids = np.sort(np.append(rng.permutation(512)[:39], 512))
        labels = ids[np.concatenate([np.arange(40), rng.integers(0, 40, 513 - 40)])]
        return model, lambda seed: state_of(np.random.default_rng(seed), model, labels)
    if name == "singletons600":
        data = random_data(rng, 600, 10)
        data[599] = np.nan                                            # an all-missing cell
        model = bs.Model(data, 0.1, 0.01, (0.25, 0.25), (0.001, 5.0))
        return model, lambda seed: state_of(np.random.default_rng(seed), model, np.arange(600))
    raise KeyError(name)


def copy_state(st):
    return bs.State(st.labels, st.theta, st.alpha)


@functools.lru_cache(maxsize=None)
def swept(name):
    """(model, [per seed: dict(start, end, margin, errors)]): the twin's sweep and concentration update of every chain"""
    model, start = sweep_case(name)
    chains = []
    for seed in SWEEP_SEEDS:
        st = start(seed)
        first = copy_state(st)
        margin = bs.Margin()
        errors = bs.gibbs_sweep(model, st, seed, SWEEP_STEP, margin)
        bs.alpha_update(model, st, seed, SWEEP_STEP, margin)
        chains.append({"seed": seed, "start": first, "end": st, "margin": margin, "errors": errors})
    return model, chains


def hi_of(st):
    """what k_bnpcs_live leaves in hi: the largest live id + 1"""
    return int(st.live()[-1]) + 1


# ---- counts and the likelihood matrix ------------------------------------------------------------------------------------------------------
COUNT_SHAPES = [(257, 257), (300, 3), (513, 40), (600, 300)]
COUNT_M = (1, 65, 130)


def count_case(N, K, M):
    """test_counts_and_likelihood_matrix's construction: ids with gaps, an all-missing cell and an all-missing column"""
    rng = np.random.default_rng(N * 1000 + K * 10 + M)
    data = random_data(rng, N, M)
    data[N - 1] = np.nan
    if M > 1:
        data[:, M // 2] = np.nan
    model = bs.Model(data, 0.1, 0.01)
    ids = np.sort(rng.permutation(N)[:K])
    labels = ids[np.concatenate([np.arange(K), rng.integers(0, K, N - K)])]
    return model, ids, state_of(rng, model, labels)


# ---- one parameter move from a loaded state (step 4) ------------------------------------------------------------------------------------------
MOVE_N = 300
MOVE_K = (257, 300)
MOVE_M = (1, 65, 200)
MOVE_PP = ((1, 1), (0.25, 0.25))
MOVE_SEEDS = (5, 6)
MOVE_STEP = 4


@functools.lru_cache(maxsize=None)
def moved(K, M, pp):
    """test_one_parameter_move_equals_twin's construction at N = 300: (model, ids, labels, [per seed: dict(start, end, margin)])"""
    N = MOVE_N
    rng = np.random.default_rng(K * 1000 + M)
    data = random_data(rng, N, M)
    if M > 1:
        data[:, M - 1] = np.nan                                       # a column with n1 = n0 = 0 in every cluster
    model = bs.Model(data, 0.1, 0.01, pp)
    ids = np.sort(rng.permutation(N)[:K])
    labels = ids[np.concatenate([np.arange(K), rng.integers(min(1, K - 1), K, N - K)])]
    chains = []
    for seed in MOVE_SEEDS:
        st = state_of(np.random.default_rng(seed), model, labels)
        st.theta[ids[0], 0] = bs.TMIN32
        first = copy_state(st)
        margin = bs.Margin()
        bs.parameter_move(model, st, seed, MOVE_STEP, margin)
        chains.append({"seed": seed, "start": first, "end": st, "margin": margin})
    return model, ids, labels, chains


# ---- a short run whose K crosses 256 ------------------------------------------------------------------------------------------------------------
RUN_SEED, RUN_STEPS, RUN_BURN_IN, RUN_FN, RUN_FP = 4, 8, 3, 0.1, 0.01
RUN_KW = dict(pp=(0.25, 0.25), dpa=(2.0, 0.5), dpa_prob=0.25)
RUN_SMALL_ARENA = 300


@functools.lru_cache(maxsize=None)
def run_data():
    return random_data(np.random.default_rng(300), 300, 33)


@functools.lru_cache(maxsize=None)
def run_host():
    return bs.run_chains_host(run_data(), [RUN_SEED], RUN_STEPS, RUN_BURN_IN, RUN_FN, RUN_FP, **RUN_KW)[0]


# ---- the posterior estimate ----------------------------------------------------------------------------------------------------------------------
ESTIMATE_SHAPES = [(257, 3, 200), (2049, 5, 6), (2100, 3, 1500), (4133, 2, 3000)]
ESTIMATE_WIDE = [(2100, 3, 1500), (4133, 2, 3000)]                    # more than 1 024 distinct labels per sample, labels >= 2048


@functools.lru_cache(maxsize=None)
def estimated(N, S, K):
    """test_codist_and_mpear_against_twin's inputs and the twin's answers: a, p, D, cuts, the three MPEAR sums, and per final assignment
    (the first sample's own clusters, a random one with a one-cell cluster) the mean parameters, the branches and n_used"""
    a, p = generated(N * 1000 + S, N, S, K)
    host = bnpc._Host(a, p)
    D = host.codist()
    rng = np.random.default_rng(S)
    cuts = np.stack([rng.integers(0, 1 + k % N, N) for k in range(7)])
    sums = host.mpear_sums(cuts)
    random = rng.integers(0, K, N)
    random[0] = K
    finals = [(final, host.mean_params(final)) for final in (a[0], random)]
    return {"a": a, "p": p, "D": D, "cuts": cuts, "sums": sums, "finals": finals}
