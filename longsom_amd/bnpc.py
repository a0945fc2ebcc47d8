"""BnpC's posterior estimate (scripts/CellClustering/libs/utils.py:90-245) and the three files it ends in (libs/dpmmIO.py:464-521).

BnpC has two halves.  The sampler (libs/CRP.py, libs/MCMC.py) is stochastic: the reference's own, or longsom_amd.bnpc_sampler's on the
device, feeds this module its chains.  The posterior estimate is deterministic: the co-clustering distance of every cell pair over every posterior
sample, a ward tree over it, the MPEAR score of every candidate cut, and the mean parameters of the chosen clusters.  The three passes
over big index spaces run on the device (csrc/bnpc.hip, lsg_bnpc_*), and so do the ward tree, its cuts and the cluster count that sets the
cut range (csrc/bnpc_linkage.hip), bit for bit scipy's linkage and cut_tree; linkage="scipy" keeps those two on the host, as in the reference.

posterior_estimate        the estimate on the device
posterior_estimate_host   its twin in numpy: what the CPU tests pin to the reference's goldens, and the GPU tests compare against
ward_linkage_host, cut_tree_host   numpy twins of scipy's linkage(y, "ward") and cut_tree: what the device's tree and cuts compute
concat_chains, save_chains, load_chains, save_assignments, save_geno, save_errors
"""
import os

import numpy as np

EPSILON = np.finfo(np.float64).resolution          # utils.py:16

_CHAIN_KEYS = ("assignments", "params", "DP_alpha", "FN", "FP", "ML", "MAP")


# ---- chains --------------------------------------------------------------------------------------------------------------------
def concat_chains(results):
    """_concat_chain_results (utils.py:206-223): the chains' samples after burn-in, one after the other; the parameter blocks padded with
    zero rows to the largest cluster count.  params are stored from the first step after burn-in (MCMC.py:260-282) and taken whole."""
    out = {k: np.concatenate([r[k][r["burn_in"]:] for r in results]) for k in ("assignments", "DP_alpha", "ML", "MAP", "FN", "FP")}
    params = [r["params"] for r in results]
    cl_max = np.max([p.shape[1] for p in params])
    out["params"] = np.concatenate([np.pad(p, [(0, 0), (0, cl_max - p.shape[1]), (0, 0)]) for p in params])
    out["burn_in"] = 0
    return out


def save_chains(path, results):
    """One .npz for a run: per chain i the arrays chain<i>_assignments, _params, _DP_alpha, _FN, _FP, _ML, _MAP and chain<i>_burn_in"""
    arrays = {"n_chains": np.int64(len(results))}
    for i, r in enumerate(results):
        for k in _CHAIN_KEYS:
            arrays["chain%d_%s" % (i, k)] = np.asarray(r[k])
        arrays["chain%d_burn_in" % i] = np.int64(r["burn_in"])
    with open(path, "wb") as f:
        np.savez_compressed(f, **arrays)


def load_chains(path):
    with np.load(path) as z:
        out = []
        for i in range(int(z["n_chains"])):
            r = {k: z["chain%d_%s" % (i, k)] for k in _CHAIN_KEYS}
            r["burn_in"] = int(z["chain%d_burn_in" % i])
            out.append(r)
    return out


# ---- the input matrix --------------------------------------------------------------------------------------------------------------
def load_data(in_file, transpose=True):
    """dpmmIO.load_data (dpmmIO.py:27-98) with get_names: the matrix as float (3 -> NaN, 2 -> 1), transposed by default, and its
    (row names, column names).  The separator is the most frequent of tab, comma and blank in the first line; a header row / an index
    column is present where the first line / the first elements of the next lines hold anything but 0, 1, 2, 3."""
    import pandas as pd
    lines = []
    with open(in_file, "r") as f:
        for _ in range(5):
            lines.append(f.readline().strip())
    if lines[0].count("\t") > lines[0].count(" ") and lines[0].count("\t") > lines[0].count(","):
        sep = "\t"
    elif lines[0].count(",") > lines[0].count(" "):
        sep = ","
    else:
        sep = " "

    def is_value(el):
        try:
            return float(el) in [0, 1, 2, 3]
        except ValueError:
            return None if el == " " else False          # a blank element is skipped

    header_row = False
    for el in lines[0].split(sep):
        if is_value(el) is False:
            header_row = True
            lines.pop(0)
            break
    index_col = any(is_value(line.split(sep)[0]) is False for line in lines)
    if index_col and header_row:
        df = pd.read_csv(in_file, sep=sep, index_col=0, header=0, na_values=[3, " ", "."]).astype(float)
    elif index_col:
        col_types = dict([(i, str) if i == 0 else (i, float) for i in range(len(lines[0].split(sep)))])
        df = pd.read_csv(in_file, sep=sep, index_col=0, header=None, dtype=col_types)
    elif header_row:
        df = pd.read_csv(in_file, sep=sep, index_col=None, header=0, dtype=float)
    else:
        df = pd.read_csv(in_file, sep=sep, index_col=None, header=None, dtype=float)
    if transpose:
        df = df.T
    df = df.replace(3, np.nan).replace(2, 1)
    return df.values, (df.index.values, df.columns.values)


def out_dir_of(output, in_file, stamp):
    """dpmmIO._get_out_dir (dpmmIO.py:172-192): -o names the directory (or a .txt / .gv / .csv file in it); without it, BnpC_<stamp> beside the
    input, numbered if it exists"""
    if output:
        out_dir = os.path.dirname(output) if any(output.endswith(e) for e in (".txt", ".gv", ".csv")) else output
    else:
        out_dir = raw = os.path.join(os.path.dirname(in_file), "BnpC_" + stamp)
        i = 1
        while os.path.exists(out_dir):
            out_dir = "%s_%d" % (raw, i)
            i += 1
    os.makedirs(out_dir, exist_ok=True)
    return out_dir


# ---- the two backends: the same five questions asked of numpy and of the device -------------------------------------------------------
def _check_samples(assignments, params):
    a = np.asarray(assignments)
    if a.ndim != 2:
        raise ValueError("assignments must be [samples, cells]")
    if a.shape[0] < 1 or a.shape[1] < 2:
        raise ValueError("the estimate needs at least 1 sample and 2 cells, got %d x %d" % a.shape)
    if a.min() < 0 or a.max() >= a.shape[1]:
        raise ValueError("a label lies outside [0, %d)" % a.shape[1])
    a = np.ascontiguousarray(a, dtype=np.int64)
    if params is not None:
        p32 = np.ascontiguousarray(params, dtype=np.float32)
        if p32.ndim != 3 or p32.shape[0] != a.shape[0]:
            raise ValueError("params must be [samples, clusters, mutations] with one block per sample")
        if np.asarray(params).dtype != np.float32 and not np.array_equal(p32, params):
            raise ValueError("params do not fit float32 (a chain run with --runtime extends them as float64): the estimate reads float32")
        params = p32
    return a, params


def _rank_map(chunk):
    """[n, N] -> per sample and label value, the number of distinct labels of the sample below it"""
    n, N = chunk.shape
    present = np.zeros((n, N), bool)
    present[np.arange(n)[:, None], chunk] = True
    return np.cumsum(present, axis=1, dtype=np.int32) - present


def _candidate_range(avg_cl_no, n_cells):
    n_range = cut_range(avg_cl_no, n_cells)
    if n_range.size == 0:
        raise ValueError("BnpC posterior estimate: no candidate cluster number (n_range is empty: on average %.3g clusters of more than 2 cells "
                         "over %d cells); the reference fails here in np.unique(None)" % (avg_cl_no, n_cells))
    return n_range


def _scipy_cuts(D, a):
    """(n_range, cuts [len(n_range), N]) as the reference makes them (utils.py:100-123): scipy's ward tree of D / S, cut once for the whole range"""
    from scipy.cluster.hierarchy import cut_tree, linkage
    S, N = a.shape
    Z = linkage(D / S, method="ward")                                # uint32 / int -> float64 true division, the bits of get_dist's int32 / int
    n_range = _candidate_range(avg_cluster_number(a), N)
    return n_range, np.ascontiguousarray(cut_tree(Z, n_clusters=list(n_range)).T)      # one call: its columns equal the per-n calls (utils.py:123)


class _Host:
    """numpy, no device.  Samples go through in chunks so that no temporary outgrows ~64 MB."""

    def __init__(self, assignments, params):
        self.a, self.params = assignments, params
        self.S, self.N = assignments.shape

    def _chunks(self, width):
        step = max(1, int(16_000_000 // max(width, 1)))
        for s0 in range(0, self.S, step):
            yield s0, min(self.S, s0 + step)

    def codist(self, fetch=True):
        i, j = np.triu_indices(self.N, 1)                    # row-major over i < j: pdist's condensed order
        d = np.zeros(len(i), np.uint32)
        for s0, s1 in self._chunks(len(i)):
            d += np.count_nonzero(self.a[s0:s1][:, i] != self.a[s0:s1][:, j], axis=0).astype(np.uint32)
        self.d = d
        return d

    def candidate_cuts(self):
        return _scipy_cuts(self.d, self.a)

    def mpear_sums(self, cuts):
        i, j = np.triu_indices(self.N, 1)
        sim = self.S - self.d.astype(np.int64)
        same = [cut[i] == cut[j] for cut in cuts]
        return (np.array([int(np.count_nonzero(m)) for m in same], np.uint64), np.array([int(sim[m].sum()) for m in same], np.uint64), int(self.d.astype(np.int64).sum()))

    def mean_params(self, final):
        if self.params is None:
            raise ValueError("the samples were given without parameters")
        clusters = np.unique(final)
        C, S, M = len(clusters), self.S, self.params.shape[2]
        cells = [np.nonzero(final == c)[0] for c in clusters]
        same = np.zeros((C, S), bool); alone = np.zeros((C, S), bool); rel = np.zeros((C, S), np.int64)
        for s0, s1 in self._chunks(self.N):
            chunk = self.a[s0:s1]
            n = s1 - s0
            rank = _rank_map(chunk)
            counts = np.bincount((chunk + np.arange(n)[:, None] * self.N).ravel(), minlength=n * self.N).reshape(n, self.N)
            for k, idx in enumerate(cells):
                L = chunk[:, idx[0]]
                same[k, s0:s1] = (chunk[:, idx] == L[:, None]).all(axis=1)
                alone[k, s0:s1] = counts[np.arange(n), L] == len(idx)
                rel[k, s0:s1] = rank[np.arange(n), L]
        if rel.max() >= self.params.shape[1]:
            raise ValueError("a sample has more distinct labels than the %d parameter rows" % self.params.shape[1])
        out = np.zeros((C, M)); branch = np.zeros(C, np.uint8); n_used = np.zeros(C, np.int32)
        for k, idx in enumerate(cells):
            both = same[k] & alone[k]
            if same[k].any():
                use = np.nonzero(both if both.any() else same[k])[0]
                branch[k] = 3 if len(idx) == 1 else 0 if both.any() else 1
                n_used[k] = len(use)
                for row in self.params[use, rel[k, use]]:            # one += per sample, ascending: the reference's loop (utils.py:177-180) bit for bit
                    out[k] += row
                out[k] /= use.size
            else:
                branch[k] = 2
                n_used[k] = S
                for s0, s1 in self._chunks(max(self.N, len(idx) * M)):
                    r = _rank_map(self.a[s0:s1])[np.arange(s1 - s0)[:, None], self.a[s0:s1][:, idx]]
                    if r.max() >= self.params.shape[1]:
                        raise ValueError("a sample has more distinct labels than the %d parameter rows" % self.params.shape[1])
                    out[k] += self.params[np.arange(s0, s1)[:, None], r].sum(axis=(0, 1), dtype=np.float64)
                out[k] /= S * idx.size
        return out, branch, n_used

    def close(self):
        pass


class _Device:
    """linkage "device": the tree, its cuts and the cluster count are the library's, and D leaves the device only where it is asked for;
    "scipy": D is fetched and those three are the host's, as in _Host"""

    def __init__(self, engine, assignments, params, linkage="device"):
        if linkage not in ("device", "scipy"):
            raise ValueError("linkage must be \"device\" or \"scipy\", got %r" % (linkage,))
        self.e, self.a, self.linkage = engine, assignments, linkage
        engine.bnpc_load_samples(assignments, params)

    def codist(self, fetch=True):
        self.d = self.e.bnpc_codist(fetch=fetch or self.linkage == "scipy")
        return self.d if fetch else None

    def candidate_cuts(self):
        if self.linkage == "scipy":
            return _scipy_cuts(self.d, self.a)
        n_range = _candidate_range(self.e.bnpc_avg_cluster_number(), self.a.shape[1])
        self.e.bnpc_linkage(fetch=False)
        return n_range, self.e.bnpc_cut_tree(n_range).astype(np.int64)

    def mpear_sums(self, cuts):
        return self.e.bnpc_mpear(cuts)

    def mean_params(self, final):
        return self.e.bnpc_mean_params(final)

    def close(self):
        self.e.bnpc_unload()


# ---- the ward tree and its cuts: numpy twins of scipy's linkage(y, "ward") and cut_tree, which lsg_bnpc_linkage / _cut_tree are held to ------
def _ward_chain(y, N):
    """The merges of scipy's nn_chain for method "ward" in the order the chain makes them: rows (x, y, height, size x + size y), x < y the
    two slots (y carries the union on).  What k_bnpc_ward computes."""
    W = np.full((N, N), np.inf)
    iu = np.triu_indices(N, 1)
    W[iu] = y
    W.T[iu] = y
    size = np.ones(N, np.int64)
    alive = np.ones(N, bool)
    chain, lowest = [], 0
    rec = np.zeros((N - 1, 4))
    scans, max_scans = 0, 3 * (N - 1)
    for k in range(N - 1):
        if not chain:
            while not alive[lowest]:
                lowest += 1
            chain.append(lowest)
        while True:
            if scans == max_scans:
                raise RuntimeError("ward linkage: the chain did not end in %d scans" % max_scans)
            scans += 1
            x = chain[-1]
            row = np.where(alive, W[x], np.inf)
            row[x] = np.inf
            j = int(np.argmin(row))
            below = chain[-2] if len(chain) > 1 else -1
            if below >= 0 and W[x, below] <= row[j]:
                j = below
            cur = W[x, j]
            if j == below:
                break
            chain.append(j)
        del chain[-2:]
        x, j = min(x, j), max(x, j)
        nx, ny = size[x], size[j]
        rec[k] = x, j, cur, nx + ny
        size[x], size[j] = 0, nx + ny
        alive[x] = False
        idx = alive.copy()
        idx[j] = False
        ni = size[idx]
        t = 1.0 / (nx + ny + ni)
        dx, dy = W[x, idx], W[j, idx]
        new = np.sqrt((ni + nx) * t * dx * dx + (ni + ny) * t * dy * dy - ni * t * cur * cur)
        W[j, idx] = new
        W[idx, j] = new
    return rec


def ward_linkage_host(dist, chain_sizes=False):
    """scipy.cluster.hierarchy.linkage(dist, "ward") of a condensed distance, bit for bit: the nearest-neighbour chain over a square working
    copy (a row scan is one argmin: the first minimum, and the element below the chain's top wins every tie), the records sorted stably
    by height, then named by a union-find whose sizes are those of the sorted order.  chain_sizes: also return the sizes the chain itself
    recorded, in the sorted order (they differ from Z[:, 3] where rounding puts a parent below its child)."""
    y = np.ascontiguousarray(dist, dtype=np.float64)
    N = int(round((1 + np.sqrt(1 + 8 * y.size)) / 2))
    if y.ndim != 1 or N < 2 or N * (N - 1) // 2 != y.size:
        raise ValueError("ward_linkage_host: %d values are no condensed distance matrix" % y.size)
    rec = _ward_chain(y, N)
    rec = rec[np.argsort(rec[:, 2], kind="stable")]
    Z = np.zeros((N - 1, 4))
    parent = np.arange(2 * N - 1)
    members = np.ones(2 * N - 1, np.int64)

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root
    for k in range(N - 1):
        a, b = find(int(rec[k, 0])), find(int(rec[k, 1]))
        parent[a] = parent[b] = N + k
        members[N + k] = members[a] + members[b]
        Z[k] = min(a, b), max(a, b), rec[k, 2], members[N + k]
    return (Z, rec[:, 3].copy()) if chain_sizes else Z


def cut_order(Z):
    """The order in which cut_tree applies a linkage matrix's nodes (row numbers): ascending height, nodes of equal height in the reverse
    of a breadth-first visit from the root that queues the right child before the left (bisect.insort_left over deque.popleft)."""
    N = Z.shape[0] + 1
    visit = np.zeros(N - 1, np.int64)
    queue, at = [2 * N - 2], 0
    while at < len(queue):
        node = queue[at]
        if node >= N:
            visit[node - N] = at
            queue += [int(Z[node - N, 1]), int(Z[node - N, 0])]
        at += 1
    return np.lexsort((-visit, Z[:, 2]))


def cut_tree_host(Z, ns):
    """scipy's cut_tree(Z, n_clusters=ns) as rows: labels [len(ns), N], row k the clustering after N - ns[k] nodes in cut_order; a cluster's
    label is its rank by its lowest leaf.  n = N is refused: scipy returns zeros for it unless it is the list's first entry."""
    Z = np.asarray(Z, dtype=np.float64)
    N = Z.shape[0] + 1
    ns = np.atleast_1d(np.asarray(ns, dtype=np.int64))
    if ns.size and (ns.min() < 1 or ns.max() > N - 1):
        raise ValueError("cut_tree_host: n_clusters must lie in 1 .. %d (cells - 1), got %d" % (N - 1, ns.min() if ns.min() < 1 else ns.max()))
    order = cut_order(Z)
    low = np.arange(2 * N - 1)                             # a node's lowest leaf names its cluster
    lab = np.arange(N)
    out = np.zeros((ns.size, N), np.int64)
    for step in range(N):
        for k in np.nonzero(N - ns == step)[0]:
            out[k] = np.unique(lab, return_inverse=True)[1]
        if step < N - 1:
            row = order[step]
            a, b = low[int(Z[row, 0])], low[int(Z[row, 1])]
            low[N + row] = min(a, b)
            lab[lab == max(a, b)] = min(a, b)
    return out


# ---- the estimate --------------------------------------------------------------------------------------------------------------
def avg_cluster_number(assignments):
    """utils.py:106-111: the mean over the samples of the number of clusters with more than 2 cells"""
    return np.mean(np.array([np.count_nonzero(np.bincount(a) > 2) for a in assignments], dtype=np.int64))


def cut_range(avg_cl_no, n_cells):
    """utils.py:113-114, verbatim: np.arange with float bounds and dtype=int has semantics of its own"""
    return np.arange(max(2, avg_cl_no * 0.2),
        min(avg_cl_no * 2.5, n_cells), dtype=int)


def mpear_scores(same_pairs, same_sim, dist_sum, n_samples, n_cells):
    """_calc_MPEAR (utils.py:132-143) from the three integer sums, in fp64"""
    from scipy.special import binom
    pairs = n_cells * (n_cells - 1) // 2
    I_sum = np.asarray(same_pairs, dtype=np.float64)
    pi_sum = (pairs * n_samples - int(dist_sum)) / n_samples
    index = np.asarray(same_sim, dtype=np.float64) / n_samples
    expected_index = (I_sum * pi_sum) / binom(n_cells, 2)
    max_index = .5 * (I_sum + pi_sum)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (index - expected_index) / (max_index - expected_index)


def _estimate(backend, a, data, dp_alpha, fn, fp, final_assignment, details):
    import pandas as pd
    S, N = a.shape
    info = {}
    try:
        if final_assignment is None:
            D = backend.codist(fetch=details)
            n_range, cuts = backend.candidate_cuts()
            same_pairs, same_sim, dist_sum = backend.mpear_sums(cuts)
            scores = mpear_scores(same_pairs, same_sim, dist_sum, S, N)
            best, best_score = None, -np.inf
            for k, score in enumerate(scores):                           # the first maximum (utils.py:125)
                if score > best_score:
                    best, best_score = k, score
            if best is None:
                raise ValueError("BnpC posterior estimate: no candidate cut has a score (all %d are NaN)" % len(scores))
            assign = cuts[best]
            if details:
                info.update(D=D, dist=D / S)
            info.update(n_range=n_range, cuts=cuts, same_pairs=same_pairs, same_sim=same_sim, dist_sum=dist_sum, scores=scores, n=int(n_range[best]))
        else:
            assign = np.asarray(final_assignment)
        params, branch, n_used = backend.mean_params(assign)
        info.update(params=params, branch=branch, n_used=n_used)
    finally:
        backend.close()
    geno = pd.DataFrame(params).T[assign]                                # utils.py:191
    rounded = geno.values.round()
    FN_geno = (((geno.T.values.round() == 1) & (data == 0)).sum() + EPSILON) / (rounded.sum() + EPSILON)              # utils.py:235-238
    FP_geno = (((geno.T.values.round() == 0) & (data == 1)).sum() + EPSILON) / ((1 - rounded).sum() + EPSILON)
    out = {"a": (np.mean(dp_alpha), np.std(dp_alpha)), "assignment": assign, "genotypes": geno, "FN": (np.mean(fn), np.std(fn)), "FP": (np.mean(fp), np.std(fp)),
           "FN_geno": FN_geno, "FP_geno": FP_geno}
    return (out, info) if details else out


def posterior_estimate(engine, assignments, params, data, dp_alpha, fn, fp, final_assignment=None, details=False, linkage="device"):
    """_get_latents_posterior_chain (utils.py:226-241) of samples that are past their burn-in, on the device: the dict with a, assignment,
    genotypes, FN, FP, FN_geno, FP_geno.  data: the cells x mutations matrix the sampler ran on (NaN for missing).  final_assignment:
    take this clustering (labels 0 .. C-1) instead of the MPEAR cut.  details: also return what the steps produced (D, n_range, scores, ...).
    linkage: "device" (the ward tree, its cuts and the cluster count on the device) or "scipy" (scipy's linkage and cut_tree and the numpy
    count on the host, over the same resident samples); both give the same bits."""
    a, p = _check_samples(assignments, params)
    return _estimate(_Device(engine, a, p, linkage), a, data, dp_alpha, fn, fp, final_assignment, details)


def posterior_estimate_host(assignments, params, data, dp_alpha, fn, fp, final_assignment=None, details=False):
    """The same estimate in numpy, without a device"""
    a, p = _check_samples(assignments, params)
    return _estimate(_Host(a, p), a, data, dp_alpha, fn, fp, final_assignment, details)


# ---- the files (dpmmIO.py:464-521).  inferred: {chain: {estimator: estimate}}, as _infer_results (dpmmIO.py:199-225) builds it ----------
def save_errors(inferred, estimators, chains, out_dir):
    """errors.txt: len(estimators) x chains rows, of which only the inferred ones are filled; the others print as empty rows"""
    import pandas as pd
    idx = np.arange(len(estimators) * chains)
    cols = ["chain", "estimator", "FN_model", "FN_data", "FP_model", "FP_data"]
    df = pd.DataFrame(index=idx, columns=cols)
    i = 0
    for chain, data_chain in inferred.items():
        for est, data_est in data_chain.items():
            if est == "posterior":
                errors = [f'{data_est["FN"][0]:.4f}+-{data_est["FN"][1]:.4f}', data_est["FN_geno"].round(4),
                          f'{data_est["FP"][0]:.8f}+-{data_est["FP"][1]:.8f}', data_est["FP_geno"].round(8)]
            else:
                errors = [data_est["FN"].round(4), data_est["FN_geno"].round(4), data_est["FP"].round(8), data_est["FP_geno"].round(8)]
            df.iloc[i] = [chain, est] + errors
            i += 1
    df.to_csv(os.path.join(out_dir, "errors.txt"), index=False, sep="\t")


def save_assignments(inferred, estimators, chains, out_dir):
    import pandas as pd
    idx = np.arange(len(estimators) * chains)
    df = pd.DataFrame(columns=["chain", "estimator", "Assignment"], index=idx)
    i = 0
    for chain, data_chain in inferred.items():
        for est, data_est in data_chain.items():
            df.iloc[i] = [chain, est, " ".join([str(x) for x in data_est["assignment"]])]
            i += 1
    df.to_csv(os.path.join(out_dir, "assignment.txt"), index=False, sep="\t")


def save_geno(inferred, out_dir, names=np.array([])):
    """genotypes_<est>_<chain>.tsv (rounded) and, unless every value is an integer already, genotypes_cont_<est>_<chain>.tsv (4 decimals);
    like the reference, it puts names on the estimate's genotypes"""
    for chain, data_chain in inferred.items():
        for est, data_est in data_chain.items():
            geno = data_est["genotypes"]
            if names.size == geno.index.size:
                geno.index = names
            if (geno.round() == geno).all().all():
                geno.astype(int).to_csv(os.path.join(out_dir, f"genotypes_{est}_{chain:0>2}.tsv"), sep="\t")
            else:
                geno.round(4).to_csv(os.path.join(out_dir, f"genotypes_cont_{est}_{chain:0>2}.tsv"), sep="\t")
                geno.round().astype(int).to_csv(os.path.join(out_dir, f"genotypes_{est}_{chain:0>2}.tsv"), sep="\t")
