"""longsom_amd.bnpc's numpy twins of scipy's ward linkage and cut_tree (what lsg_bnpc_linkage and lsg_bnpc_cut_tree compute), held to scipy
itself bit for bit, over label matrices that make tied heights and heights that rounding puts out of order."""
import functools

import numpy as np
import pytest

from longsom_amd import bnpc

NS = (2, 3, 4, 45, 63, 64, 65, 87, 130)
SS = (1, 2, 7, 33, 257)
LAYOUTS = ("one", "alone", "planted2", "planted30")


def labels(layout, N, S):
    """[S, N] label matrices: one cluster in every sample (all distances 0, every height tied), every cell alone, or planted clusters with
    2 % / 30 % of the cells relabelled, every sample named through a random injection into [0, N)"""
    if layout == "one":
        return np.zeros((S, N), np.int64)
    if layout == "alone":
        return np.tile(np.arange(N), (S, 1))
    rng = np.random.default_rng(N * 1000 + S)
    K = max(1, min(5, N // 2))
    truth = rng.integers(0, K, N)
    noise = 0.02 if layout == "planted2" else 0.3
    a = np.zeros((S, N), np.int64)
    for s in range(S):
        lab = truth.copy()
        move = rng.random(N) < noise
        inj = rng.permutation(N)[:min(N, K + 3)]
        lab[move] = rng.integers(0, len(inj), int(move.sum()))
        a[s] = inj[lab % len(inj)]
    return a


def condensed(a):
    return bnpc._Host(a, None).codist() / a.shape[0]


CASES = [(layout, N, S) for layout in LAYOUTS for N in NS for S in SS]


@functools.lru_cache(maxsize=None)
def solved(layout, N, S):
    """(scipy's Z, the twin's Z, the sizes the twin's chain recorded) of one case, computed once"""
    from scipy.cluster.hierarchy import linkage
    dist = condensed(labels(layout, N, S))
    return (linkage(dist, method="ward"),) + bnpc.ward_linkage_host(dist, chain_sizes=True)


@pytest.mark.parametrize("layout,N,S", CASES)
def test_twins_against_scipy(layout, N, S):
    from scipy.cluster.hierarchy import cut_tree
    want, Z, _ = solved(layout, N, S)
    assert Z.shape == want.shape and np.array_equal(Z.view(np.uint64), want.view(np.uint64))
    ns = list(range(1, N))
    cuts = bnpc.cut_tree_host(want, ns)
    assert cuts.shape == (N - 1, N) and np.array_equal(cuts, cut_tree(want, n_clusters=ns).T)


def test_the_two_subtle_rules_are_exercised():
    """some case has tied heights (cut_tree's order among them), some a chain whose own sizes are not the labelled ones"""
    tied = [c for c in CASES if (np.diff(solved(*c)[0][:, 2]) == 0).any()]
    sizes_differ = [c for c in CASES if (solved(*c)[2] != solved(*c)[0][:, 3]).any()]
    print("tied heights in %d cases; chain sizes differ in %s" % (len(tied), sizes_differ))
    assert tied and sizes_differ


def test_cuts_in_any_order_and_twice():
    from scipy.cluster.hierarchy import cut_tree, linkage
    Z = linkage(condensed(labels("planted30", 65, 7)), method="ward")
    ns = [7, 2, 64, 7, 1, 33]
    assert np.array_equal(bnpc.cut_tree_host(Z, ns), cut_tree(Z, n_clusters=ns).T)
    assert np.array_equal(bnpc.cut_tree_host(Z, 5), cut_tree(Z, n_clusters=5).T)


def test_n_clusters_of_all_cells_raises():
    Z = bnpc.ward_linkage_host(condensed(labels("planted2", 45, 7)))
    for n in (45, 0, 46):
        with pytest.raises(ValueError, match=r"n_clusters must lie in 1 \.\. 44"):
            bnpc.cut_tree_host(Z, [2, n])
    with pytest.raises(ValueError, match="no condensed distance matrix"):
        bnpc.ward_linkage_host(np.zeros(4))
