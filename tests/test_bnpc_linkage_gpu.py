"""The ward tree, its cuts and the cluster count of BnpC's posterior estimate on the device (csrc/bnpc_linkage.hip: lsg_bnpc_linkage,
lsg_bnpc_cut_tree, lsg_bnpc_cluster_counts) against scipy's linkage and cut_tree and numpy's count, bit for bit."""
import numpy as np
import pytest

from longsom_amd import _lib, bnpc
from tests.test_bnpc_cpu import CASES, chains, gold
from tests.test_bnpc_linkage_cpu import LAYOUTS, labels

pytestmark = pytest.mark.gpu

# (N, S): degenerate chains; the 64-cell tile edge of the packed labels and one more tile; one cell a lane of the 1024 that walk the chain,
# and the first lane with two; three a lane.  S = 1 at N = 45 and 87: heights that rounding puts out of order.
SHAPES = [(2, 1), (3, 2), (63, 33), (64, 7), (65, 257), (130, 33), (1023, 3), (1024, 5), (1025, 5), (2049, 5)]
GENERATED = [(layout, N, S) for N, S in SHAPES for layout in LAYOUTS] + [(layout, N, 1) for N in (45, 87) for layout in LAYOUTS]


@pytest.mark.parametrize("layout,N,S", GENERATED)
def test_tree_cuts_and_count_against_scipy(engine, layout, N, S):
    from scipy.cluster.hierarchy import cut_tree, linkage
    a = labels(layout, N, S)
    engine.bnpc_load_samples(a)
    avg = engine.bnpc_avg_cluster_number()                           # needs the samples alone
    want_avg = bnpc.avg_cluster_number(a)
    assert isinstance(avg, np.float64) and avg == want_avg
    D = engine.bnpc_codist()
    want = linkage(D / S, method="ward")
    Z = engine.bnpc_linkage()
    assert Z.shape == want.shape and np.array_equal(Z.view(np.uint64), want.view(np.uint64))
    ns = sorted({int(n) for n in bnpc.cut_range(want_avg, N)} | {n for n in (1, 2, N - 1) if 1 <= n <= N - 1})
    cuts = engine.bnpc_cut_tree(ns)
    assert cuts.dtype == np.int32 and np.array_equal(cuts, cut_tree(want, n_clusters=ns).T)
    engine.bnpc_codist(fetch=False)                                  # new distances: the next cut makes its own tree, in any order of n
    assert np.array_equal(engine.bnpc_cut_tree(ns[::-1]), cuts[::-1])
    engine.bnpc_unload()


@pytest.mark.parametrize("case", [c for c in CASES if c != "sep"])
def test_estimate_with_either_linkage(engine, case):
    cat, g = bnpc.concat_chains(chains(case)), gold(case)
    args = (engine, cat["assignments"], cat["params"], g["data"], cat["DP_alpha"], cat["FN"], cat["FP"])
    dev, dinfo = bnpc.posterior_estimate(*args, final_assignment=g["forced"], details=True, linkage="device")
    sci, sinfo = bnpc.posterior_estimate(*args, final_assignment=g["forced"], details=True, linkage="scipy")
    assert np.array_equal(dev["assignment"], sci["assignment"]) and np.array_equal(dev["genotypes"].values, sci["genotypes"].values)
    assert dev["FN_geno"] == sci["FN_geno"] and dev["FP_geno"] == sci["FP_geno"]
    assert sorted(dinfo) == sorted(sinfo)
    for k in dinfo:
        assert np.array_equal(dinfo[k], sinfo[k]), k
    quiet = bnpc.posterior_estimate(*args, final_assignment=g["forced"])          # without details D stays on the device
    assert np.array_equal(quiet["assignment"], dev["assignment"]) and np.array_equal(quiet["genotypes"].values, dev["genotypes"].values)
    with pytest.raises(ValueError, match="linkage must be"):
        bnpc.posterior_estimate(*args, linkage="host")


def test_error_paths(engine):
    engine.bnpc_unload()
    with pytest.raises(_lib.LsgError, match="lsg_bnpc_cluster_counts: no samples resident"):
        engine.bnpc_avg_cluster_number()
    with pytest.raises(_lib.LsgError, match="lsg_bnpc_linkage: no distances resident"):
        engine.bnpc_linkage()
    a = labels("planted30", 65, 7)
    engine.bnpc_load_samples(a)
    with pytest.raises(_lib.LsgError, match="lsg_bnpc_linkage: no distances resident"):              # loaded, not yet measured
        engine.bnpc_linkage()
    with pytest.raises(_lib.LsgError, match="lsg_bnpc_cut_tree: no distances resident"):
        engine.bnpc_cut_tree([2])
    D = engine.bnpc_codist()
    with pytest.raises(_lib.LsgError, match=r"lsg_bnpc_cut_tree: 0 cuts"):
        engine.bnpc_cut_tree([])
    with pytest.raises(_lib.LsgError, match=r"n_clusters\[1\] = 65 is outside 1 \.\. 64"):
        engine.bnpc_cut_tree([2, 65])
    with pytest.raises(_lib.LsgError, match=r"n_clusters\[0\] = 0 is outside 1 \.\. 64"):
        engine.bnpc_cut_tree([0])
    from scipy.cluster.hierarchy import cut_tree, linkage                                             # the context is as usable as before
    want = linkage(D / 7, method="ward")
    assert np.array_equal(engine.bnpc_cut_tree([3, 64]), cut_tree(want, n_clusters=[3, 64]).T)
    assert np.array_equal(engine.bnpc_linkage().view(np.uint64), want.view(np.uint64))
    assert engine.bnpc_avg_cluster_number() == bnpc.avg_cluster_number(a)
    engine.bnpc_unload()
    with pytest.raises(_lib.LsgError, match="lsg_bnpc_cut_tree: no distances resident"):              # unload took the tree with it
        engine.bnpc_cut_tree([2])
