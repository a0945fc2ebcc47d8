"""CPU: the conditions the wide BnpC cases (tests/support/bnpc_wide_cases.py) must meet for tests/test_bnpc_wide_gpu.py to test what it
says.  They are conditions on the cases and their seeds, asserted on the numpy twin alone: no decision of the twin lies within 1e-9 of its
edge (so a device that adds in another order decides the same), clusters are born, and every width the case is there for is crossed.  If
one fails under another numpy build, the seed changes, never the threshold."""
import numpy as np
import pytest

from longsom_amd import bnpc_sampler as bs
from tests.support import bnpc_wide_cases as wc


# ---- the sweep cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.SWEEP_CASES)
def test_sweep_cases_decide_clear_of_their_edges_and_open_clusters(name):
    _, chains = wc.swept(name)
    for ch in chains:
        print(name, "seed", ch["seed"], "margin %.3g" % ch["margin"].value, "births", ch["margin"].births, "K", len(ch["start"].live()), "->", len(ch["end"].live()))
        assert ch["margin"].value >= 1e-9, "seed %d: a decision of the twin lies within %g of its edge" % (ch["seed"], ch["margin"].value)
        assert ch["margin"].births > 0, "seed %d opened no cluster: it does not reach the birth path" % ch["seed"]
        assert ch["errors"] == 0


def test_random300_passes_256_slots_inside_the_sweep():
    """hi + 1 <= 256 at the start, so a lane owns one slot; above it at the end, so it owns two: the width changes between two cells"""
    model, chains = wc.swept("random300")
    assert model.N == 300 and model.M == 130
    for ch in chains:
        assert wc.hi_of(ch["start"]) < 256 < wc.hi_of(ch["end"])
        assert ch["end"].labels.max() >= 256                          # cells sit in clusters whose id has no column of LL and lies past the first slot of every lane


@pytest.mark.parametrize("name,N,M,K", [("singletons257", 257, 65, 257), ("gaps513", 513, 33, 40), ("singletons600", 600, 10, 600)])
def test_wide_starts_are_wide(name, N, M, K):
    model, chains = wc.swept(name)
    assert (model.N, model.M) == (N, M)
    for ch in chains:
        assert wc.hi_of(ch["start"]) + 1 > 256 and len(ch["start"].live()) == K
    if name == "gaps513":
        live = chains[0]["start"].live()
        assert live[-1] == 512 and np.count_nonzero(live < 256) > 0 and np.count_nonzero(live >= 256) > 1
        assert all(len(ch["end"].live()) > K for ch in chains)        # the births take free ids inside the lanes' runs
    else:
        # K falls: the ids of the emptied clusters, those >= 256 among them, are free and a later birth of the sweep may take them
        assert all(len(ch["end"].live()) < K for ch in chains)
        assert any((ch["end"].sizes[256:] == 0).any() for ch in chains)
    if name == "singletons600":
        assert not (model.pop1[599] + model.pop0[599])                # the all-missing cell


# ---- the parameter move ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pp", wc.MOVE_PP)
@pytest.mark.parametrize("K", wc.MOVE_K)
def test_parameter_moves_accept_clear_of_their_thresholds(K, pp):
    for M in wc.MOVE_M:
        model, ids, labels, chains = wc.moved(K, M, pp)
        assert len(ids) == K and np.array_equal(np.unique(labels), ids) and model.N == wc.MOVE_N
        for ch in chains:
            assert ch["margin"].value >= 1e-9, "K %d M %d seed %d: an acceptance of the twin lies within %g of its threshold" % (K, M, ch["seed"], ch["margin"].value)
            assert (ch["end"].theta[ids] != ch["start"].theta[ids]).any()


# ---- the run -----------------------------------------------------------------------------------------------------------------------------
def test_run_replayed_step_by_step_crosses_256_clusters():
    """the eight steps again, move by move under one Margin: the replay is the run (its labels at every step), no decision of it is near its
    edge, and a kept step has more than 256 live clusters, so the record's sums and the arena rows go past one slot per lane"""
    host = wc.run_host()
    model = bs.Model(wc.run_data(), wc.RUN_FN, wc.RUN_FP, **wc.RUN_KW)
    st = bs.initial_state(model, wc.RUN_SEED)
    margin = bs.Margin()
    assert np.array_equal(st.labels, host["assignments"][0])
    for s in range(1, wc.RUN_STEPS + 1):
        assert bs.gibbs_sweep(model, st, wc.RUN_SEED, s, margin) == 0
        assert bs.alpha_update(model, st, wc.RUN_SEED, s, margin) == 0
        bs.parameter_move(model, st, wc.RUN_SEED, s, margin)
        assert np.array_equal(st.labels, host["assignments"][s]), s
    print("replay margin %.3g" % margin.value)
    assert margin.value >= 1e-9
    K = [len(np.unique(row)) for row in host["assignments"]]
    print("K per step", K)
    assert max(K[wc.RUN_BURN_IN:]) > 256
    assert host["params"].shape == (wc.RUN_STEPS + 1 - wc.RUN_BURN_IN, max(K[wc.RUN_BURN_IN:]), 33) and host["variate_errors"] == 0
    assert sum(K[wc.RUN_BURN_IN:]) > wc.RUN_SMALL_ARENA >= max(K)      # the small arena holds any one step and not the kept steps together


# ---- the estimate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,K", wc.ESTIMATE_WIDE)
def test_wide_estimate_shapes_have_many_labels(N, S, K):
    a = wc.estimated(N, S, K)["a"]
    for row in a:
        assert len(np.unique(row)) > 1024                             # more clusters than four per lane; ranks far above 255
    assert a.max() >= 2048                                            # labels in the upper half of the presence bitmap's words


def test_estimate_shapes_reach_every_branch():
    seen = set()
    for shape in wc.ESTIMATE_SHAPES:
        for _, (_, branch, _) in wc.estimated(*shape)["finals"]:
            seen |= set(int(b) for b in branch)
    assert {1, 2, 3} <= seen
