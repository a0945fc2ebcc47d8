"""CPU: step 3 with its rows decided and printed by the row code the device shares (csrc/step3_core.h, csrc/step3_cluster.h), through its
host twin (lsio_step3_core_rows, calling.step3_native), against calling.step3 - whose pandas path the reference-generated goldens pin."""
import pytest

from longsom_amd import calling

from . import step3_cases as sc


def native(tmp_path, name, args, text):
    rep = {}
    got = sc.check_against_reference(tmp_path, name, args, text, calling.step3_native, report=rep)
    return got, rep


@pytest.mark.parametrize("prefix,args", sc.GOLDENS)
def test_host_twin_writes_the_reference_golden_files(tmp_path, prefix, args):
    text = sc.rd(prefix + ".calling.step2.tsv")
    (final, unfiltered), rep = native(tmp_path, prefix, args, text)
    assert unfiltered == sc.rd(prefix + ".calling.step3.unfiltered.tsv")
    assert final == sc.rd(prefix + ".calling.step3.tsv")
    assert rep["path"] == "native" and rep["rows_in"] == 565 and rep["n_undecided"] == 0, rep
    assert rep["rows_all"] == unfiltered.count("\n") - text.count("\n#") - 2 and rep["rows_pass"] == final.count("\n") - text.count("\n#") - 2, rep
    assert 0 < rep["rows_pass"] < rep["rows_pass_unclustered"] and rep["n_clustered"] > 0, rep


@pytest.fixture(scope="module")
def replicated():
    return sc.replicated_tables()


@pytest.mark.parametrize("which", [0, 1], ids=["30k_rows", "one_cell_type"])
@pytest.mark.parametrize("clust", [10000, 150, 1])
def test_host_twin_equals_step3_on_the_replicated_tables(tmp_path, replicated, which, clust):
    got, rep = native(tmp_path, "t%d" % which, (0.05, 0.3, 3, 2, clust), replicated[which])
    assert rep["path"] == "native" and rep["rows_in"] >= 3000 and rep["rows_all"] > rep["rows_pass"] > 0, rep
    if clust == 1:
        assert rep["n_clustered"] == 0 and rep["rows_pass"] == rep["rows_pass_unclustered"], rep


HAND = sc.hand_made()


@pytest.mark.parametrize("name,args,text", HAND, ids=[c[0] for c in HAND])
def test_host_twin_equals_step3_on_hand_made_rows(tmp_path, name, args, text):
    (final, unfiltered), rep = native(tmp_path, name, args, text)
    assert rep["path"] == "native", rep
    tags = [l.split("\t")[-2] for l in unfiltered.split("\n")[len(sc.hc.HEAD) + 1:] if l]
    if name == "multi_two_types":
        rows = [l.split("\t") for l in unfiltered.split("\n") if l and not l.startswith("#")]
        i_f, i_bc, i_alt = sc.COLS.index("FILTER"), sc.COLS.index("Bc"), sc.COLS.index("ALT")
        assert [r[i_f] for r in rows[:4]] == ["Multi-allelic"] * 4, "a FILTER of two cell types stays as it came"
        assert rows[0][i_bc] == rows[2][i_bc] == "2,30" and rows[0][i_alt] == "T,T", "the pairs print Non-Cancer, Cancer in either order of Cell_types"
        assert "Multi-Allelic" in tags and "Multi-Allelic,LowDepth" in tags and "Multi-Allelic,CancerNonSig" in tags and "PASS" in tags, tags
    if name == "multi_one_type":
        assert {"Multi-Allelic", "Multi-Allelic,LowDepth,CancerNonSig", "CancerNonSig", "PASS"} <= set(tags), tags
    if name == "chrm":
        assert {"LowDepth", "LowDeltaVAF", "LowDeltaMCF", "LowVAF", "LowMCF", "Multi-Allelic,LowDepth", "PASS"} <= set(tags), tags
    if name == "counts_and_significance":
        assert {"NoCov", "LowDepth", "CancerNonSig", "NonCancerSig", "NoCov,CancerNonSig", "NoCov,NonCancerSig", "LowDepth,CancerNonSig", "LowDepth,NonCancerSig",
                "Multi-Allelic,LowDepth,CancerNonSig", "Multi-Allelic,LowDepth,NonCancerSig", "PASS"} <= set(tags), tags
    if name == "cluster_string_order_10":
        assert tags == ["PASS"] * 6, "9999 and 10001 are neighbours in numeric order only"
    if name == "cluster_string_order_60000":
        assert tags.count("Clust_dist_60000") == 2 and tags[:3] == ["PASS"] * 3, tags
    if name == "same_index":
        assert tags[:5] == ["Clust_dist_10000", "LowDepth,Clust_dist_10000", "Clust_dist_10000", "PASS", "NoCov"] and rep["n_clustered"] == 2, (tags, rep)


ODD = sc.decided_oddities()


@pytest.mark.parametrize("name,args,text", ODD, ids=[c[0] for c in ODD])
def test_host_twin_decides_what_the_reference_never_looks_at(tmp_path, name, args, text):
    _, rep = native(tmp_path, name, args, text)
    assert rep["path"] == "native", rep


UNDECIDED = sc.undecided()


@pytest.mark.parametrize("name,args,text,why,ordinal,reason", UNDECIDED, ids=[c[0] for c in UNDECIDED])
def test_host_twin_hands_back_what_it_cannot_decide(tmp_path, name, args, text, why, ordinal, reason):
    """the result, or the exception's type, is the pandas path's; the report names the row and the reason"""
    _, rep = native(tmp_path, name, args, text)
    assert rep["path"] == "fallback", rep
    if why is not None:
        assert rep["why"] == why, rep
    else:
        assert (rep["first_undecided"], rep["reason"]) == (ordinal, reason) and rep["n_undecided"] >= 1, rep
        assert rep["why"] == "row %d: %s" % (ordinal, calling.STEP3_REASONS[reason]), rep


def test_the_pandas_switches_keep_the_pandas_path(tmp_path, monkeypatch):
    monkeypatch.setenv("LONGSOM_STEP3_PANDAS", "1")
    _, rep = native(tmp_path, "sample", sc.ARGS, sc.rd("sample.calling.step2.tsv"))
    assert rep["path"] == "fallback" and "rows_in" not in rep, rep
