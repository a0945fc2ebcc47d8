"""CPU: the HCCV filter with its rows decided and printed by the row code the device shares (csrc/hccv_core.h), through its host twin
(lsio_hccv_rows) and the driver both forms use (reanno.hccv_filter_native): the reference's own output (tests/golden/sample*.HCCV.tsv*,
made by running HighConfidenceCancerVariants.py) byte for byte, and reanno.hccv_filter on tables built around every comparison the
filter makes."""
import os

import pytest

from longsom_amd import reanno
from longsom_amd.reanno import hccv_filter_native

from . import hccv_cases as hc


@pytest.mark.parametrize("tag,args", hc.GOLDEN_ARGS)
def test_native_equals_the_reference_output(tmp_path, tag, args):
    rep = {}
    out = hccv_filter_native(hc.STEP2, str(tmp_path / tag), *args, report=rep)
    assert rep["path"] == "native" and rep["n_undecided"] == 0, rep          # decided by the row code, not handed to the pandas form
    for suffix in ("", "2", "3"):
        assert open(out + suffix).read() == open(os.path.join(hc.G, tag + ".HCCV.tsv" + suffix)).read(), "%s.HCCV.tsv%s differs" % (tag, suffix)
    assert rep["rows_in"] == 565 and rep["rows_tsv2"] > rep["rows_tsv3"] > rep["rows_pass"] >= 3


@pytest.mark.parametrize("seed", range(4))
def test_native_equals_hccv_filter_on_tables_of_golden_rows(tmp_path, seed):
    decided = 0
    for name, args, text in hc.seeded_tables(seed):
        rep = {}
        got = hc.check_against_reference(tmp_path, name, args, text, hccv_filter_native, report=rep)
        decided += rep.get("path") == "native"
        if name.startswith("all"):
            assert rep["path"] == "native" and not isinstance(got, type), rep
    assert decided >= 2                                  # (tables of one kind of row may leave no row: those are the pandas form's)


CASES = hc.hand_made()


@pytest.mark.parametrize("name,args,text", CASES, ids=[c[0] for c in CASES])
def test_native_equals_hccv_filter_on_hand_made_rows(tmp_path, name, args, text):
    rep = {}
    got = hc.check_against_reference(tmp_path, name, args, text, hccv_filter_native, report=rep)
    if name == "rows_0":
        assert rep["path"] == "fallback", rep                # no row reaches .tsv2: the reference's frame code decides what happens
    else:
        assert rep["path"] == "native" and not isinstance(got, type), rep


def test_hand_made_rows_reach_every_verdict(tmp_path):
    """the tables above are not all of one outcome: every verdict, a dropped and a kept multi-allelic row, an emptied FILTER, a blank cell"""
    seen, text3 = set(), ""
    for name, args, text in CASES:
        if name in ("verdict", "runner_up", "filter_text"):
            path = tmp_path / (name + ".tsv"); path.write_text(text)
            out = hccv_filter_native(str(path), str(tmp_path / name), *args)
            rows = [l.split("\t") for l in open(out + "3").read().split("\n")[1:-1]]
            seen |= {r[-1] for r in rows}
            text3 += open(out + "3").read()
    assert seen == {"PASS", "Low VAF/MCF", "NonSig", "Heterozygous", "LowDeltaMCF", "NonCancer"}
    assert "\tT,T\t\tCancer,Non-Cancer\t" in text3           # FILTER "Multi-allelic" stripped to nothing
    assert "\tchr1:2000:C|T\t" in text3 and "chr1:1000:C|T" not in text3 and "chr1:5000:C|T" not in text3      # runner-up 1/21 kept, 1/20 and a tie dropped
    assert "\tCancer,Non-Cancer\t\t\t1\t" in text3           # Up_context "NA" and Down_context "null" print as nothing


UNDECIDED = hc.undecided()


@pytest.mark.parametrize("name,args,text,ordinal,reason", UNDECIDED, ids=[c[0] for c in UNDECIDED])
def test_undecided_tables_go_to_hccv_filter(tmp_path, name, args, text, ordinal, reason):
    rep = {}
    got = hc.check_against_reference(tmp_path, name, args, text, hccv_filter_native, report=rep)
    assert rep["path"] == "fallback" and (name == "max_zero") == isinstance(got, type), (rep, got)
    if ordinal is None:
        assert rep["n_undecided"] == 0 and rep["why"] == "column kinds", rep
    else:
        assert rep["n_undecided"] == 1 and rep["first_undecided"] == ordinal and rep["reason"] == reason, rep
        assert not os.path.exists(str(tmp_path / (name + ".probe.HCCV.tsv")))
        assert reanno._hccv_drive(reanno._HostRows(text.encode()), text.splitlines(True)[:3], "", str(tmp_path / (name + ".probe")), *args, fallback=False) is None


def test_cli_flag_native_writes_the_same_files(tmp_path):
    from longsom_amd import cli
    cli.hccv(["--SNVs", hc.STEP2, "--outfile", str(tmp_path / "s"), "--min_dp", "50", "--deltaVAF", "0.2", "--deltaMCF", "0.25", "--clust_dist", "10000", "--native"])
    for suffix in ("", "2", "3"):
        assert open(str(tmp_path / "s.HCCV.tsv") + suffix).read() == open(os.path.join(hc.G, "sample.HCCV.tsv" + suffix)).read()
