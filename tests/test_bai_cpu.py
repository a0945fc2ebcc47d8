"""CPU: the whole BAM index of the host twin (hostio.build_bai(full=True) -> lsio_build_bai_full, csrc/bamindex_core.h) against the
contract of DESIGN.md §16 restated in plain Python (tests/support/bai_oracle.py), against the existing linear-index builder, and against
what an index is for: a region query through it must reach every record that overlaps the region.  No htslib-written .bai exists among
the fixtures, so nothing here is pinned against samtools."""
import os
import random

import numpy as np
import pytest

from longsom_amd import hostio
from tests.support import bai_cases, bai_oracle


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (bam path, the file's bytes, the host twin's .bai bytes, the oracle's Records)"""
    d = tmp_path_factory.mktemp("bai")
    out = {}
    for name, raw in bai_cases.cases().items():
        bam = str(d / (name + ".bam"))
        with open(bam, "wb") as f:
            f.write(raw)
        bai = hostio.build_bai(bam, full=True)
        assert bai == bam + ".bai"
        out[name] = (bam, raw, open(bai, "rb").read(), bai_oracle.Records(raw))
    return out


@pytest.mark.parametrize("name", bai_cases.NAMES)
def test_host_twin_equals_the_oracle(built, name):
    _, raw, bai, _ = built[name]
    assert bai == bai_oracle.build(raw)


@pytest.mark.parametrize("name", bai_cases.NAMES)
def test_linear_index_equals_the_existing_builder(built, tmp_path, name):
    bam, _, bai, _ = built[name]
    lin = hostio.read_bai(hostio.build_bai(bam, str(tmp_path / "lin.bai")))
    full = hostio.read_bai_full(bai)
    assert len(lin) == len(full["refs"])
    for a, ref in zip(lin, full["refs"]):
        assert np.array_equal(a, ref["ioffset"])
    assert [np.array_equal(a, b) for a, b in zip(lin, hostio.read_bai(bam + ".bai"))] == [True] * len(lin)      # read_bai skips the bins of either file


def test_shapes_are_what_the_cases_say(built):
    """the counts the cases were laid out for, read off the files"""
    idx = {n: hostio.read_bai_full(built[n][2]) for n in bai_cases.NAMES}
    e = idx["empty"]["refs"][0]
    assert idx["empty"]["n_no_coor"] == 0 and e["bins"] == {} and e["meta"] is None and len(e["ioffset"]) == 0
    assert idx["all_unplaced"]["n_no_coor"] == 5 and idx["all_unplaced"]["refs"][0]["bins"] == {}
    mid = idx["middle_empty"]
    assert mid["n_no_coor"] == 5 and mid["refs"][1]["bins"] == {} and mid["refs"][1]["meta"] is None and len(mid["refs"][1]["ioffset"]) == 0
    assert mid["refs"][0]["meta"][2:] == (2, 2) and mid["refs"][2]["meta"][2:] == (2, 1)
    lev = idx["levels"]["refs"][0]
    assert sorted(lev["bins"]) == [0, 1, 9, 73, 585, 4681, 4681 + 2, 4681 + 32767] and len(lev["ioffset"]) == 32768      # levels 0..5, the last window
    assert len(idx["bin_back_one_block"]["refs"][0]["bins"][4681]) == 1 and len(idx["bin_back_two_blocks"]["refs"][0]["bins"][4681]) == 2
    many = idx["many_bins"]["refs"][0]
    assert len(many["bins"]) == 513 and sum(len(c) for c in many["bins"].values()) == 513 and many["meta"][2:] == (769, 0)
    deep = idx["deep_window"]["refs"][0]
    assert list(deep["bins"]) == [4681] and len(deep["bins"][4681]) == 1 and deep["meta"][2:] == (2970, 30)
    lc = idx["long_cigar"]["refs"][0]
    assert len(lc["ioffset"]) == 84 and len(set(int(x) for x in lc["ioffset"][9:84])) == 1      # the spliced read's 75 windows


def edges(recs):
    """every window and bin edge the records touch, as one-base and straddling regions"""
    out = set()
    for tid, pos, end, *_ in recs.recs:
        if tid < 0:
            continue
        for x in (pos, end):
            for shift in (14, 17, 20, 23, 26):
                e = (x >> shift) << shift
                for b, en in ((e - 1, e), (e, e + 1), (e - 1, e + 1), (e, e + (1 << shift))):
                    if b >= 0 and en <= (1 << 29):
                        out.add((tid, b, en))
    return sorted(out)


@pytest.mark.parametrize("name", bai_cases.NAMES)
def test_a_query_reaches_every_overlapping_record(built, name):
    """seeded random regions and every window / bin edge: the records that start inside bai_query's chunks are a superset of the brute-force
    overlaps; and every chunk boundary is a record boundary"""
    _, _, bai, recs = built[name]
    index = hostio.read_bai_full(bai)
    starts = np.array([r[4] for r in recs.recs], np.uint64)
    bounds = set(int(s) for s in starts) | ({recs.recs[-1][5]} if recs.recs else set())
    for ref in index["refs"]:
        for chunks in ref["bins"].values():
            for b, e in chunks:
                assert b in bounds and e in bounds and b < e
        if ref["meta"]:
            assert ref["meta"][0] in bounds and ref["meta"][1] in bounds
    rng = random.Random(20261021)
    regions = edges(recs)
    if len(regions) > 600:
        regions = rng.sample(regions, 600)
    for tid in range(recs.n_ref):
        mine = [r for r in recs.recs if r[0] == tid]
        hi = max((r[2] for r in mine), default=1000) + 20000
        for _ in range(300 // recs.n_ref):
            b = rng.randrange(0, hi); regions.append((tid, b, min(b + rng.choice((1, 50, 5000, 40000, 3_000_000)), 1 << 29)))
    for tid, b, e in regions:
        want = recs.overlapping(tid, b, e)
        chunks = hostio.bai_query(index, tid, b, e)
        got = np.zeros(len(starts), bool)
        for cb, ce in chunks:
            got |= (starts >= cb) & (starts < ce)
        assert got[want].all(), (name, tid, b, e)


@pytest.mark.parametrize("name", bai_cases.REFUSED_NAMES)
def test_refusals_name_the_record(tmp_path, name):
    raw, ordinal, kind = bai_cases.refused()[name]
    with pytest.raises(bai_oracle.Refused) as o:
        bai_oracle.build(raw)
    assert (o.value.ordinal, o.value.kind) == (ordinal, kind)
    bam = str(tmp_path / "x.bam")
    with open(bam, "wb") as f:
        f.write(raw)
    with pytest.raises(hostio.BaiError) as e:
        hostio.build_bai(bam, full=True)
    assert (e.value.info["bad_ordinal"], e.value.info["bad_kind"]) == (ordinal, kind) and "record %d)" % ordinal in str(e.value)
    assert not os.path.exists(bam + ".bai")
    hostio.build_bai(bam, str(tmp_path / "lin.bai"))            # (the linear-index builder is what it was: it checks none of this)


def test_cli_index_bam_on_the_host(tmp_path, built, capsys):
    import json
    from longsom_amd import cli
    bam, _, bai, _ = built["middle_empty"]
    out = str(tmp_path / "m.bai")
    cli.index_bam(["--bam", bam, "--out", out])
    assert json.loads(capsys.readouterr().out)["indexed_on"] == "host" and open(out, "rb").read() == bai
