"""GPU: the BAM index made on the device (csrc/bamindex.hip: lsg_bam_index -> table LSG_TABLE_BAI; lsg_split_bam under lsg_set_split_index ->
tables LSG_TABLE_SPLIT_BAI + t) against the host twin (hostio.build_bai(full=True)), which tests/test_bai_cpu.py pins against the contract
restated in Python.  Three routes to one file: the split's own index, the host twin's index of the written BAM, lsg_bam_index of it."""
import json
import os

import pytest

from longsom_amd import _lib, cli, hostio
from tests.support import bai_cases

pytestmark = pytest.mark.gpu
SPLIT_NAMES = tuple(n for n in bai_cases.NAMES)


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("bai_gpu")
    out = {}
    for name, raw in bai_cases.cases().items():
        out[name] = str(d / (name + ".bam"))
        with open(out[name], "wb") as f:
            f.write(raw)
    return out


def host_bai(bam, tmp_path, tag="h"):
    with open(hostio.build_bai(bam, str(tmp_path / (tag + ".bai")), full=True), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", bai_cases.NAMES)
def test_bam_index_equals_the_host_twin(engine, bams, tmp_path, name):
    info = engine.bam_index(bams[name])
    got = engine.table_bytes(engine.TABLE_BAI, info["n_bytes"])
    assert got == host_bai(bams[name], tmp_path)
    idx = hostio.read_bai_full(got)
    assert info["n_no_coor"] == idx["n_no_coor"] == info["n_records"] - info["n_placed"]
    assert info["n_bins"] == sum(len(r["bins"]) for r in idx["refs"]) and info["n_chunks"] == sum(len(c) for r in idx["refs"] for c in r["bins"].values())
    assert info["n_windows"] == sum(len(r["ioffset"]) for r in idx["refs"]) and info["n_runs"] >= info["n_chunks"]
    assert info["bad_ordinal"] == -1 and info["bad_kind"] == 0 and info["ms_total"] > 0
    engine.free_table(engine.TABLE_BAI)


def split(engine, bam, index):
    table = bai_cases.split_table()
    engine.set_split_index(index)
    try:
        info = engine.split_bam(bam, table.barcodes, table.celltype_of, len(table.celltype_names), 60)
    finally:
        engine.set_split_index(False)
    return info, [engine.table_bytes(engine.TABLE_SPLIT_BAM + t, info["n_file_bytes"][t]) for t in range(2)]


@pytest.mark.parametrize("name", SPLIT_NAMES)
def test_split_index_three_routes_one_file(engine, bams, tmp_path, name):
    """each cell type's BAI out of the routing's arrays = the host twin's index of the written BAM = lsg_bam_index of that BAM; and the
    BAMs are byte for byte those of the call without the switch, which leaves no BAI table"""
    info, files = split(engine, bams[name], True)
    bais = [engine.table_bytes(engine.TABLE_SPLIT_BAI + t, info["index"][t]["n_bytes"]) for t in range(2)]
    assert len(info["index"]) == 2
    for t in range(2):
        path = str(tmp_path / ("ct%d.bam" % t))
        with open(path, "wb") as f:
            f.write(files[t])
        assert bais[t] == host_bai(path, tmp_path, "ct%d" % t), "cell type %d" % t
        again = engine.bam_index(path)
        assert engine.table_bytes(engine.TABLE_BAI, again["n_bytes"]) == bais[t], "cell type %d" % t
        assert info["index"][t]["n_records"] == info["n_written"][t] == again["n_records"] and info["index"][t]["n_no_coor"] == 0
        assert (info["index"][t]["n_runs"], info["index"][t]["n_chunks"], info["index"][t]["n_bins"]) == (again["n_runs"], again["n_chunks"], again["n_bins"])
    if name not in ("empty", "all_unplaced"):
        assert sum(info["n_written"]) > 0
    off, files_off = split(engine, bams[name], False)
    assert files_off == files and "index" not in off
    for t in range(4):
        with pytest.raises(_lib.LsgError):
            engine.table_bytes(engine.TABLE_SPLIT_BAI + t, 8)


def test_oversize_record_leaves_a_block_open_in_the_split_output(engine, bams):
    """the 70 000-base read spills over 0xff00-byte blocks of cell type 1's file; the record behind it starts inside the block its tail opened"""
    info, files = split(engine, bams["oversize"], True)
    idx = hostio.read_bai_full(engine.table_bytes(engine.TABLE_SPLIT_BAI + 1, info["index"][1]["n_bytes"]))
    starts = sorted(c[0] for chunks in idx["refs"][0]["bins"].values() for c in chunks)
    assert info["n_blocks"][1] >= 3 and any(s & 0xffff for s in starts)


@pytest.mark.parametrize("name", bai_cases.REFUSED_NAMES)
def test_refusals(engine, tmp_path, name):
    raw, ordinal, kind = bai_cases.refused()[name]
    bam = str(tmp_path / "x.bam")
    with open(bam, "wb") as f:
        f.write(raw)
    with pytest.raises(_lib.LsgError) as e:
        engine.bam_index(bam)
    assert e.value.rc == -1 and (e.value.info["bad_ordinal"], e.value.info["bad_kind"]) == (ordinal, kind)
    assert "lsg_bam_index: record %d: " % ordinal in str(e.value) and bai_cases.REFUSED_TEXT[kind] in str(e.value)
    with pytest.raises(_lib.LsgError):
        engine.table_bytes(engine.TABLE_BAI, 8)


@pytest.mark.parametrize("name", sorted(bai_cases.SPLIT_REFUSED))
def test_split_index_refuses_and_keeps_no_table(engine, tmp_path, name):
    """an input whose cell type 0 file cannot be indexed: the call fails with its own message - the cell type, the ordinal in that file,
    the reason -, the refused cell type's info is the last one kept, and neither BAM nor BAI tables stay"""
    raw = bai_cases.refused()[name][0]
    ordinal, kind = bai_cases.SPLIT_REFUSED[name]
    bam = str(tmp_path / "x.bam")
    with open(bam, "wb") as f:
        f.write(raw)
    with pytest.raises(_lib.LsgError) as e:
        split(engine, bam, True)
    assert e.value.rc == -1 and len(e.value.info["index"]) == 1
    bad = e.value.info["index"][0]
    assert (bad["bad_ordinal"], bad["bad_kind"]) == (ordinal, kind)
    text = str(e.value)
    assert text.startswith("lsg_split_bam failed (rc=-1): lsg_split_bam: cell type 0's file cannot be indexed: record %d of it: " % ordinal), text
    assert bai_cases.REFUSED_TEXT[kind] in text and "lsg_get_split_index_info" not in text
    for t in range(2):
        for tab in (engine.TABLE_SPLIT_BAM + t, engine.TABLE_SPLIT_BAI + t):
            with pytest.raises(_lib.LsgError):
                engine.table_bytes(tab, 8)
    info, files = split(engine, bam, False)                     # without the switch the call is what it was: the records are routed
    assert info["n_written"][0] > ordinal and "index" not in info


def test_a_failed_split_keeps_its_own_message_under_the_switch(engine, tmp_path):
    """a failure that has nothing to do with the index (an aligned read at a negative position: lsg_split_bam's validation) reads the same with
    the switch on as with it off"""
    bam = str(tmp_path / "x.bam")
    with open(bam, "wb") as f:
        f.write(bai_cases.refused()["negative_pos"][0])
    texts = []
    for index in (False, True):
        with pytest.raises(_lib.LsgError) as e:
            split(engine, bam, index)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "an alignment that leaves its reference" in texts[0]


def test_cli_writes_the_files(tmp_path, bams, capsys):
    meta = str(tmp_path / "meta.tsv")
    hostio.write_barcodes_tsv(meta, bai_cases.BARCODES, bai_cases.CELLTYPE_OF, bai_cases.CELLTYPES)
    cli.split_bam(["--bam", bams["many_bins"], "--meta", meta, "--id", "s", "--outdir", str(tmp_path), "--min_MQ", "60", "--device", "0", "--index"])
    for ct in bai_cases.CELLTYPES:
        bam = str(tmp_path / ("s.%s.bam" % ct))
        with open(bam + ".bai", "rb") as f:
            assert f.read() == host_bai(bam, tmp_path, ct)
        assert hostio.find_bai(bam) == bam + ".bai"
    capsys.readouterr()
    out = str(tmp_path / "whole.bai")
    cli.index_bam(["--bam", bams["many_bins"], "--out", out, "--device", "0"])
    said = json.loads(capsys.readouterr().out)
    assert said["indexed_on"] == "device" and said["records"] == 769
    with open(out, "rb") as f:
        assert f.read() == host_bai(bams["many_bins"], tmp_path, "whole")
