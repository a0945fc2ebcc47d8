"""CPU: the fusion branch's host side.  hostio.bam_fastq (lsio_bam_fastq, the twin of the device printer) against the FASTQs the
reference's BamToFastq.py wrote (tests/golden/fusion, tools/make_fusion_goldens.py) and against the hand-stated text of the edge-case BAM
(tests/support/fastq_cases.py); routed mode against hostio.split_bam + plain mode per cell type; longsom_amd.fusions against the three
files the reference's FusionCalling.py wrote; the CLI shims against the reference's flag lines."""
import os
import re

import pytest

from longsom_amd import _lib, cli, fusions, hostio
from tests.support import fastq_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fusion")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_plain_mode_equals_the_reference_scripts_fastq(tmp_path):
    out = str(tmp_path / "plain.fastq")
    info = hostio.bam_fastq(os.path.join(GOLD, "plain.bam"), out)
    want = read(os.path.join(GOLD, "plain.fastq"))
    assert read(out) == want
    assert info["n_records"] == info["n_printed"][0] == want.count(b"\n+\n") and info["n_bytes"][0] == len(want) and info["bad_ordinal"] == -1


def test_plain_mode_equals_the_hand_stated_edge_cases(tmp_path):
    recs, text = fc.edge_records()
    bam, out = str(tmp_path / "edge.bam"), str(tmp_path / "edge.fastq")
    fc.write(bam, recs)
    info = hostio.bam_fastq(bam, out)
    got = read(out)
    want = text.encode("latin-1")
    # record by record first, so that a failure names the case
    at = 0
    for (name, n, hq, _tags, _mapped, header) in fc.EDGE:
        piece = got[at:].split(b"\n", 4)
        assert piece[0].decode() == "@" + header, name
        assert len(piece[1]) == max(n, 1) and piece[2] == b"+" and len(piece[3]) == (n if n and hq else 1), name
        at += sum(len(p) + 1 for p in piece[:4])
    assert got == want
    assert info["n_records"] == len(fc.EDGE) == info["n_printed"][0] and info["n_bytes"][0] == len(want)
    assert info["n_printed"][1:] == [0, 0, 0] and info["bad_kind"] == _lib.FASTQ_OK


@pytest.mark.parametrize("kind,code", [("no_cb", _lib.FASTQ_NO_CB), ("cb_type", _lib.FASTQ_CB_TYPE), ("ub_type", _lib.FASTQ_UB_TYPE)])
def test_a_record_that_cannot_be_printed_is_named(tmp_path, kind, code):
    recs, ordinal = fc.bad_records(kind)
    bam = str(tmp_path / "bad.bam")
    fc.write(bam, recs)
    with pytest.raises(hostio.FastqError, match=r"record %d\)" % ordinal) as e:
        hostio.bam_fastq(bam, str(tmp_path / "bad.fastq"))
    assert e.value.info["bad_ordinal"] == ordinal and e.value.info["bad_kind"] == code
    assert recs[ordinal]["name"] in str(e.value)


@pytest.mark.parametrize("filters,golden", [(None, "routed.fastq"), (hostio.SplitFilters(max_nM=2), "routed.nM2.fastq")])
def test_routed_mode_equals_split_bam_then_plain_mode(tmp_path, filters, golden):
    bam, meta = str(tmp_path / "routed.bam"), str(tmp_path / "meta.tsv")
    fc.write(bam, fc.routed_records())
    with open(meta, "w") as f:
        f.write(fc.ROUTED_META)
    table = hostio.read_barcodes(meta)
    assert table.celltype_names == ["Cancer", "Non-Cancer"]
    split = [str(tmp_path / (ct + ".bam")) for ct in table.celltype_names]
    report = hostio.split_bam(bam, table, split, 30, filters)
    chain, per_ct = b"", []
    for b in split:
        i = hostio.bam_fastq(b, b + ".fastq")
        per_ct.append((i["n_printed"][0], i["n_bytes"][0]))
        chain += read(b + ".fastq")
    out = str(tmp_path / "routed.fastq")
    info = hostio.bam_fastq(bam, out, table, 30, filters)
    assert read(out) == chain
    assert chain == read(os.path.join(GOLD, golden))            # ... which is also what the reference's script wrote over the split BAMs
    assert [(info["n_printed"][t], info["n_bytes"][t]) for t in range(2)] == per_ct
    assert sum(info["n_printed"]) == report["Pass_reads"] and info["n_records"] == len(fc.routed_records())
    # the cases the BAM is there for: low MAPQ, unlisted, no CB and unmapped reads are in neither piece
    for name in (b"c2.lowq", b"unlisted", b"nocb", b"^un\n"):
        assert name not in chain
    assert (b"^c1\n" in chain) == (filters is None) and (b"^n2\n" in chain) == (filters is None)      # nM 3 / no nM tag: gone under --max_nM 2


def edge_table():
    import numpy as np
    return hostio.BarcodeTable(list(fc.EDGE_BARCODES), np.asarray(fc.EDGE_CELLTYPE_OF, np.uint8), ["Cancer", "Non-Cancer"])


@pytest.mark.parametrize("max_nm", [None, 2])
def test_routed_mode_over_the_edge_cases_equals_the_hand_stated_text(tmp_path, max_nm):
    """the 70 000-base read at a per-cell-type offset, the unmapped read dropped, "-1" / "X-1-1" / two CB fields routed by the cleaned last
    CB:Z and printed with the first"""
    bam, out = str(tmp_path / "edge.bam"), str(tmp_path / "edge.fastq")
    fc.write(bam, fc.edge_records()[0])
    info = hostio.bam_fastq(bam, out, edge_table(), 60, hostio.SplitFilters(max_nM=max_nm))
    text, counts = fc.edge_routed_text(max_nm)
    got = read(out)
    assert got == text.encode("latin-1")
    assert info["n_printed"][:2] == counts and min(counts) > 0 and sum(info["n_bytes"]) == len(got)
    assert b"@CCCA^U1^long.read\n" in got and b"@FIRST^NA^abcdefg\n" in got and b"un.mapped.q" not in got


@pytest.mark.parametrize("kind,code", [("nm_type", _lib.FASTQ_NM_TYPE), ("nh_type", _lib.FASTQ_NH_TYPE)])
def test_a_listed_read_with_a_string_nM_or_NH_is_named_in_routed_mode(tmp_path, kind, code):
    recs, ordinal = fc.bad_records(kind)
    bam = str(tmp_path / "bad.bam")
    fc.write(bam, recs)
    limit = hostio.SplitFilters(max_nM=2) if kind == "nm_type" else hostio.SplitFilters(max_NH=2)
    with pytest.raises(hostio.FastqError, match=r"read 'tagstr' \(record %d\)" % ordinal) as e:
        hostio.bam_fastq(bam, str(tmp_path / "bad.fastq"), edge_table(), 60, limit)
    assert e.value.info["bad_ordinal"] == ordinal and e.value.info["bad_kind"] == code
    other = hostio.SplitFilters(max_NH=2) if kind == "nm_type" else hostio.SplitFilters(max_nM=2)
    hostio.bam_fastq(bam, str(tmp_path / "ok.fastq"), edge_table(), 60, other)       # the other limit never reads that tag
    hostio.bam_fastq(bam, str(tmp_path / "ok.fastq"), edge_table(), 60)              # ... and without a limit nobody does


def test_routed_mode_refuses_n_trim(tmp_path):
    bam, meta = str(tmp_path / "routed.bam"), str(tmp_path / "meta.tsv")
    fc.write(bam, fc.routed_records())
    with open(meta, "w") as f:
        f.write(fc.ROUTED_META)
    with pytest.raises(hostio.FastqError, match="n_trim"):
        hostio.bam_fastq(bam, str(tmp_path / "o.fastq"), hostio.read_barcodes(meta), 30, hostio.SplitFilters(n_trim=3))


def test_fuzz_records_print_what_their_fields_say(tmp_path):
    """the seeded fuzz the GPU test compares device and host on: here the host's SEQ / QUAL lines against the records' own fields"""
    recs = fc.fuzz_records(300, 700)
    bam, out = str(tmp_path / "fuzz.bam"), str(tmp_path / "fuzz.fastq")
    fc.write(bam, recs)
    info = hostio.bam_fastq(bam, out)
    lines = read(out).split(b"\n")
    assert info["n_printed"][0] == len(recs) and len(lines) == 4 * len(recs) + 1
    for k, r in enumerate(recs):
        head, seq, plus, qual = lines[4 * k:4 * k + 4]
        assert head.endswith(b"^" + r["name"].encode()) and plus == b"+"
        assert seq.decode() == r["seq"]
        assert qual == (bytes(q + 33 for q in r["qual"]) if r["qual"] and r["seq"] != "*" else b"*")


# ---- SomaticFusions ---------------------------------------------------------------------------------------------------------------------------
FUSION_FILES = ("fusionsunfiltered.Fusions.tsv", "fusions.Fusions.tsv", "fusions.Fusions.SingleCellGenotype.tsv")


def test_somatic_fusions_equal_the_reference_scripts_files(tmp_path):
    n = fusions.fusion_report(os.path.join(GOLD, "predictions.tsv"), os.path.join(GOLD, "barcodes.tsv"), 3, 2, 0.1, 0.3, str(tmp_path / "fusions"))
    for name in FUSION_FILES:
        assert read(str(tmp_path / name)) == read(os.path.join(GOLD, name)), name
    unfiltered = read(os.path.join(GOLD, FUSION_FILES[0])).decode().splitlines()[1:]
    outcomes = {line.split("\t")[1] for line in unfiltered}
    assert outcomes == {"PASS", "Low_Cancer_UMI", "Low_Cancer_BC", "Low_delta_MCF", "High_Non-Cancer_MCF"}      # the golden reaches every outcome
    names = [line.split("\t")[0] for line in unfiltered]
    assert "A--B1" in names and "A--B2" in names and not any(x.startswith("K--L") for x in names)
    assert n == {"unfiltered": 7, "pass": 3, "long": 12 + 13 + 12}


def test_somatic_fusions_cli_shim(tmp_path):
    cli.somatic_fusions(["--fusions", os.path.join(GOLD, "predictions.tsv"), "--barcodes", os.path.join(GOLD, "barcodes.tsv"), "--min_ac_reads", "3",
                         "--min_ac_cells", "2", "--max_MCF_noncancer", "0.1", "--deltaMCF", "0.3", "--outdir", str(tmp_path / "fusions")])
    for name in FUSION_FILES:
        assert read(str(tmp_path / name)) == read(os.path.join(GOLD, name)), name


def test_a_malformed_accession_is_an_error_naming_the_row(tmp_path):
    text = read(os.path.join(GOLD, "predictions.tsv")).decode().splitlines()
    text[3] = text[3].replace("C00^U2^read1", "C00^U2")                       # the C--D row (index 2 of the table)
    bad = tmp_path / "bad.tsv"
    bad.write_text("\n".join(text) + "\n")
    with pytest.raises(fusions.FusionInputError, match=r"row 2: accession 'C00\^U2' has 2"):
        fusions.fusion_report(str(bad), os.path.join(GOLD, "barcodes.tsv"), 3, 2, 0.1, 0.3, str(tmp_path / "x"))


def test_per_celltype_copy_stops_on_a_short_file(tmp_path, monkeypatch):
    """--per_celltype slices {id}.fastq by n_bytes: a file shorter than that is an error, not a loop"""
    real = hostio.bam_fastq

    def longer(*a, **k):
        info = real(*a, **k)
        info["n_bytes"][1] += 7
        return info
    monkeypatch.setattr(hostio, "bam_fastq", longer)
    with pytest.raises(RuntimeError, match="7 bytes shorter"):
        cli.fusion_fastq(["--bam", os.path.join(GOLD, "routed.bam"), "--meta", os.path.join(GOLD, "routed.meta.tsv"), "--id", "S", "--outdir", str(tmp_path),
                          "--min_MQ", "30", "--host", "--per_celltype"])


def test_number_duplicates():
    assert fusions.number_duplicates(["a", "b", "a", "c", "a", "b"]) == ["a1", "b1", "a2", "c", "a3", "b2"]


# ---- the scripts ------------------------------------------------------------------------------------------------------------------------------
def test_bam_to_fastq_shim_parses_the_reference_flag_line_and_prints_on_the_host(tmp_path, capsys):
    out = str(tmp_path / "o.fastq")
    cli.bam_to_fastq(["--bam", os.path.join(GOLD, "plain.bam"), "--fastq", out, "--host"])
    assert read(out) == read(os.path.join(GOLD, "plain.fastq"))
    assert '"printed_on": "host"' in capsys.readouterr().out


def test_fusion_fastq_script_on_the_host(tmp_path):
    cli.fusion_fastq(["--bam", os.path.join(GOLD, "routed.bam"), "--meta", os.path.join(GOLD, "routed.meta.tsv"), "--id", "S", "--outdir", str(tmp_path),
                      "--min_MQ", "30", "--max_nM=", "--max_NH=", "--host", "--per_celltype"])
    whole = read(str(tmp_path / "S.fastq"))
    assert whole == read(os.path.join(GOLD, "routed.fastq"))
    assert read(str(tmp_path / "S.Cancer.fastq")) + read(str(tmp_path / "S.Non-Cancer.fastq")) == whole
    assert b"^c1\n" in read(str(tmp_path / "S.Cancer.fastq")) and b"^n2\n" in read(str(tmp_path / "S.Non-Cancer.fastq"))


def test_shims_and_rules_exist():
    for name, entry in (("BamToFastq.py", "bam_to_fastq"), ("FusionCalling.py", "somatic_fusions"), ("longsom_gpu_fastq.py", "fusion_fastq")):
        text = read(os.path.join(ROOT, "workflow", "scripts_gpu", "FusionCalling", name)).decode()
        assert re.search(r"cli\.%s\(\)" % entry, text)
    rules = read(os.path.join(ROOT, "workflow", "rules", "FusionCalling.gpu.smk")).decode()
    assert re.findall(r"^rule (\w+):", rules, re.M) == ["FusionFastq_gpu", "BamToFastq", "SomaticFusions"]      # CTATFusion stays the reference's


def test_table_slot_is_appended():
    from longsom_amd.engine import Engine
    header = read(os.path.join(ROOT, "include", "longsom_hip.h")).decode()
    enum = re.search(r"enum lsg_table \{(.*?)\};", header, re.S).group(1)
    assert re.sub(r"\s", "", enum).endswith("LSG_TABLE_BNPC_VAF,LSG_TABLE_FASTQ,LSG_TABLE_SLOTS")
    assert Engine.TABLE_FASTQ == Engine.TABLE_BNPC_VAF + 1
