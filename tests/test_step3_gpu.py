"""GPU: step 3's final filters decided and printed on the device (csrc/step3.hip) - an uploaded table against the reference's own output and
against the host twin of the same row code, the row shapes its kernels care about, the fused run, where it reads the rows
lsg_step2_summary left resident, against the same run with step 3 on the host, and the script's --device flag."""
import os

import pytest

from longsom_amd import calling, hostio, pipeline, synth

from . import step3_cases as sc

pytestmark = pytest.mark.gpu

COUNTS = ("rows_in", "rows_all", "rows_pass", "rows_pass_unclustered", "n_clustered", "n_undecided", "first_undecided", "reason", "why")


def device_against_native(engine, tmp_path, name, args, text):
    """both forms over the same file: the same files (or the same exception), the same counts, the same path taken; returns the device's report"""
    (tmp_path / (name + ".tsv")).write_text(text)
    rep_n, rep_d = {}, {}
    want = sc.run_files(calling.step3_native, tmp_path, name, "native", args, report=rep_n)
    got = sc.run_files(lambda *a, **k: calling.step3_device(engine, *a, **k), tmp_path, name, "device", args, report=rep_d)
    if isinstance(want, type) or isinstance(got, type):
        assert got == want, (name, got, want)
    else:
        assert got[1] == want[1], (name, "unfiltered")
        assert got[0] == want[0], (name, "final")
    assert rep_d["path"] == {"native": "device-uploaded", "fallback": "fallback"}[rep_n["path"]], (rep_d, rep_n)
    for k in COUNTS:
        assert rep_d.get(k) == rep_n.get(k), (name, k, rep_d, rep_n)
    return rep_d


@pytest.mark.parametrize("prefix,args", sc.GOLDENS)
def test_uploaded_golden_equals_the_reference_output(engine, tmp_path, prefix, args):
    rep = {}
    final, unfiltered = calling.step3_device(engine, os.path.join(sc.G, prefix + ".calling.step2.tsv"), str(tmp_path / "f.tsv"), str(tmp_path / "u.tsv"), *args, report=rep)
    assert rep["path"] == "device-uploaded" and rep["n_undecided"] == 0 and rep["rows_in"] == 565 and rep["n_clustered"] > 0, rep
    assert open(unfiltered).read() == sc.rd(prefix + ".calling.step3.unfiltered.tsv")
    assert open(final).read() == sc.rd(prefix + ".calling.step3.tsv")


@pytest.fixture(scope="module")
def replicated():
    return sc.replicated_tables()


@pytest.mark.parametrize("which", [0, 1], ids=["30k_rows", "one_cell_type"])
@pytest.mark.parametrize("clust", [10000, 150, 1])
def test_uploaded_replicated_tables_equal_the_host_twin(engine, tmp_path, replicated, which, clust):
    rep = device_against_native(engine, tmp_path, "t%d" % which, (0.05, 0.3, 3, 2, clust), replicated[which])
    assert rep["path"] == "device-uploaded" and rep["rows_all"] > rep["rows_pass"] > 256, rep


CASES = sc.hand_made() + sc.decided_oddities() + sc.shapes()


@pytest.mark.parametrize("name,args,text", CASES, ids=[c[0] for c in CASES])
def test_uploaded_hand_made_rows_equal_the_host_twin(engine, tmp_path, name, args, text):
    rep = device_against_native(engine, tmp_path, name, args, text)
    assert rep["path"] == "device-uploaded", rep
    if name in ("rows_0", "no_survivors"):
        assert rep["rows_all"] == 0 and open(str(tmp_path / (name + ".device.step3.tsv"))).read().endswith("\tSTEP3FILTER\tINDEX\n"), rep
    if name == "short_rows":
        assert rep["rows_in"] == 702 and rep["rows_pass"] > 256 and rep["rows_all"] - rep["rows_pass"] > 100 and rep["n_clustered"] == 2, rep
    if name == "chrm_in_the_middle":
        chroms = [l.split("\t")[0] for l in open(str(tmp_path / (name + ".device.step3.unfiltered.tsv"))).read().split("\n") if l and not l.startswith("#")]
        assert chroms == ["chr1"] * 3 + ["chr2"] + ["chr1"] * 2 + ["chrM"] * 2, chroms


UNDECIDED = sc.undecided()


@pytest.mark.parametrize("name,args,text,why,ordinal,reason", UNDECIDED, ids=[c[0] for c in UNDECIDED])
def test_uploaded_undecided_tables_report_the_same_row(engine, tmp_path, name, args, text, why, ordinal, reason):
    rep = device_against_native(engine, tmp_path, name, args, text)
    assert rep["path"] == "fallback", rep
    if ordinal is not None:
        assert (rep["first_undecided"], rep["reason"]) == (ordinal, reason), rep


def test_cli_flag_device_writes_the_reference_files(tmp_path):
    from longsom_amd import cli
    cli.calling_step3(["--infile", os.path.join(sc.G, "sample.calling.step2.tsv"), "--outfile", str(tmp_path / "s"), "--deltaVAF", "0.05", "--deltaMCF", "0.3",
                       "--min_ac_reads", "3", "--min_ac_cells", "2", "--clust_dist", "10000", "--device", "0"])
    for suffix in (".calling.step3.tsv", ".calling.step3.unfiltered.tsv"):
        assert open(str(tmp_path / "s") + suffix).read() == sc.rd("sample" + suffix)


def strip_date(path):
    return "\n".join(l for l in open(path).read().split("\n") if not l.startswith("##fileDate="))


def test_fused_run_filters_the_resident_rows(engine, tmp_path, monkeypatch):
    """run_snv with step 3 over the resident survivors against the same run with LONGSOM_HOST_STEP3=1 (calling.step3 over the rows copied
    back): every file of the run (the sample of test_hccv_gpu.py; a cluster distance of 5, at which the host path alone keeps PASS rows)"""
    m = synth.named("C1", n_reads=30000, n_genes=12, n_cb=80, snp_mod=120)
    bam, fa, bct = str(tmp_path / "S1.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "barcodes.tsv")
    hostio.synth_bam(m, bam, fa)
    hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
    params = pipeline.SnvParams(min_ac_cells=2, min_ac_reads=3, clust_dist=5)
    outs = {}
    for how in ("host", "device"):
        monkeypatch.setenv("LONGSOM_HOST_STEP3", "1" if how == "host" else "0")
        outs[how] = pipeline.run_snv(bam, bct, fa, str(tmp_path / how), "S1", params=params, engine=engine)
    host_rows = [l.split("\t") for l in open(outs["host"].step3_unfiltered).read().split("\n") if l and not l.startswith("#")]
    assert any(r[-2] == "PASS" for r in host_rows) and any(r[-2] != "PASS" for r in host_rows), "the host path alone must show both kinds of row"
    assert outs["host"].step3_path == "host"
    assert outs["device"].step3_path == "device-resident", (outs["device"].timings, outs["device"].step3_report)
    rep = outs["device"].step3_report
    assert rep["n_undecided"] == 0 and rep["rows_pass"] >= 1 and rep["rows_all"] > rep["rows_pass"], rep
    assert rep["rows_all"] == len(host_rows)
    d, h = outs["device"], outs["host"]
    pairs = [(d.merged, h.merged), (d.step1, h.step1), (d.step2, h.step2), (d.step3, h.step3), (d.step3_unfiltered, h.step3_unfiltered)]
    pairs += [(d.counts[k], h.counts[k]) for k in sorted(h.counts)]
    for a, b in pairs:                                  # (every table; the split's report holds the run's time)
        assert strip_date(a) == strip_date(b), a
