"""GPU: the HCCV filter decided and printed on the device (csrc/hccv.hip) - an uploaded table against the host twin of the same row code
and the reference's own output, the row shapes its kernels care about, and the fused re-annotation run, where it reads the resident
step-2 text, against the same run with the filter on the host."""
import os

import pytest

from longsom_amd import hostio, pipeline, reanno, synth

from . import hccv_cases as hc

pytestmark = pytest.mark.gpu


def device_against_native(engine, tmp_path, name, args, text):
    """both forms over the same file: the same files (or the same exception), the same path taken; returns the device's report"""
    path = tmp_path / (name + ".tsv")
    path.write_text(text)
    rep_n, rep_d = {}, {}
    want = hc.run(reanno.hccv_filter_native, str(path), str(tmp_path / (name + ".native")), args, report=rep_n)
    got = hc.run(lambda *a, **k: reanno.hccv_filter_device(engine, *a, **k), str(path), str(tmp_path / (name + ".device")), args, report=rep_d)
    if isinstance(want, type) or isinstance(got, type):
        assert got == want, (name, got, want)
    else:
        for s in ("", "2", "3"):
            assert open(got + s).read() == open(want + s).read(), (name, ".HCCV.tsv" + s)
    assert rep_d["path"] == {"native": "device-uploaded", "fallback": "fallback"}[rep_n["path"]], (rep_d, rep_n)
    for k in ("rows_in", "rows_tsv2", "rows_tsv3", "rows_pass", "n_undecided", "first_undecided", "reason", "why"):
        assert rep_d.get(k) == rep_n.get(k), (name, k, rep_d, rep_n)
    return rep_d


@pytest.mark.parametrize("tag,args", hc.GOLDEN_ARGS)
def test_uploaded_table_equals_the_reference_output(engine, tmp_path, tag, args):
    rep = {}
    out = reanno.hccv_filter_device(engine, hc.STEP2, str(tmp_path / tag), *args, report=rep)
    assert rep["path"] == "device-uploaded" and rep["n_undecided"] == 0 and rep["rows_in"] == 565, rep
    for suffix in ("", "2", "3"):
        assert open(out + suffix).read() == open(os.path.join(hc.G, tag + ".HCCV.tsv" + suffix)).read(), "%s.HCCV.tsv%s differs" % (tag, suffix)


def test_uploaded_tables_of_golden_rows_equal_the_host_twin(engine, tmp_path):
    paths = [device_against_native(engine, tmp_path, name, args, text)["path"] for name, args, text in hc.seeded_tables(0)]
    assert paths[0] == "device-uploaded" and paths.count("device-uploaded") >= 2, paths


CASES = hc.hand_made() + hc.shapes()


@pytest.mark.parametrize("name,args,text", CASES, ids=[c[0] for c in CASES])
def test_uploaded_hand_made_rows_equal_the_host_twin(engine, tmp_path, name, args, text):
    rep = device_against_native(engine, tmp_path, name, args, text)
    assert rep["path"] == ("fallback" if name == "rows_0" else "device-uploaded"), rep
    if name == "short_rows":
        assert rep["rows_in"] == 700 and rep["rows_tsv3"] > 256 and 0 < rep["rows_pass"] < rep["rows_tsv3"] < rep["rows_tsv2"] < 700, rep


UNDECIDED = hc.undecided()


@pytest.mark.parametrize("name,args,text,ordinal,reason", UNDECIDED, ids=[c[0] for c in UNDECIDED])
def test_uploaded_undecided_tables_report_the_same_row(engine, tmp_path, name, args, text, ordinal, reason):
    rep = device_against_native(engine, tmp_path, name, args, text)
    assert rep["path"] == "fallback", rep
    if ordinal is not None:
        assert (rep["n_undecided"], rep["first_undecided"], rep["reason"]) == (1, ordinal, reason), rep


def test_cli_flag_device_writes_the_reference_files(tmp_path):
    from longsom_amd import cli
    cli.hccv(["--SNVs", hc.STEP2, "--outfile", str(tmp_path / "s"), "--min_dp", "50", "--deltaVAF", "0.2", "--deltaMCF", "0.25", "--clust_dist", "10000", "--device", "0"])
    for suffix in ("", "2", "3"):
        assert open(str(tmp_path / "s.HCCV.tsv") + suffix).read() == open(os.path.join(hc.G, "sample.HCCV.tsv" + suffix)).read()


def strip_date(path):
    return "\n".join(l for l in open(path).read().split("\n") if not l.startswith("##fileDate="))


def test_fused_run_filters_the_resident_text(engine, tmp_path, monkeypatch):
    """run_reannotation with the filter over the resident step-2 text against the same run with LONGSOM_HOST_HCCV=1 (reanno.hccv_filter over
    the file): the three HCCV files and every later file of the loop (the sample and parameters of test_reanno_pipeline_gpu.py)"""
    m = synth.named("C1", n_reads=30000, n_genes=12, n_cb=80, snp_mod=120)
    bam, fa, bct = str(tmp_path / "S1.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "barcodes.tsv")
    hostio.synth_bam(m, bam, fa)
    hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
    rp = pipeline.ReannoParams(chain=pipeline.SnvParams(min_ac_cells=2, min_ac_reads=3), hccv_min_depth=10, hccv_delta_vaf=0.05, hccv_delta_mcf=0.05,
                               hccv_clust_dist=5, chrm_contaminant="True", min_variants=2, min_fraction=0.2)
    outs = {}
    for how in ("device", "host"):
        monkeypatch.setenv("LONGSOM_HOST_HCCV", "1" if how == "host" else "0")
        outs[how] = pipeline.run_reannotation(bam, bct, fa, str(tmp_path / how), "S1", rp, pipeline.SnvParams(), engine=engine, pass1_step3=True)
    assert outs["device"].timings["hccv_path"] == "device-resident", (outs["device"].timings, outs["device"].pass1.hccv_report)
    assert outs["host"].timings["hccv_path"] == "host" and outs["host"].pass1.hccv == ""
    rep = outs["device"].pass1.hccv_report
    assert rep["n_undecided"] == 0 and rep["rows_pass"] >= 3 and rep["rows_in"] > rep["rows_tsv2"] >= rep["rows_tsv3"], rep
    assert outs["device"].pass2 is not None and 0 < outs["device"].n_cancer < outs["device"].n_cells_kept
    rels = ["CellTypeReannotation/HCCV/S1.HCCV.tsv", "CellTypeReannotation/HCCV/S1.HCCV.tsv2", "CellTypeReannotation/HCCV/S1.HCCV.tsv3",
            "CellTypeReannotation/HCCV/S1.SNVs.SingleCellGenotype.tsv", "CellTypeReannotation/ReannotatedCellTypes/S1.tsv"]
    for sub in ("CellTypeReannotation", "SNVCalling"):
        rels += [sub + "/" + r for r in ("BaseCellCounter/S1/S1.Cancer.tsv", "BaseCellCounter/S1/S1.Non-Cancer.tsv", "MergeCounts/S1.BaseCellCounts.AllCellTypes.tsv",
                                         "BaseCellCalling/S1.calling.step1.tsv", "BaseCellCalling/S1.calling.step2.tsv", "BaseCellCalling/S1.calling.step3.tsv",
                                         "BaseCellCalling/S1.calling.step3.unfiltered.tsv")]
    for rel in rels:
        assert strip_date(str(tmp_path / "device" / rel)) == strip_date(str(tmp_path / "host" / rel)), rel
