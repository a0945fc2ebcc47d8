"""CPU: what the device splitter (csrc/split.hip) adds to the surface that needs no GPU: cli.split_bam's --device flag, the host twin
untouched without it, the new exports and table constants.  On the GPU: tests/test_split_bam_gpu.py."""
import ctypes
import os
import re

import pytest

from longsom_amd import _lib, cli, engine as engine_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_the_parser_accepts_device(monkeypatch):
    import argparse
    seen = {}
    orig = argparse.ArgumentParser.parse_args

    def grab(self, args=None, namespace=None):
        seen["a"] = orig(self, args, namespace)
        raise SystemExit(0)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    for argv, want in ((["--bam", "b", "--meta", "m", "--device", "3"], 3), (["--bam", "b", "--meta", "m"], None)):
        with pytest.raises(SystemExit):
            cli.split_bam(argv)
        assert seen["a"].device == want


def test_without_device_no_engine_is_made(tmp_path, monkeypatch):
    """the host twin's path is what it was: no Engine, the reference's report"""
    def boom(*a, **k):
        raise AssertionError("cli.split_bam made an Engine without --device")
    monkeypatch.setattr(cli, "Engine", boom)
    cli.split_bam(["--bam", os.path.join(G, "readfilter.bam"), "--meta", os.path.join(G, "readfilter.barcodes.tsv"), "--id", "s", "--outdir", str(tmp_path),
                   "--min_MQ", "60", "--max_nM", "5"])
    head, row = open(tmp_path / "s.report.txt").read().rstrip("\n").split("\n")
    ghead, grow = open(os.path.join(G, "readfilter.nm.report.txt")).read().rstrip("\n").split("\n")
    assert head.split("\t")[:-1] == ghead.split("\t") and row.split("\t")[:-1] == grow.split("\t")
    assert os.path.getsize(tmp_path / "s.Cancer.bam") > 28


@pytest.mark.parametrize("rc,why", [(-4, "straddle"), (-3, "does not fit")])
def test_a_bam_the_device_cannot_take_goes_to_the_host_twin(tmp_path, monkeypatch, capsys, rc, why):
    """rc -4 (the record chain does not settle) and rc -3 (no device memory): said on stderr, then the host twin's files and report"""
    class NoRoom:
        TABLE_SPLIT_BAM = engine_mod.Engine.TABLE_SPLIT_BAM

        def __init__(self, device):
            assert device == 2

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def set_split_filters(self, filters):
            pass

        def split_bam(self, *a, **k):
            e = _lib.LsgError("lsg_split_bam failed (rc=%d)" % rc)
            e.rc = rc
            raise e
    monkeypatch.setattr(cli, "Engine", NoRoom)
    cli.split_bam(["--bam", os.path.join(G, "readfilter.bam"), "--meta", os.path.join(G, "readfilter.barcodes.tsv"), "--id", "s", "--outdir", str(tmp_path),
                   "--min_MQ", "60", "--max_nM", "5", "--device", "2"])
    err = capsys.readouterr().err
    assert why in err and "on the host" in err
    head, row = open(tmp_path / "s.report.txt").read().rstrip("\n").split("\n")
    ghead, grow = open(os.path.join(G, "readfilter.nm.report.txt")).read().rstrip("\n").split("\n")
    assert head.split("\t")[:-1] == ghead.split("\t") and row.split("\t")[:-1] == grow.split("\t")
    assert os.path.getsize(tmp_path / "s.Cancer.bam") > 28


def test_another_error_of_the_device_is_raised(tmp_path, monkeypatch):
    class Broken:
        def __init__(self, device):
            e = _lib.LsgError("lsg_create failed (rc=-1)")
            e.rc = -1
            raise e
    monkeypatch.setattr(cli, "Engine", Broken)
    with pytest.raises(_lib.LsgError):
        cli.split_bam(["--bam", os.path.join(G, "readfilter.bam"), "--meta", os.path.join(G, "readfilter.barcodes.tsv"), "--outdir", str(tmp_path), "--device", "0"])


def test_the_new_exports_and_tables():
    lib = ctypes.CDLL(os.path.join(ROOT, "longsom_amd", "lib", "liblongsom_hip.so"))
    for name in ("lsg_split_bam", "lsg_bgzf_compress"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "longsom_hip.h")).read(), flags=re.S)
    more = re.sub(r"\s", "", re.search(r"enum lsg_table_more \{(.*?)\}", header, re.S).group(1)).split(",")
    assert more[:6] == ["LSG_TABLE_GENE_COUNTS=LSG_TABLE_SLOTS", "LSG_TABLE_HCCV2", "LSG_TABLE_HCCV3", "LSG_TABLE_HCCV_PASS", "LSG_TABLE_STEP3_ALL", "LSG_TABLE_STEP3_PASS"]
    E = engine_mod.Engine
    assert E.TABLE_SPLIT_BAM == E.TABLE_STEP3_PASS + 1 and E.TABLE_BGZF == E.TABLE_SPLIT_BAM + _lib.MAX_CELLTYPES      # no earlier table moved
    assert ctypes.sizeof(_lib.SplitInfo) == 8 * (1 + 5 + 36 + 16 + 1) + 4 * 2 + 4 * 10
    text = open(os.path.join(ROOT, "include", "longsom_hip.h")).read()
    assert "SplitBamCellTypes.py:39-192" in text and "lsg_split_info" in text
