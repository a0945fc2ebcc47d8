"""CPU: the host half of step 2's gnomAD filter on the device (longsom_amd/calling.py): allele keys, a source's answers to a run's queries
(gnomad_hit_keys), prepared sets (write_gnomad_set / GnomadSet) and the flags that carry them."""
import json
import sqlite3

import numpy as np
import pytest

from longsom_amd import calling, cli

NAMES = ["chr1", "1", "chrM", "chr2_alt"]
ROWS = [("1", 100, "A", "G", 0.5), ("1", 100, "A", "C", 0.01), ("1", 101, "A", "C", 0.009999), ("1", 102, "T", "C", None), ("1", 103, "T", "C", 0.02),
        ("M", 7, "C", "T", 1.0), ("M", 8, "C", "TT", 0.9), ("M", 9, "CA", "T", 0.9), ("2_alt", 5, "G", "A", 0.3), ("chr2_alt", 6, "G", "A", 0.3), ("7", 5, "G", "A", 0.3)]


@pytest.fixture
def sqlite_dir(tmp_path):
    """a database laid out as the gnomad_db package's (test_rules_cpu.py::test_gnomad_sqlite_reader): chroms without "chr" """
    d = tmp_path / "gnomAD_v4.1"; d.mkdir()
    db = sqlite3.connect(str(d / "gnomad_db.sqlite3"))
    db.execute("CREATE TABLE gnomad_db (chrom TEXT, pos INTEGER, ref TEXT, alt TEXT, AF REAL, PRIMARY KEY (chrom, pos, ref, alt))")
    db.executemany("INSERT INTO gnomad_db VALUES (?,?,?,?,?)", ROWS)
    db.commit(); db.close()
    return str(d)


def queries():
    """every one-base allele of ROWS on every contig of NAMES, and alleles the database does not hold"""
    t, p, r, a = [], [], "", ""
    for tid in range(len(NAMES)):
        for pos in list(range(98, 106)) + [5, 6, 7, 8, 9]:
            for ref in "ACGT":
                for alt in "ACGT":
                    t.append(tid); p.append(pos); r += ref; a += alt
    return calling.pack_allele_keys(t, p, r, a)


def by_get(source, keys, gmax):
    tid, pos, ref, alt = calling.unpack_allele_keys(keys)
    hit = [calling.af_hits(source.get("%s:%d:%s:%s" % (NAMES[t], p, chr(r), chr(a)), 0.0), gmax) for t, p, r, a in zip(tid.tolist(), pos.tolist(), ref.tolist(), alt.tolist())]
    return np.unique(keys[np.asarray(hit, bool)])


def test_keys_round_trip_at_the_limits():
    tid = [0, 0, calling.ALLELE_MAX_TID - 1, calling.ALLELE_MAX_TID - 1, 5]
    pos = [0, calling.ALLELE_MAX_POS - 1, 0, calling.ALLELE_MAX_POS - 1, 123456789]
    k = calling.pack_allele_keys(tid, pos, "A\x00\xffTG".encode("latin-1"), [ord("C"), 255, 0, ord("G"), ord("N")])
    assert k.dtype == np.int64 and (k >= 0).all() and k[0] == (ord("A") << 8 | ord("C"))
    assert int(k[3]) == ((calling.ALLELE_MAX_TID - 1) << 48) | ((calling.ALLELE_MAX_POS - 1) << 16) | (ord("T") << 8) | ord("G")
    t, p, r, a = calling.unpack_allele_keys(k)
    assert t.tolist() == tid and p.tolist() == pos and r.tolist() == [65, 0, 255, 84, 71] and a.tolist() == [67, 255, 0, 71, 78]
    assert k[1] < k[4] < k[2]                                 # ordered by contig, then position, then REF, then ALT
    assert calling.pack_allele_keys([1], [7], "A", "C") < calling.pack_allele_keys([1], [7], "A", "G") < calling.pack_allele_keys([1], [7], "C", "A") < calling.pack_allele_keys([1], [8], "A", "A")
    for bad in (([calling.ALLELE_MAX_TID], [1]), ([0], [calling.ALLELE_MAX_POS]), ([-1], [1]), ([0], [-1])):
        with pytest.raises(ValueError):
            calling.pack_allele_keys(bad[0], bad[1], "A", "C")
    assert len(calling.pack_allele_keys([], [], "", "")) == 0
    assert calling.allele_keys_fit([10] * calling.ALLELE_MAX_TID) and not calling.allele_keys_fit([10] * (calling.ALLELE_MAX_TID + 1))
    assert calling.allele_keys_fit([calling.ALLELE_MAX_POS - 1]) and not calling.allele_keys_fit([calling.ALLELE_MAX_POS])


def test_a_number_at_or_above_the_threshold_hits():
    assert calling.af_hits(0.01, 0.01) and calling.af_hits(1, 0.01) and calling.af_hits(np.float64(0.5), 0.01)
    assert not calling.af_hits(float(np.nextafter(0.01, 0)), 0.01) and not calling.af_hits(None, 0.01) and not calling.af_hits(float("nan"), 0.01)
    assert not calling.af_hits(0.0, 0.01) and not calling.af_hits("0.5", 0.01)


@pytest.mark.parametrize("gmax", [0.01, 0.3, 1.0])
def test_hit_keys_equal_per_key_get(sqlite_dir, gmax):
    q = queries()
    src = calling.open_gnomad(sqlite_dir)
    want = by_get(src, q, gmax)
    got = calling.gnomad_hit_keys(src, NAMES, np.concatenate([q, q[:50]]), gmax)       # (repeated queries: the answer is a set)
    assert got.tolist() == want.tolist() and len(want) == {0.01: 8, 0.3: 4, 1.0: 1}[gmax]
    # "chr1" and "1" are the database's chrom "1" alike; "chr2_alt" is "2_alt", never the row stored as "chr2_alt"
    tid, pos, _, _ = calling.unpack_allele_keys(want)
    if gmax == 0.01:
        assert sorted(zip(tid.tolist(), pos.tolist())) == [(0, 100), (0, 100), (0, 103), (1, 100), (1, 100), (1, 103), (2, 7), (3, 5)]
    table = {"%s:%d:%s:%s" % ("chr" + c, p, r, a): af for c, p, r, a, af in ROWS}
    table["chr1:104:A:C"] = float("nan")
    assert calling.gnomad_hit_keys(table, NAMES, q, gmax).tolist() == by_get(table, q, gmax).tolist()
    assert len(calling.gnomad_hit_keys(table, NAMES, q, gmax)) > 0
    assert len(calling.gnomad_hit_keys(None, NAMES, q, gmax)) == 0 and len(calling.gnomad_hit_keys(src, NAMES, [], gmax)) == 0


def test_many_positions_are_asked_in_pieces(tmp_path):
    """more positions of one contig than one SELECT takes"""
    db = sqlite3.connect(str(tmp_path / "big.sqlite3"))
    db.execute("CREATE TABLE gnomad_db (chrom TEXT, pos INTEGER, ref TEXT, alt TEXT, AF REAL)")
    db.executemany("INSERT INTO gnomad_db VALUES (?,?,?,?,?)", [("1", p, "A", "C", 0.5 if p % 3 else None) for p in range(1, 1800, 2)] + [("1", 11, "A", "C", 0.0)])
    db.commit(); db.close()
    src = calling.open_gnomad(str(tmp_path / "big.sqlite3"))
    q = calling.pack_allele_keys(np.zeros(1799), np.arange(1, 1800), "A" * 1799, "C" * 1799)
    got = calling.gnomad_hit_keys(src, NAMES, q, 0.01)
    assert got.tolist() == by_get(src, q, 0.01).tolist() and len(got) > 500
    assert src.get("chr1:11:A:C") == src.get_many("chr1", [(11, "A", "C")])[0]       # an allele stored twice: whatever .get() sees


def test_a_prepared_set_answers_as_its_source(sqlite_dir, tmp_path):
    src = calling.open_gnomad(sqlite_dir)
    path = str(tmp_path / "alleles.npz")
    floor = 0.01
    n = calling.write_gnomad_set(src, path, floor)
    assert n == 7                                              # the NULL AF, the AF below the floor and the two multi-base alleles are not stored
    s = calling.open_gnomad(path)
    assert isinstance(s, calling.GnomadSet) and s.af_floor == floor and s.af.dtype == np.float64
    stored = set(zip(s.chrom.tolist(), s.pos.tolist()))
    assert ("M", 7) in stored and ("chr2_alt", 6) in stored and ("M", 8) not in stored and ("M", 9) not in stored and ("1", 101) not in stored and ("1", 102) not in stored
    q = queries()
    for gmax in (floor, 0.02, 0.3, 1.0):
        want = by_get(src, q, gmax)
        assert calling.gnomad_hit_keys(s, NAMES, q, gmax).tolist() == want.tolist()
        assert s.hit_keys(NAMES, gmax).tolist() == want.tolist()                      # (the queries hold every allele of the set on these contigs)
        assert by_get(s, q, gmax).tolist() == want.tolist()                           # the host's step 2 reads it through .get()
    with pytest.raises(calling.GnomadUnusable, match=r"0\.01.*0\.005|0\.005.*0\.01"):
        s.hit_keys(NAMES, 0.005)
    with pytest.raises(calling.GnomadUnusable):
        calling.step2("#CHROM\tStart\n", None, NAMES, [], [], [], 0, s, 0.001)
    # a JSON table is keyed by the run's own names: its set maps them as they are
    table = {"chr1:100:A:G": 0.5, "1:100:A:G": 0.5, "chrM:7:C:T": None, "chr1:100:A:GT": 0.9, "chr1:0101:A:C": 0.9}
    jpath = str(tmp_path / "json.npz")
    assert calling.write_gnomad_set(table, jpath, floor) == 2
    js = calling.open_gnomad(jpath)
    assert js.hit_keys(NAMES, floor).tolist() == by_get(table, q, floor).tolist() == calling.pack_allele_keys([0, 1], [100, 100], "AA", "GG").tolist()


def test_the_cli_prepares_a_set_and_the_fused_entries_take_it(sqlite_dir, tmp_path, capsys):
    out = str(tmp_path / "set.npz")
    cli.main(["gnomad_set", "--gnomAD_db", sqlite_dir, "--out", out, "--af_floor", "0.3"])
    said = json.loads(capsys.readouterr().out)
    assert said["alleles"] == 5 and said["af_floor"] == 0.3
    s = calling.open_gnomad(out)
    assert s.hit_keys(NAMES, 0.3).tolist() == by_get(calling.open_gnomad(sqlite_dir), queries(), 0.3).tolist()
    with pytest.raises(SystemExit):
        cli.main(["gnomad_set", "--gnomAD_db", sqlite_dir, "--out", str(tmp_path / "set.bin")])
    from tests.test_rules_cpu import parser_of
    for fn in (cli.snv, cli.reannotation):
        p = parser_of(fn)
        a = p.parse_args(["--bam", "b", "--meta", "m", "--ref", "r", "--id", "i", "--outdir", "o", "--gnomAD_db", "db", "--gnomAD_set", out])
        assert cli._gnomad_source(a) == out
        a = p.parse_args(["--bam", "b", "--meta", "m", "--ref", "r", "--id", "i", "--outdir", "o", "--gnomAD_db", "db", "--gnomAD_set"])
        assert cli._gnomad_source(a) == "db"


def test_a_table_keyed_by_alt_strings_keeps_the_host_path():
    assert calling.keyed_by_alleles({"chr1:5:A:C": 0.5}) and not calling.keyed_by_alleles({"chr1:5:A:C|G": 0.5}) and not calling.keyed_by_alleles({"chr1:5:A:C,C": 0.5})
