"""GPU: step 2's gnomAD filter on the device - the resident allele set (lsg_load_alleleset), its probe inside the step-2 table's printer
(csrc/tables.hip step1_row<STEP2>), lsg_probe_alleleset, lsg_step2_allele_queries and the fused chain with a gnomAD source - against the
reference's golden step-2 table (written with its gnomAD filter on) and against calling.step2, the host's row-by-row step 2."""
import json
import os
import sqlite3

import numpy as np
import pytest

from longsom_amd import calling, tsvio
from tests.support import step2_gnomad_cases as cases

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MAX = 0.01


def head_of(ct_names):
    return tsvio.step1_header(["##fileDate=01/01/2000\n"], ct_names).encode()


def host_step2(engine, names, ct_names, kept: bytes, possets, af) -> bytes:
    """the whole step-2 table as calling.step2 writes it from the kept rows' text (loads the position sets)"""
    return calling.step2((head_of(ct_names) + kept).decode(), engine, names, possets[0], possets[1], possets[2], 0, af, MAX).encode()


def rows_of(table: bytes) -> bytes:
    return b"".join(l + b"\n" for l in table.split(b"\n") if l and not l.startswith(b"#"))


def device_step2(engine) -> bytes:
    return engine.table_bytes(engine.TABLE_STEP2, engine.format_table(engine.TABLE_STEP2))


def kept_rows(engine) -> bytes:
    text = engine.table_bytes(engine.TABLE_STEP1_KEPT, engine.format_table(engine.TABLE_STEP1_KEPT))
    engine.free_table(engine.TABLE_STEP1_KEPT)
    return text


def fields(text: bytes):
    return [l.split("\t") for l in text.decode().split("\n") if l and not l.startswith("#")]


def allele_of(row) -> str:
    return "%s:%s:%s:%s" % (row[0], row[1], row[3], row[4])


def set_of(af: dict, names) -> np.ndarray:
    """every one-base allele of a JSON table that step 2 would tag, as sorted keys - whether a row of the run asks for it or not"""
    tid_of = {n: i for i, n in enumerate(names)}
    hit = [k.split(":") for k, v in af.items() if calling.af_hits(v, MAX)]
    hit = [(tid_of[c], int(p), r, a) for c, p, r, a in hit if c in tid_of and len(r) == 1 and len(a) == 1]
    if not hit:
        return np.zeros(0, np.int64)
    return np.unique(calling.pack_allele_keys([h[0] for h in hit], [h[1] for h in hit], "".join(h[2] for h in hit), "".join(h[3] for h in hit)))


def table_of(keys, names) -> dict:
    """an allele set as the JSON table that tags exactly its alleles"""
    tid, pos, ref, alt = calling.unpack_allele_keys(keys)
    return {"%s:%d:%s:%s" % (names[t], p, chr(r), chr(a)): 0.5 for t, p, r, a in zip(tid.tolist(), pos.tolist(), ref.tolist(), alt.tolist())}


def host_queries(kept: bytes, names) -> np.ndarray:
    tid_of = {n: i for i, n in enumerate(names)}
    one = [r for r in fields(kept) if len(r[4]) == 1]
    if not one:
        return np.zeros(0, np.int64)
    return calling.pack_allele_keys([tid_of[r[0]] for r in one], [int(r[1]) for r in one], "".join(r[3] for r in one), "".join(r[4] for r in one))


def install_golden(engine):
    names, seqs = tsvio.read_fasta(os.path.join(G, "calling.ref.fa"))
    engine.set_contigs([len(s) for s in seqs])
    for t, s in enumerate(seqs):
        engine.load_reference(t, s)
    per_ct = [tsvio.parse_counts_tsv(os.path.join(G, "counts.sample.%s.tsv" % ct), names)[:3] for ct in ("Cancer", "Non-Cancer")]
    engine.load_counts([p[0] for p in per_ct], [p[2] for p in per_ct])
    engine.call_step1()
    engine.set_table_names(names, ["Cancer", "Non-Cancer"])
    return names


@pytest.fixture
def installed(engine):
    """the edge cases' sites (tests/support/step2_gnomad_cases.py) counted, called and named; no position set, no allele set"""
    engine.set_contigs(cases.LENS)
    for t, s in enumerate(cases.sequences()):
        engine.load_reference(t, s)
    rows = cases.count_rows()
    engine.load_counts([k for k, _ in rows], [c for _, c in rows])
    engine.call_step1()
    engine.set_table_names(cases.NAMES, cases.CT_NAMES)
    for kind in range(3):
        engine.load_posset(kind, np.zeros(0, np.int64))
    engine.load_alleleset(None)
    yield engine
    engine.load_alleleset(None)
    engine.free_table()


def test_the_reference_s_step2_table_with_its_gnomad_filter_on(engine):
    """the golden counts called on the device, the three golden position sets and the allele set of calling.gnomad_af.json at 0.01 resident:
    TABLE_STEP2 is the body of the table the reference wrote with its gnomAD filter on"""
    golden = open(os.path.join(G, "sample.calling.step2.tsv"), "rb").read()
    want = fields(golden)
    assert sum("gnomAD" in r[5] for r in want) >= 10                               # 14
    assert sum(len(r[4]) == 1 and "gnomAD" not in r[5] for r in want) >= 100       # 285
    assert sum(len(r[4]) > 1 for r in want) >= 100                                 # 266
    names = install_golden(engine)
    try:
        for kind, k in enumerate(("editing", "pon_SR", "pon_LR")):
            engine.load_posset(kind, calling.read_posset_keys(os.path.join(G, "calling.%s.tsv" % k), names))
        af = json.load(open(os.path.join(G, "calling.gnomad_af.json")))
        queries = engine.step2_allele_queries()
        assert queries.tolist() == host_queries(kept_rows(engine), names).tolist() and len(queries) == sum(len(r[4]) == 1 for r in want)
        engine.load_alleleset(calling.gnomad_hit_keys(af, names, queries, MAX))
        assert device_step2(engine) == rows_of(golden)
        engine.load_alleleset(set_of(af, names))          # (the alleles no row asks for change nothing)
        assert device_step2(engine) == rows_of(golden)
    finally:
        engine.load_alleleset(None)
        engine.free_table()


def test_the_rule_s_edges(installed):
    """AF at the threshold and one float below it, AF absent / None / NaN, another alt or another ref at the position, "A|C" and "A,A"
    rows whose single alleles are in the set, a hit on a bare PASS, a hit behind two position-set tags, a hit at the last position of
    the last contig; every expectation is calling.step2's over the kept rows' text, and step2_summary's survivors are
    calling._step3_survivors' of that text"""
    eng = installed
    kept = kept_rows(eng)
    rows = fields(kept)
    passes = [r for r in rows if len(r[4]) == 1 and r[5] == "PASS" and r[0] != "chrM" and r[6] == "Cancer"]      # (rows step 3 can keep)
    other = [r for r in rows if len(r[4]) == 1 and r[5] not in ("PASS",) and r[0] != "chrM"]
    bars = [r for r in rows if "|" in r[4]]
    commas = [r for r in rows if "," in r[4]]
    last = [r for r in rows if r[0] == cases.NAMES[-1] and int(r[1]) == cases.LENS[-1]]
    assert len(passes) >= 9 and len(other) >= 2 and bars and commas and len(last) == 1 and len(last[0][4]) == 1
    at_max, below, none, nan, absent, other_alt, other_ref, tagged_pass, behind = passes[:9]
    af = {allele_of(at_max): MAX, allele_of(below): float(np.nextafter(MAX, 0.0)), allele_of(none): None, allele_of(nan): float("nan"),
          allele_of(tagged_pass): 0.5, allele_of(behind): 0.02, allele_of(other[0]): 1.0, allele_of(last[0]): 0.3}
    wrong_alt = next(b for b in "ACGT" if b not in (other_alt[3], other_alt[4]))
    af["%s:%s:%s:%s" % (other_alt[0], other_alt[1], other_alt[3], wrong_alt)] = 0.5
    wrong_ref = next(b for b in "ACGT" if b not in (other_ref[3], other_ref[4]))
    af["%s:%s:%s:%s" % (other_ref[0], other_ref[1], wrong_ref, other_ref[4])] = 0.5
    for r in (bars[0], commas[0]):
        for base in set(r[4]) - set("|,"):
            af["%s:%s:%s:%s" % (r[0], r[1], r[3], base)] = 0.9
    tid_of = {n: i for i, n in enumerate(cases.NAMES)}
    behind_key = np.asarray([(tid_of[behind[0]] << 32) | int(behind[1])], np.int64)
    possets = [behind_key, behind_key, np.zeros(0, np.int64)]
    want = host_step2(eng, cases.NAMES, cases.CT_NAMES, kept, possets, af)
    by = {(r[0], r[1]): r[5] for r in fields(want)}
    flt = lambda r: by[(r[0], r[1])]
    assert flt(at_max) == "gnomAD" and flt(tagged_pass) == "gnomAD" and flt(last[0]).endswith("gnomAD")
    assert all(flt(r) == "PASS" for r in (below, none, nan, absent, other_alt, other_ref))
    assert flt(behind) == "RNA_editing_db,PoN_SR,gnomAD" and flt(other[0]) == other[0][5] + ",gnomAD"
    assert flt(bars[0]) == bars[0][5] and flt(commas[0]) == commas[0][5]
    keys = set_of(af, cases.NAMES)
    assert len(keys) >= 10
    eng.load_alleleset(keys)
    assert device_step2(eng) == rows_of(want)
    cols = head_of(cases.CT_NAMES).decode().split("\n")[-2].split("\t")
    kinds, n_surv = eng.step2_summary(len(cols))
    surv = eng.table_bytes(eng.TABLE_STEP3_ROWS, n_surv)
    assert surv == calling._step3_survivors(want, 6)
    gone = [r for r in (at_max, tagged_pass, behind, last[0])]
    assert all(("%s\t%s\t" % (r[0], r[1])).encode() not in surv for r in gone) and ("%s\t%s\t" % (below[0], below[1])).encode() in surv
    # the set made of the source's answers to the run's own queries prints the same table
    eng.load_alleleset(calling.gnomad_hit_keys(af, cases.NAMES, eng.step2_allele_queries(), MAX))
    assert device_step2(eng) == rows_of(want)


@pytest.mark.parametrize("size", [0, 1, 2, 1000])
def test_set_sizes_with_hits_at_both_ends(installed, size):
    """sets of 0, 1, 2 and 1 000 keys whose first and last key are alleles of the run's rows (the smallest and the largest query),
    the keys between them alleles no row prints"""
    eng = installed
    kept = kept_rows(eng)
    queries = np.sort(eng.step2_allele_queries())
    ends = {0: [], 1: [queries[-1]]}.get(size, [queries[0], queries[-1]])
    # (contig 1's alleles lie between contig 0's and contig 2's; a lower-case ALT is one no row prints)
    filler = np.unique(calling.pack_allele_keys(np.full(70 * 16, 1), np.repeat(np.arange(1, 71), 16), "ACGT" * 280, "aaaaccccggggtttt" * 70))
    assert len(filler) == 70 * 16 and (queries[0] >> 48) == 0 and (queries[-1] >> 48) == 2
    keys = np.unique(np.concatenate([np.asarray(ends, np.int64), filler[:max(0, size - 2)]]))
    assert len(keys) == size and (size < 2 or (keys[0] == queries[0] and keys[-1] == queries[-1]))
    want = host_step2(eng, cases.NAMES, cases.CT_NAMES, kept, [np.zeros(0, np.int64)] * 3, table_of(keys, cases.NAMES))
    assert rows_of(want).count(b"gnomAD") == min(size, 2)
    eng.load_alleleset(keys)
    assert device_step2(eng) == rows_of(want)
    assert eng.probe_alleleset(queries).tolist() == np.isin(queries, keys).astype(np.uint8).tolist()


def test_a_set_unloaded_leaves_the_table_as_it_was(installed):
    eng = installed
    before = device_step2(eng)
    assert b"gnomAD" not in before and before == rows_of(host_step2(eng, cases.NAMES, cases.CT_NAMES, kept_rows(eng), [np.zeros(0, np.int64)] * 3, None))
    with pytest.raises(RuntimeError, match="no allele set"):
        eng.probe_alleleset(np.zeros(1, np.int64))
    eng.load_alleleset(np.sort(eng.step2_allele_queries())[::2])
    tagged = device_step2(eng)
    assert tagged.count(b"gnomAD") == (len(eng.step2_allele_queries()) + 1) // 2 > 10
    eng.load_alleleset(None)
    assert device_step2(eng) == before
    eng.load_alleleset(np.zeros(0, np.int64))                # the empty set: a source that hits nothing
    assert device_step2(eng) == before and eng.probe_alleleset(np.zeros(3, np.int64)).tolist() == [0, 0, 0]


def test_probe_alleleset_against_numpy(engine):
    rng = np.random.default_rng(31)
    def draw(n):
        return calling.pack_allele_keys(rng.integers(1, 40, n), rng.integers(5, 3000, n), rng.choice(np.frombuffer(b"ACGT", np.uint8), n), rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    keys = np.unique(draw(1100))[:1000]
    assert len(keys) == 1000
    below = calling.pack_allele_keys([0, 0, 1], [1, 4000, 4], "AAA", "CCC")
    above = calling.pack_allele_keys([40, 32767, 39], [5, (1 << 32) - 1, 3000], "TTT", "GGG")
    q = np.concatenate([rng.choice(keys, 4000), draw(5994), below, above])
    assert len(q) == 10_000 and (below < keys[0]).all() and (above > keys[-1]).all()
    try:
        engine.load_alleleset(keys)
        hits = engine.probe_alleleset(q)
    finally:
        engine.load_alleleset(None)
    want = np.isin(q, keys)
    assert 4000 <= want.sum() < 10_000 and hits.tolist() == want.astype(np.uint8).tolist()


def test_allele_queries_are_the_one_base_rows_of_the_kept_table_in_its_order(installed):
    eng = installed
    got = eng.step2_allele_queries()
    want = host_queries(kept_rows(eng), cases.NAMES)
    assert len(want) >= 40 and got.tolist() == want.tolist()
    tids = (got >> 48).tolist()                              # table order is the contig names' string order, not the index order
    assert [t for i, t in enumerate(tids) if i == 0 or tids[i - 1] != t] == [1, 0, 2]
    # none: rows that carry the reference base alone
    seqs = cases.sequences()
    keys = np.asarray([(t << 32) | p for t in range(3) for p in range(10, 40, 4)], np.int64)
    cls = {ord("A"): 0, ord("C"): 1, ord("T"): 2, ord("G"): 3}
    rows = np.stack([cases._row(cls[int(seqs[int(k >> 32)][int(k & 0xFFFFFFFF)])], 40, []) for k in keys])
    eng.load_counts([keys, keys], [rows, rows])
    n_sites, n_cand = eng.call_step1()
    assert n_sites == len(keys) and kept_rows(eng) == b""
    assert len(eng.step2_allele_queries()) == 0


# ---- the chain ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample(engine, tmp_path_factory):
    """test_tables_gpu.py's chain sample (C2's model, 200 k reads in a synthetic BAM) resident, its chain run once without a source, and a
    gnomAD table over the one-base rows that run kept: every fifth above the threshold, others below it, None or on another alt"""
    from longsom_amd import hostio, pipeline, synth
    tmp = tmp_path_factory.mktemp("gnomad_chain")
    m = synth.named("C2", n_reads=200_000)
    bam, fa, bct = str(tmp / "S.bam"), str(tmp / "ref.fa"), str(tmp / "bc.tsv")
    hostio.synth_bam(m, bam, fa)
    hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Cancer", "Non-Cancer"])
    params = pipeline.SnvParams()
    res = pipeline.load_sample(bam, bct, fa, engine, params.min_mapping_quality, count_params=params.count())

    def chain(name, source=None):
        return pipeline.run_chain(res, res.table.celltype_of, res.table.celltype_names, res.dec.report, str(tmp / name), "S", params, gnomad_af_json=source)
    base = chain("base")
    one = [r for r in fields(open(base.step2, "rb").read()) if len(r[4]) == 1]
    assert len(one) > 500
    af = {}
    for i, r in enumerate(one):
        if i % 5 == 0:
            af[allele_of(r)] = 0.25 if i % 10 else MAX
        elif i % 5 == 1:
            af[allele_of(r)] = 0.001
        elif i % 5 == 2:
            af[allele_of(r)] = None
        elif i % 5 == 3:
            af["%s:%s:%s:%s" % (r[0], r[1], r[3], "N")] = 0.5
    srcs = {"json": str(tmp / "af.json")}
    json.dump(af, open(srcs["json"], "w"))
    d = tmp / "gnomAD_v4.1"; d.mkdir()
    db = sqlite3.connect(str(d / "gnomad_db.sqlite3"))
    db.execute("CREATE TABLE gnomad_db (chrom TEXT, pos INTEGER, ref TEXT, alt TEXT, AF REAL, PRIMARY KEY (chrom, pos, ref, alt))")
    db.executemany("INSERT INTO gnomad_db VALUES (?,?,?,?,?)", [(k.split(":")[0][3:] if k.startswith("chr") else k.split(":")[0], int(k.split(":")[1]), k.split(":")[2], k.split(":")[3], v)
                                                                 for k, v in af.items()])
    db.commit(); db.close()
    srcs["sqlite"] = str(d)
    srcs["set"] = str(tmp / "alleles.npz")
    assert calling.write_gnomad_set(calling.open_gnomad(srcs["sqlite"]), srcs["set"], 0.005) == sum(1 for i in range(len(one)) if i % 5 == 0) + sum(1 for i in range(len(one)) if i % 5 == 3)
    yield chain, base, srcs, sum(1 for i in range(len(one)) if i % 5 == 0)
    engine.load_alleleset(None)
    engine.unload_reads()


@pytest.mark.parametrize("kind", ["json", "sqlite", "set"])
def test_the_chain_with_a_gnomad_source_writes_the_host_path_s_files(sample, monkeypatch, kind):
    """run_chain with a JSON table, a gnomad_db sqlite and a prepared set made from it: step 2 stays on the device and leaves, byte for byte,
    the step-2 and step-3 files of the run whose step 2 is the host's (LONGSOM_HOST_STEP2=1); the run after it on the same engine,
    without a source, writes no gnomAD tag"""
    chain, base, srcs, n_tagged = sample
    monkeypatch.setenv("LONGSOM_HOST_STEP2", "1")
    host = chain("host_" + kind, srcs[kind])
    monkeypatch.delenv("LONGSOM_HOST_STEP2")
    dev = chain("dev_" + kind, srcs[kind])
    assert "step2_gnomad" in dev.timings and "step2_gnomad" not in host.timings
    for name in ("step2", "step3", "step3_unfiltered"):
        want = open(getattr(host, name), "rb").read()
        assert len(want) > 200 and open(getattr(dev, name), "rb").read() == want, name
    tagged = [r for r in fields(open(dev.step2, "rb").read()) if "gnomAD" in r[5]]
    assert len(tagged) == n_tagged >= 100
    assert open(dev.step3_unfiltered, "rb").read() != open(base.step3_unfiltered, "rb").read()
    after = chain("after_" + kind)
    assert "step2_gnomad" not in after.timings
    for name in ("step2", "step3", "step3_unfiltered"):
        assert open(getattr(after, name), "rb").read() == open(getattr(base, name), "rb").read(), name
    assert b"gnomAD" not in rows_of(open(after.step2, "rb").read())
