"""GPU: the beta-binomial fit on the device (csrc/bbfit.hip) against its numpy twin (longsom_amd/bbfit.py) and the likelihood's root at
50 digits: the pass over resident count rows (installed and counted ones, thinned and not), the solve from given histograms, and the
fused panel-of-normals run that fits its own alpha / beta.

Tolerances: histograms and row counts exactly; the solve within 1e-7 relative of the root (VGAM's epsilon, the precision to which the
reference fixes these numbers); the fused run's estimates within 1e-12 relative of the twin's solve over the same histograms."""
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from longsom_amd import _lib, bbfit, hostio, pipeline, synth
from longsom_amd._lib import CountParams
from longsom_amd.engine import Engine
from tests.support import bbfit_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 65 * 1024                  # above 2^16: a value of CAP - 1 needs 32-bit planes
LDS = 1024                       # csrc/bbfit.hip BB_LDS_BINS: values below it are binned in LDS, the others straight in HBM
CONTIG = 1 << 20


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def make_rows(n, seed, top):
    """n count rows at strictly ascending sites (runs of neighbours - whole 64-row units - and scattered ones), REF over the table's
    letters, N and R; depths on both sides of the LDS limit; with top: one kept row at DP = top (the last bin when top = CAP - 1)"""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(np.arange(1, 40 * n + 200), n, replace=False)) if n else np.zeros(0, np.int64)
    if n > 130:
        pos[:n // 2] = np.arange(1, n // 2 + 1)                  # neighbours: units of 63 and 64 rows
        pos = np.unique(pos)
        pos = np.concatenate([pos, pos[-1] + 1 + np.arange(n - len(pos))])
    counts = np.zeros((n, 42), np.uint32)
    refs = rng.choice(np.frombuffer(b"ACTGACTGACTGNR", np.uint8), n)
    dp = np.where(rng.random(n) < 0.3, rng.integers(LDS - 40, LDS + 400, n), rng.integers(5, 300, n))
    nc = np.minimum(dp, rng.integers(5, 200, n))
    counts[:, 0], counts[:, 1] = dp, nc
    counts[:, 2:8] = rng.integers(0, 3, (n, 6)) * (rng.random((n, 6)) < 0.08)
    counts[:, 10:16] = rng.integers(0, 40, (n, 6)) * (rng.random((n, 6)) < 0.08)
    counts[:, 8:10] = rng.integers(0, 5, (n, 2))                 # N and O: resident, never summed
    counts[:, 16:18] = rng.integers(0, 5, (n, 2))
    if top and n:
        i = n // 2
        refs[i] = ord("C")
        counts[i, :18] = 0
        counts[i, 0], counts[i, 1], counts[i, 3], counts[i, 11] = top, min(top, 70000), 0, 0
    return pos.astype(np.int64), refs.astype(np.uint8), counts


def twin_sum(tables, cap, sample_n=0, seed=1992):
    hist, seen, kept = np.zeros((6, cap), np.uint64), [], []
    for t, (_, refs, counts) in enumerate(tables):
        h, s, k = bbfit.histograms(refs, counts, cap, t, sample_n, seed)
        hist += h
        seen.append(s); kept.append(k)
    return hist, seen, kept


@pytest.mark.parametrize("n_ct", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_accumulate_installed_rows(eng, n, n_ct):
    """32-bit planes (lsg_load_counts installs wide rows), REF passed per row; the 64-row block edge, a partial last block, empty tables"""
    sizes = [n, n // 2, n][:n_ct]
    tables = [make_rows(m, 100 * n + ct, CAP - 1 if ct == 0 else 0) for ct, m in enumerate(sizes)]
    eng.set_contigs([CONTIG])
    eng.load_counts([t[0] for t in tables], [t[2] for t in tables])
    for sample_n in (0, 1000):
        want, seen, kept = twin_sum(tables, CAP, sample_n)
        eng.bbfit_reset(CAP)
        got = [eng.bbfit_accumulate(ct, ref=tables[ct][1], table=ct, sample_n=sample_n) for ct in range(n_ct)]
        assert got == list(zip(seen, kept))
        hist = eng.bbfit_fetch()
        assert np.array_equal(hist, want), [np.flatnonzero(hist[h] != want[h])[:5] for h in range(6)]
        if n == 4097:
            assert want[5, LDS:].sum() > 100 and want[5, :LDS].sum() > 100            # values on both sides of the LDS limit
            if sample_n:
                assert all(700 < s < 1300 for s in seen)                              # every table has more rows than sample_n: thinned to about it
            else:
                assert want[5, CAP - 1] == 1 and want[4, CAP - 1] == 1                # the last bin
        elif sample_n:
            assert seen == sizes                                                      # no table has more rows than sample_n: nothing thinned


def test_a_value_at_capacity_is_an_error(eng):
    pos, refs, counts = make_rows(200, 7, 0)
    counts[:, 0], counts[:, 1] = 200 + np.arange(200) % 50, 20
    refs[100] = ord("C")
    counts[100, :18] = 0
    counts[100, 0], counts[100, 1] = 1000, 1000
    eng.set_contigs([CONTIG])
    eng.load_counts([pos], [counts])
    eng.bbfit_reset(1001)
    assert eng.bbfit_accumulate(0, ref=refs)[0] == 200
    eng.bbfit_reset(1000)
    with pytest.raises(_lib.LsgError, match="value 1000 does not fit"):
        eng.bbfit_accumulate(0, ref=refs)
    with pytest.raises(_lib.LsgError, match="lsg_bbfit_reset"):                   # the histograms hold a part of that pass
        eng.bbfit_fetch()
    counts[5, 1] = 0
    eng.load_counts([pos], [counts])
    eng.bbfit_reset(CAP)
    with pytest.raises(_lib.LsgError, match="DP or NC zero"):
        eng.bbfit_accumulate(0, ref=refs)


def test_accumulate_counted_rows(eng):
    """the rows lsg_pileup_count leaves (16-bit planes where a unit allows them), REF from the resident reference"""
    model = synth.named("C1", n_reads=9000, n_genes=6, n_cb=40, snp_mod=90)
    cp = CountParams.longsom_defaults()
    eng.set_contigs(model.contig_len)
    eng.synth_reference(model.seed)
    eng.set_barcodes(model.celltype_of, 2)
    eng.synth_reads(model)
    rows, _ = eng.pileup_count(cp)
    assert min(rows) > 200
    tables = [eng.fetch_counts(ct) for ct in range(2)]
    for sample_n in (0, 150):
        want, seen, kept = twin_sum(tables, 2048, sample_n, seed=5)
        eng.bbfit_reset(2048)
        got = [eng.bbfit_accumulate(ct, table=ct, sample_n=sample_n, seed=5) for ct in range(2)]
        print(sample_n, rows, seen, kept)
        assert got == list(zip(seen, kept)) and 0 < sum(kept) <= sum(seen) <= sum(rows)
        assert np.array_equal(eng.bbfit_fetch(), want)
    # the same rows with their REF column passed give the same histograms
    eng.bbfit_reset(2048)
    for ct in range(2):
        eng.bbfit_accumulate(ct, ref=tables[ct][1], table=ct, sample_n=150, seed=5)
    assert np.array_equal(eng.bbfit_fetch(), want)
    eng.unload_reads()


def device_solve(eng, hist, max_iter=0):
    eng.bbfit_reset(hist.shape[1])
    eng.bbfit_add(hist)
    assert np.array_equal(eng.bbfit_fetch(), hist)
    return eng.bbfit_solve(max_iter)


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_solve_against_the_root_at_50_digits(eng, name):
    hist = cases.shape_hist(name)
    est, infos = device_solve(eng, hist)
    root = cases.shape_roots(name)                    # from the same histograms (mpmath), not from a run of the device
    err = cases.rel(est, root)
    print(name, est, root, err, infos)
    assert [i["status"] for i in infos] == [bbfit.CONVERGED] * 2
    assert err <= 1e-7
    again, infos2 = eng.bbfit_solve()
    assert np.array_equal(np.array(est).view(np.uint64), np.array(again).view(np.uint64)) and infos2 == infos
    eng.bbfit_add(np.zeros_like(hist))
    assert eng.bbfit_solve()[0] == est


def test_statuses(eng):
    cap = 4096
    sc = cases.status_cases(cap)
    good = np.zeros((3, cap), np.uint64)
    good[:, :1024] = cases.shape_hist("cells")[:3]
    for name, status in (("zero", bbfit.NO_FINITE_MAXIMUM), ("binomial", bbfit.NO_FINITE_MAXIMUM), ("empty", bbfit.NO_DATA)):
        est, infos = device_solve(eng, np.concatenate([sc[name], good]))
        assert infos[0]["status"] == status and infos[1]["status"] == bbfit.CONVERGED, (name, infos)
        with pytest.raises(bbfit.FitFailed, match="cell counts"):
            bbfit.device_solve(eng)
    assert np.isnan(est[0]) and np.isnan(est[1]) and infos[0]["iterations"] == 0
    est, infos = device_solve(eng, np.concatenate([good, good]), max_iter=1)
    assert [i["status"] for i in infos] == [bbfit.ITERATION_CAP] * 2 and [i["iterations"] for i in infos] == [1, 1]


def body(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("##fileDate=")]


def floats_of(path):
    head, line = open(path).read().split("\n")[:2]
    assert head == "alpha1\tbeta1\talpha2\tbeta2"
    return [float(x) for x in line.split("\t")]


def test_fused_run_says_when_the_normals_have_no_fit(eng, tmp_path):
    """the project's synthetic normals (tests/test_pon_gpu.py) carry one common mismatch rate: after the filter their counts are no
    more dispersed than a binomial's, the likelihood has no finite maximum, and the run says so instead of writing numbers"""
    normals = []
    for i, (seed_reads, snp_mod) in enumerate(((9000, 90), (7000, 120), (8000, 90))):
        m = synth.named("C1", n_reads=seed_reads, n_genes=6, n_cb=40, snp_mod=snp_mod)
        d = tmp_path / ("n%d" % i)
        os.makedirs(d)
        bam, fa, bct = str(d / "N.bam"), str(d / "ref.fa"), str(d / "barcodes.tsv")
        hostio.synth_bam(m, bam, fa)
        hostio.write_barcodes_tsv(bct, hostio.synth_barcodes(m), m.celltype_of, ["Epithelial", "Stromal"])
        normals.append(("N%d_Norm" % i, bam, bct))
    with pytest.raises(bbfit.FitFailed, match="cell counts.*no finite maximum"):
        pipeline.run_pon(normals, str(tmp_path / "n0" / "ref.fa"), str(tmp_path / "fit"), engine=eng, fit=True)
    assert not os.path.exists(str(tmp_path / "fit" / "PoN" / "PoN" / "BetaBinEstimates.txt"))
    assert not os.path.exists(str(tmp_path / "fit" / "PoN" / "PoN" / "PoN_LR.tsv"))


def test_fused_run_fits_its_own_parameters(eng, tmp_path):
    """three small normals whose sites have error rates of their own (cases.write_normal: beta-binomial by construction, so the fit exists)"""
    normals = []
    for i in range(3):
        d = tmp_path / ("n%d" % i)
        os.makedirs(d)
        bam, bct = str(d / "N.bam"), str(d / "barcodes.tsv")
        cases.write_normal(bam, str(d / "ref.fa"), bct, seed=31 + i, n_reads=400 - 50 * i)
        normals.append(("N%d_Norm" % i, bam, bct))
    ref = str(tmp_path / "n0" / "ref.fa")
    p = pipeline.pon_params(alpha1=1.0, beta1=1.0, alpha2=1.0, beta2=1.0)         # (not read under fit=True)
    out = pipeline.run_pon(normals, ref, str(tmp_path / "fit"), p, engine=eng, fit=True)
    assert out.estimates_path == str(tmp_path / "fit" / "PoN" / "PoN" / "BetaBinEstimates.txt")
    assert floats_of(out.estimates_path) == out.estimates

    # the twin over the three normals' fetched count rows
    cap = bbfit.capacity_for(p.max_depth)
    want = np.zeros((6, cap), np.uint64)
    for _, bam, bct in normals:
        res = pipeline.load_sample(bam, bct, ref, eng, p.min_mapping_quality)
        eng.set_barcodes(res.table.celltype_of, len(res.table.celltype_names))
        eng.pileup_count(p.count())
        for ct in range(len(res.table.celltype_names)):
            _, refs, counts = eng.fetch_counts(ct)
            want += bbfit.histograms(refs, counts, cap)[0]
    est, infos = bbfit.solve(want)
    bbfit.require_converged(infos)
    print(out.estimates, est, cases.rel(out.estimates, est))
    assert cases.rel(out.estimates, est) <= 1e-12

    # the panel is the one the plain run writes when given those estimates
    fitted = dataclasses.replace(p, alpha1=out.estimates[0], beta1=out.estimates[1], alpha2=out.estimates[2], beta2=out.estimates[3])
    plain = pipeline.run_pon(normals, ref, str(tmp_path / "plain"), fitted, engine=eng)
    assert plain.estimates is None and not os.path.exists(str(tmp_path / "plain" / "PoN" / "PoN" / "BetaBinEstimates.txt"))
    assert body(plain.pon) == body(out.pon) and out.n_sites == plain.n_sites > 0

    # two ranks on device 0 (gloo): the same two files
    tsv = tmp_path / "normals.tsv"
    tsv.write_text("".join("%s\t%s\t%s\n" % n for n in normals))
    script = os.path.join(ROOT, "workflow", "scripts_gpu", "PoN", "longsom_gpu_pon.py")
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    env = dict(os.environ, LSG_DIST_BACKEND="gloo", LSG_DIST_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        script, "--normals", str(tsv), "--ref", ref, "--outdir", str(tmp_path / "ranks"), "--fit"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert '"ranks": 2' in r.stdout
    assert open(tmp_path / "ranks" / "PoN" / "PoN" / "BetaBinEstimates.txt").read() == open(out.estimates_path).read()
    assert body(tmp_path / "ranks" / "PoN" / "PoN" / "PoN_LR.tsv") == body(out.pon)

    # the drop-in script over the count tables the run wrote, every site: the same four numbers
    lst = tmp_path / "BaseCellCounter_files.txt"
    tables = [os.path.join(str(tmp_path / "fit"), "PoN", "BaseCellCounter", n[0], "%s.%s.tsv" % (n[0], ct)) for n in normals for ct in ("Epithelial", "Stromal")]
    assert all(os.path.exists(t) for t in tables)
    lst.write_text("".join(t + "\n" for t in tables) + str(tmp_path / "missing.tsv") + "\n")          # (a path that does not exist is skipped, :186)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "workflow", "scripts_gpu", "PoN", "BetaBinEstimation.py"), "--in_tsv", str(lst),
                           "--outfile", str(tmp_path / "shim.txt"), "--n_sites", "0"], cwd=ROOT, stdout=subprocess.DEVNULL)
    assert floats_of(tmp_path / "shim.txt") == out.estimates
