"""BnpC's posterior estimate without a device: longsom_amd.bnpc's numpy twin, its chain and file functions and the rule's script against
goldens the reference's own libs/utils.py and libs/dpmmIO.py produced (tools/make_bnpc_estimate_goldens.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from longsom_amd import bnpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCRIPT = os.path.join(ROOT, "workflow", "scripts_gpu", "CellClustering", "run_BnpC.py")
CASES = ["n2s1", "n3s2", "n63s33", "n64s257", "n65s2", "n130s9", "n130one", "n130cells", "sep", "together", "real"]
FILES = (("assignment.txt", "assignment.txt"), ("errors.txt", "errors.txt"), ("genotypes_posterior_mean.tsv", "genotypes.tsv"),
         ("genotypes_cont_posterior_mean.tsv", "genotypes_cont.tsv"))


def gold(case):
    with np.load(os.path.join(GOLD, "bnpcest.%s.npz" % case)) as z:
        g = {k: z[k] for k in z.files}
    g["forced"] = g["forced"] if g["forced"].size else None
    return g


def chains(case):
    return bnpc.load_chains(os.path.join(GOLD, "bnpcest.%s.chains.npz" % case))


def check_mean_params(g, params, branch, n_used):
    """bit-equal where the reference adds sample by sample; where it sums through np.dot (branch 2) within the worst-case bound for two
    summation orders of S x cells non-negative terms, 4 (S cells) 2^-53 relative"""
    assert np.array_equal(branch, g["branch"]) and np.array_equal(n_used, g["n_used"])
    S = g["concat_assignments"].shape[0]
    clusters = np.unique(g["assignment"])
    for k, b in enumerate(g["branch"]):
        if b != 2:
            assert np.array_equal(params[k], g["params"][k]), "cluster %d (branch %d)" % (k, b)
        else:
            cells = int(np.count_nonzero(g["assignment"] == clusters[k]))
            bound = 4 * S * cells * 2.0 ** -53
            assert np.all(np.abs(params[k] - g["params"][k]) <= bound * np.abs(g["params"][k])), "cluster %d (branch 2)" % k


def check_estimate(g, est, info):
    if g["forced"] is None:
        assert np.array_equal(info["D"], g["D"]) and info["D"].dtype == np.uint32
        assert np.array_equal(info["dist"], g["dist"])
        assert np.array_equal(info["n_range"], g["n_range"])
        assert info["n"] == int(g["best_n"])
        assert np.allclose(info["scores"], g["scores"], rtol=1e-9, atol=0)
    assert np.array_equal(est["assignment"], g["assignment"])
    check_mean_params(g, info["params"], info["branch"], info["n_used"])
    if not (g["branch"] == 2).any():
        assert np.array_equal(est["genotypes"].values, g["genotypes"])
    assert est["FN_geno"] == g["FN_geno"] and est["FP_geno"] == g["FP_geno"]
    for k in ("a", "FN", "FP"):
        assert np.array_equal(np.array(est[k]), g[k])


@pytest.mark.parametrize("case", CASES)
def test_concat_chains(case):
    g = gold(case)
    cat = bnpc.concat_chains(chains(case))
    for k in ("assignments", "params", "DP_alpha", "FN", "FP", "ML", "MAP"):
        assert np.array_equal(cat[k], g["concat_" + k]) and cat[k].dtype == g["concat_" + k].dtype, k
    assert cat["burn_in"] == 0


@pytest.mark.parametrize("case", CASES)
def test_twin_against_reference(case):
    g = gold(case)
    cat = bnpc.concat_chains(chains(case))
    est, info = bnpc.posterior_estimate_host(cat["assignments"], cat["params"], g["data"], cat["DP_alpha"], cat["FN"], cat["FP"], final_assignment=g["forced"], details=True)
    check_estimate(g, est, info)
    if g["forced"] is not None:                      # the distance of the cases that force their assignment
        host = bnpc._Host(*bnpc._check_samples(cat["assignments"], None))
        assert np.array_equal(host.codist(), g["D"])


def test_every_branch_is_covered():
    seen = set()
    for case in CASES:
        seen |= set(gold(case)["branch"].tolist())
    assert seen == {0, 1, 2, 3}


def test_one_cut_tree_call_equals_the_per_n_calls():
    from scipy.cluster.hierarchy import cut_tree, linkage
    g = gold("n130s9")
    Z = linkage(g["dist"], method="ward")
    ns = list(range(2, 14))
    both = cut_tree(Z, n_clusters=ns)
    for k, n in enumerate(ns):
        assert np.array_equal(both[:, k], cut_tree(Z, n_clusters=n).flatten())


def test_cut_range_is_the_reference_expression():
    assert bnpc.cut_range(4.0, 63).tolist() == list(range(2, 10))
    assert bnpc.cut_range(0.0, 20).size == 0
    assert bnpc.cut_range(1.0, 20).tolist() == [2]
    assert bnpc.cut_range(12.6, 20).tolist() == np.arange(2.52, 20, dtype=int).tolist()


def test_empty_range_raises_with_a_message():
    cat = bnpc.concat_chains(chains("sep"))
    with pytest.raises(ValueError, match="n_range is empty"):
        bnpc.posterior_estimate_host(cat["assignments"], cat["params"], gold("sep")["data"], cat["DP_alpha"], cat["FN"], cat["FP"])


def test_bad_samples_are_refused():
    with pytest.raises(ValueError, match="at least 1 sample and 2 cells"):
        bnpc._check_samples(np.zeros((3, 1), int), None)
    with pytest.raises(ValueError, match="outside"):
        bnpc._check_samples(np.array([[0, 2]]), None)
    with pytest.raises(ValueError, match="float32"):
        bnpc._check_samples(np.array([[0, 1]]), np.full((1, 2, 1), 0.1))


def test_save_and_load_chains(tmp_path):
    res = chains("n63s33")
    p = str(tmp_path / "c.npz")
    bnpc.save_chains(p, res)
    back = bnpc.load_chains(p)
    assert len(back) == len(res) == 2
    for a, b in zip(res, back):
        assert a["burn_in"] == b["burn_in"]
        for k in ("assignments", "params", "DP_alpha", "FN", "FP", "ML", "MAP"):
            assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype


def compare_files(out_dir, case):
    for made, kept in FILES:
        want = os.path.join(GOLD, "bnpcest.%s.%s" % (case, kept))
        if os.path.exists(want):
            assert open(os.path.join(out_dir, made), "rb").read() == open(want, "rb").read(), (case, made)
        else:
            assert not os.path.exists(os.path.join(out_dir, made)), (case, made)


@pytest.mark.parametrize("case", CASES)
def test_files_against_reference(case, tmp_path):
    g = gold(case)
    cat = bnpc.concat_chains(chains(case))
    est = bnpc.posterior_estimate_host(cat["assignments"], cat["params"], g["data"], cat["DP_alpha"], cat["FN"], cat["FP"], final_assignment=g["forced"])
    inferred = {"mean": {"posterior": est}}
    rows = int(g["rows"])
    bnpc.save_errors(inferred, ["posterior"], rows, str(tmp_path))
    bnpc.save_assignments(inferred, ["posterior"], rows, str(tmp_path))
    bnpc.save_geno(inferred, str(tmp_path), np.array(["m%02d" % i for i in range(g["data"].shape[1])]))
    compare_files(str(tmp_path), case)


def write_input(path, data):
    """the cells x mutations matrix as BnpC_input/<id>.BinaryMatrix.tsv holds it: mutations in rows, 3 for missing"""
    with open(path, "w") as f:
        f.write("\t".join([""] + ["c%03d" % i for i in range(data.shape[0])]) + "\n")
        for m in range(data.shape[1]):
            f.write("\t".join(["m%02d" % m] + ["3" if np.isnan(v) else str(int(v)) for v in data[:, m]]) + "\n")


def run_script(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONDONTWRITEBYTECODE="1")
    return subprocess.run([sys.executable, SCRIPT] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.parametrize("case", ["n63s33", "n130s9", "real"])
def test_script_host_estimate(case, tmp_path):
    g = gold(case)
    inp = str(tmp_path / "in.tsv")
    write_input(inp, g["data"])
    out = str(tmp_path / "out")
    r = run_script([inp, "--chains_npz", os.path.join(GOLD, "bnpcest.%s.chains.npz" % case), "--no_plots", "--host_estimate", "-n", str(int(g["rows"])), "-o", out, "-v", "0"])
    assert r.returncode == 0, r.stderr
    compare_files(out, case)


def test_script_refuses_what_it_does_not_state(tmp_path):
    inp = str(tmp_path / "in.tsv")
    write_input(inp, gold("n3s2")["data"])
    npz = os.path.join(GOLD, "bnpcest.n3s2.chains.npz")
    r = run_script([inp, "--chains_npz", npz, "--no_plots", "--host_estimate", "-sc", "-o", str(tmp_path / "o")])
    assert r.returncode != 0 and "--single_chains" in r.stderr and "not supported" in r.stderr
    r = run_script([inp, "--chains_npz", npz, "--no_plots", "--host_estimate", "-e", "posterior", "ML", "-o", str(tmp_path / "o")])
    assert r.returncode != 0 and "--chains_npz" in r.stderr and "ML" in r.stderr
    r = run_script([inp, "--chains_npz", npz, "--host_estimate", "-o", str(tmp_path / "o"), "--bnpc_libs", str(tmp_path / "nowhere")])
    assert r.returncode != 0 and "--no_plots" in r.stderr


@pytest.mark.skipif(not os.environ.get("LONGSOM_CHECKOUT"), reason="LONGSOM_CHECKOUT names no LongSom checkout (the sampler is the checkout's)")
def test_script_sampling_path(tmp_path):
    """the sampler of a checkout, the estimate of the twin: the three files appear and the saved chains give the same files again"""
    libs = os.path.join(os.environ["LONGSOM_CHECKOUT"], "workflow", "scripts", "CellClustering", "libs")
    g = gold("real")
    inp = str(tmp_path / "in.tsv")
    write_input(inp, g["data"])
    out, npz = str(tmp_path / "out"), str(tmp_path / "chains.npz")
    r = run_script([inp, "--bnpc_libs", libs, "-n", "2", "-s", "40", "--seed", "5", "--no_plots", "--host_estimate", "--save_chains", npz, "-o", out, "-v", "0"])
    assert r.returncode == 0, r.stderr
    out2 = str(tmp_path / "out2")
    r = run_script([inp, "--chains_npz", npz, "-n", "2", "--no_plots", "--host_estimate", "-o", out2, "-v", "0"])
    assert r.returncode == 0, r.stderr
    for f in ("assignment.txt", "errors.txt", "genotypes_posterior_mean.tsv"):
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(out2, f), "rb").read()
