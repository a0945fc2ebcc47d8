"""CPU: tests/support/grid_caps.py lists every place in longsom_amd/csrc/*.hip that reads the CU count - a grid capped at a multiple of
it, with the test that takes the kernel past the cap - and nothing that is gone.  A plain text search for `n_cus`, file by file: a new
capped launch cannot be added without deciding how its loop is tested.  The test ids the table names must exist."""
import glob
import os
import re
from collections import Counter

from tests.support import grid_caps as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "longsom_amd", "csrc")


def uses():
    """{file: [the lines that hold n_cus]} over the .hip sources"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            lines = [l.strip() for l in f if "n_cus" in l]
        if lines:
            out[os.path.basename(path)] = lines
    return out


def unlisted_and_gone(launches, others):
    """(source lines no entry's text matches, or more of them than entries; entries whose text matches fewer lines than there are entries of it)"""
    listed = Counter((e.file, e.match) for e in list(launches) + list(others))
    found = Counter()
    unlisted = []
    for name, lines in uses().items():
        for line in lines:
            hit = [k for k in listed if k[0] == name and k[1] in line]
            assert len(hit) <= 1, "two entries' texts match one line of %s: %s" % (name, hit)
            if not hit:
                unlisted.append((name, line))
            else:
                found[hit[0]] += 1
    unlisted += [k for k in listed if found[k] > listed[k]]
    gone = [k for k in listed if found[k] < listed[k]]
    return unlisted, gone


def test_every_use_of_the_cu_count_is_listed_and_none_is_gone():
    assert len(uses()) >= 10, "the search found too few files: %s" % sorted(uses())
    unlisted, gone = unlisted_and_gone(gc.LAUNCHES, gc.OTHER_USES)
    assert not unlisted, "a grid sized from n_cus that tests/support/grid_caps.py does not list: %s" % (unlisted,)
    assert not gone, "tests/support/grid_caps.py lists a launch that is gone: %s" % (gone,)


def test_the_guard_notices_a_missing_and_a_stale_entry():
    for k in (0, len(gc.LAUNCHES) // 2, len(gc.LAUNCHES) - 1):
        unlisted, gone = unlisted_and_gone(gc.LAUNCHES[:k] + gc.LAUNCHES[k + 1:], gc.OTHER_USES)
        assert unlisted and not gone, gc.LAUNCHES[k].kernel
    stale = gc.Launch("fastq.hip", "k_none", "dim3((unsigned)(c->n_cus * 3))", lambda cu: 3 * cu, "nothing", test="x")
    assert unlisted_and_gone(gc.LAUNCHES + [stale], gc.OTHER_USES) == ([], [("fastq.hip", stale.match)])


def test_every_entry_says_how_it_is_tested_and_the_tests_exist():
    ids = set()
    for e in gc.LAUNCHES:
        assert e.cap(256) > 0 and e.unit
        if e.test:
            assert e.why is None and not e.covered_by, e.kernel
            assert e.test.startswith("tests/test_grid_caps_gpu.py::"), e.kernel
            ids.add(e.test)
        else:
            assert e.why and e.why.rstrip().endswith(".") and e.covered_by, e.kernel
            ids.update(e.covered_by)
    for tid in sorted(ids):
        path, name = tid.split("::")
        assert path.endswith("_gpu.py"), tid
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(r"^def %s\(" % re.escape(name), f.read(), re.M), "%s is not a test of %s" % (name, path)
