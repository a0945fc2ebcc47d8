"""CPU: the decision about a load's form (csrc/load_form.h: what an attempt wants, what it settles on or the rung it starts again on, the
predicates about read filters and references) is plain host C++; here it is compiled under AddressSanitizer + UndefinedBehaviorSanitizer
and walked as a table (tests/native/test_load_form.cpp).  The forms on the GPU: tests/test_fused_gpu.py, tests/test_load_pipeline_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
       "-I" + os.path.join(ROOT, "longsom_amd", "csrc")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_load_form_table(tmp_path):
    """every single reason against a load by windows gives the outcome stated by hand; over every combination of the facts a returned
    rung is lower than the attempt's, and the restarts end in the form the lowest rung gives directly"""
    exe = str(tmp_path / "test_load_form")
    subprocess.check_call(SAN + ["-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "test_load_form.cpp"), "-o", exe])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "load form ok" in r.stdout
