"""CPU: the device's DEFLATE encoder (csrc/deflate_core.h, host + device code as inflate_core.h is) compiled for the host under
AddressSanitizer + UndefinedBehaviorSanitizer and checked against zlib's inflate and the device's own decoder
(tests/native/test_deflate.cpp: every size 0-300, the window's and the block's edges, nine kinds of content, 2 000 seeded mixes, the
inflated blocks of two golden BAMs; one lane and 64 emulated lanes with interleaved tables).  The same code on the GPU:
tests/test_split_bam_gpu.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
       "-I" + os.path.join(ROOT, "longsom_amd", "csrc")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.mark.parametrize("hash_bits", [7, 8, 9])
def test_deflate_core_inflates_with_zlib(tmp_path, hash_bits):
    """every stream inflates with zlib's inflate(-15) to the input with total_out == n; random bytes come out stored; a repeat beyond the
    window is never coded; at n = 0xff00 four byte values at random take <= 0.40 n (Huffman codes: fixed codes give 0.549 n) and a repeated
    64-byte string <= 0.10 n (LZ77 matches: Huffman alone gives 0.72 n) - with each of the three table sizes the device can run"""
    exe = str(tmp_path / "test_deflate")
    subprocess.check_call(SAN + ["-DLSD_TEST_HB=%d" % hash_bits] + [os.path.join(ROOT, "tests", "native", "test_deflate.cpp"), "-o", exe, "-lz"])
    r = subprocess.run([exe, os.path.join(G, "readfilter.bam"), os.path.join(G, "fusion", "routed.bam")], env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = re.search(r"deflate ok: (\d+) streams \((\d+) stored\), (\d+) BAM blocks", r.stdout)
    assert m and int(m.group(1)) > 20000 and int(m.group(2)) > 0 and int(m.group(3)) >= 4, r.stdout[-2000:]
    four = float(re.search(r"four values: \d+ -> \d+ \(([0-9.]+) n\)", r.stdout).group(1))
    rep = float(re.search(r"64-byte string repeated: \d+ -> \d+ \(([0-9.]+) n\)", r.stdout).group(1))
    assert four <= 0.40 and rep <= 0.10
