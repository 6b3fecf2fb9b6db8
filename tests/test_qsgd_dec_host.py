"""The QSGD receive side's host rules on the CPU (omnifed_amd/csrc/omf_qsgd_dec.h, tests/host/qsgd_dec_check.cpp).

The chaining rule of the K-client sums (groups of at most `per` clients; every group but the first starts
from y; the first fills the padding unless the call's init; only the last divides; the padding's divisor is
the whole call's), the levels scale (the exact 2^-s for a power of two, else 0) and the overlap test are
plain C++ with no HIP header, shared by omf_qsgd_decode_sum and omf_qsgd_decode_sum_packed.  The checker
sweeps per in {4, 8}, K in {1, per - 1, per, per + 1, 2 per, 2 per + 1, 3 per + 1}, init in {0, 1} and
divisor in {0, 3} under AddressSanitizer and UBSan.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "host", "qsgd_dec_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_qsgd_dec_host_rules(tmp_path):
    exe = str(tmp_path / "qsgd_dec_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-o", exe, CHECKER], check=True)
    out = subprocess.run([exe], check=False, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("0 failures, ") or "\n0 failures, " in out.stdout, out.stdout
    checks = int(out.stdout.strip().rsplit(" ", 2)[-2])
    assert checks > 500, out.stdout  # 2 x 7 x 2 x 2 calls of one to four groups, seven checks a group
