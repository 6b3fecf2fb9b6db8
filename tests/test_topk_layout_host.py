"""The Top-K host side on the CPU (omnifed_amd/csrc/omf_topk_layout.cpp, tests/host/topk_layout_check.cpp).

The per-tensor rules, the encoder's constant tables, the pipeline groups, the carve of the encode and
decode workspaces and the decoder's tables are pure integer code with no HIP header.  The checker runs
them over the four plans of tests/golden/topk_matrix_inputs.py at their ratios and over tiny arenas of
its own (n = 1, sizes around 512 and 16384, two super-items, ratio 1.0, 257 tensors, sample sizes
64 / 2048 / 2^20, 1 to nt + 3 groups) and asserts what the kernels rely on, under AddressSanitizer and
UBSan; the flat-item ranges are held to omf_plan_layout.cpp's tables.  For the plans of the sampled path
the workspace total is also held to the size an MI355X build recorded before the encoder stopped
allocating eight regions (tests/golden/topk_layout_parent.npz, the fixture of
tests/test_gpu_topk_layout.py): the recorded size minus those regions.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import topk_layout_cases as C
import topk_matrix_inputs as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnifed_amd", "csrc")
CHECKER = os.path.join(ROOT, "tests", "host", "topk_layout_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "topk_layout_parent.npz")


def arena_rows():
    """One line per (plan, ratio): name ratio tmp_bytes expected_total nt size offset ..."""
    with np.load(GOLDEN) as z:
        recorded = {str(k): int(row[0]) for k, row in zip(z["keys"], z["sizes"])}
        cus = int(z["cus"])
    rows = []
    for name, ratio in C.CASES:
        spec = M.PLANS[name]
        # the sampled path's temporary is the exact tail's digit table, 4 x 256 bytes per CU; the exact
        # path's is rocPRIM's to size, so only the GPU test compares that plan's total
        expect = -1 if name in C.EXACT_PLANS else recorded[C.case_key(name, ratio)] - C.dead_bytes(len(spec.sizes))
        cells = [f"{name}@{ratio!r}", repr(float(ratio)), str(4 * 256 * cus), str(expect), str(len(spec.sizes))]
        cells += [f"{n} {o}" for n, o in zip(spec.sizes, spec.offsets)]
        rows.append(" ".join(cells))
    return rows


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_topk_layout_invariants(tmp_path):
    exe = str(tmp_path / "topk_layout_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(CSRC, "omf_topk_layout.cpp"),
                    os.path.join(CSRC, "omf_plan_layout.cpp"), CHECKER], check=True)
    rows = arena_rows()
    assert len(rows) == len(C.CASES) == 9 and sum(r.split()[3] != "-1" for r in rows) == 8
    table = tmp_path / "arenas.txt"
    table.write_text("\n".join(rows) + "\n")
    out = subprocess.run([exe, str(table)], check=False, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1].split()
    assert last[:2] == ["0", "failures,"] and int(last[2]) == len(rows), out.stdout
    assert int(last[7]) >= 3 * (len(rows) + 10), out.stdout  # three sample sizes per arena, ten arenas of its own
