"""The plan's host side on the CPU (omnifed_amd/csrc/omf_plan_layout.cpp, tests/host/plan_layout_check.cpp).

The work-item tables, the carve of the plan's device allocation and the encoder choice are pure integer
code with no HIP header.  The checker builds the tables of tiny arenas under every ring configuration
kind, both big modes, gaps -1 / 0 / 3 and 8 / 16 rows per thread and asserts what the kernels rely on
(every element quantised once and counted in one norm partial, NORM before QUANT, disjoint partial and
granule bases, fold segments, decoder blocks, register-resident rows, 16-byte carve offsets), under
AddressSanitizer and UBSan.  The choice function is checked against the encoders an MI355X build
recorded in tests/golden/encoder_choice_parent.npz (the fixture of tests/test_gpu_encoder_choice.py).
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnifed_amd", "csrc")
CHECKER = os.path.join(ROOT, "tests", "host", "plan_layout_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "encoder_choice_parent.npz")

ENCODERS = {"resident": 0, "ordered": 1, "ring": 2, "bracket": 3, "grid": 4, "norm_in": 5}
STRATEGIES = ("resident", "ordered", "ring", "bracket", "grid")


def choice_rows(cells):
    """The recorded cells as calls of the choice function: 'strategy bits caller_u caller_norms fmt divide
    last_client wide_levels fused_bracket grid_fits op encoder' (op '=': chooses it, '!': does not, '|': this
    call or the same one without divide and last client chooses it)."""
    grid_fits = int(cells["grid_w1_f1_s4_dev"][0] == "grid")
    plain = dict(u=0, ni=0, fmt=0, div=0, last=0)
    calls = {
        "dev": plain, "u": dict(plain, u=1), "norm_in": dict(plain, ni=1), "bf16": dict(plain, fmt=1),
        "fp16": dict(plain, fmt=2), "ps": dict(plain, div=1),
        "ps_inplace": plain,  # in place: a divide, then a plain encode
    }
    rows = []

    def row(st, s, c, wide, fb, op, enc):
        rows.append(f"{st} {s} {c['u']} {c['ni']} {c['fmt']} {c['div']} {c['last']} {wide} {fb} {grid_fits} {op} {enc}")

    for key, (encoder, _, _) in cells.items():
        strategy, wide, fb, s, mode = key.split("_", 4)
        st, wide, fb, s, enc = STRATEGIES.index(strategy), int(wide[1:]), int(fb[1:]), int(s[1:]), ENCODERS[encoder]
        if mode.startswith("acc"):
            # the fused last client: one pass where the bracketed encoder serves it, else the decoder's
            # accumulate into avg_out, a divide in place and a plain encode (which may be a bracketed one)
            last = dict(plain, div=1, last=1)
            if encoder == "bracket":
                row(st, s, last, wide, fb, "|", enc)
            else:
                row(st, s, last, wide, fb, "!", ENCODERS["bracket"])
                row(st, s, plain, wide, fb, "=", enc)
        else:
            row(st, s, calls[mode], wide, fb, "=", enc)
    return rows


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_plan_layout_invariants_and_choice(tmp_path):
    exe = str(tmp_path / "plan_layout_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(CSRC, "omf_plan_layout.cpp"), CHECKER],
                   check=True)
    with np.load(GOLDEN) as z:
        cells = {str(k): (str(e), None, None) for k, e in zip(z["keys"], z["encoder"])}
    rows = choice_rows(cells)
    assert len(rows) >= len(cells)
    table = tmp_path / "choice_rows.txt"
    table.write_text("\n".join(rows) + "\n")
    out = subprocess.run([exe, str(table)], check=False, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"0 failures, {len(rows)} choice rows" in out.stdout, out.stdout
