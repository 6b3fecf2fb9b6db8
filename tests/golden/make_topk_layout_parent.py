"""Writes topk_layout_parent.npz: the Top-K workspace sizes the checked-out build reports on the GPU for
the four matrix plans at their ratios (tests/golden/topk_layout_cases.py), the two plans of
tests/test_gpu_topk_layout.py's second part, and the device's CU count.

Run it on the commit whose sizes are the reference (the parent of a change that must keep them):
    python tests/golden/make_topk_layout_parent.py [out.npz]
"""

import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root

import topk_layout_cases as C  # noqa: E402
import topk_matrix_inputs as M  # noqa: E402
from omnifed_amd import codec  # noqa: E402
from omnifed_amd._lib import lib  # noqa: E402


def sizes_of(plan, spec, ratio):
    """(encode, decode, decode for the ratio's own counts, decode for the mixed counts) workspace bytes."""
    L = lib()
    row = [L.omf_topk_workspace_bytes(plan.handle, float(ratio)),
           L.omf_topk_decode_workspace_bytes(plan.handle, float(ratio))]
    for counts in C.count_vectors(spec, ratio):
        row.append(L.omf_topk_decode_counts_workspace_bytes(plan.handle, (ctypes.c_int64 * plan.nt)(*counts)))
    return [int(v) for v in row]


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "topk_layout_parent.npz")
    dev = torch.device("cuda", 0)
    plans = {name: codec.Plan(spec.sizes, offsets=spec.offsets, device=dev) for name, spec in M.PLANS.items()}
    rows = [sizes_of(plans[name], M.PLANS[name], ratio) for name, ratio in C.CASES]
    # both alive at once, each asked before any encode: every answer is a fresh computation
    pair = [codec.Plan(s, offsets=C.PAIR_OFFSETS, device=dev) for s in C.PAIR_SIZES]
    pair_ws = [int(lib().omf_topk_workspace_bytes(p.handle, C.PAIR_RATIO)) for p in pair]
    np.savez_compressed(out, keys=np.array([C.case_key(*c) for c in C.CASES]), sizes=np.array(rows, np.int64),
                        pair_ws=np.array(pair_ws, np.int64),
                        cus=np.int64(torch.cuda.get_device_properties(0).multi_processor_count))
    for c, r in zip(C.CASES, rows):
        print(C.case_key(*c), r)
    print("pair", pair_ws, "wrote", out)
