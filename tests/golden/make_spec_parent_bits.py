"""Writes spec_parent_bits.npz: the bracketed encoder's norm bits and payload digests of the cases of
tests/test_gpu_spec_pass_bits.py, as the checked-out build computes them on the GPU.

Run it on the commit whose bits are the reference (the parent of a change that must keep them):
    python tests/golden/make_spec_parent_bits.py [out.npz]
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root

import test_gpu_spec_pass_bits as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "spec_parent_bits.npz")
    np.savez(out, **cases.parent_bits_cases(torch.device("cuda", 0)))
    print("wrote", out)
