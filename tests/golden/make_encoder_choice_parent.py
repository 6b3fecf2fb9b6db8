"""Writes encoder_choice_parent.npz: the encoder, norm bits and payload digest of every cell of
tests/test_gpu_encoder_choice.py, as the checked-out build computes them on the GPU.

Run it on the commit whose behaviour is the reference (the parent of a change that must keep it):
    python tests/golden/make_encoder_choice_parent.py [out.npz]
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root

import test_gpu_encoder_choice as cases  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "encoder_choice_parent.npz")
    cells = cases.choice_cells(torch.device("cuda", 0))
    np.savez_compressed(out, **cases.pack_cells(cells))
    print("wrote", out, len(cells), "cells")
