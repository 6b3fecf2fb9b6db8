"""The Top-K workspaces' sizes against the build before the layout moved to omf_topk_layout.cpp, and two
plans that an address-keyed layout cache could not tell apart.

tests/golden/topk_layout_parent.npz (tests/golden/make_topk_layout_parent.py, run on an MI355X from that
build) holds, for the four plans of tests/golden/topk_matrix_inputs.py at their ratios, the encode, decode
and decode-by-counts workspace sizes, and the encode sizes of the two plans below.

Part one (no kernel is launched): the decode sizes are the recorded ones exactly; the encode size is the
recorded one minus the eight regions the encoder no longer allocates (koff, kk, kb2, tfirst, tlast, bbase,
sbase, and the unread fse table: ``topk_layout_cases.dead_bytes``, read off the recorded build's layout and
checked against the fixture when it was made).

Part two: two plans of equal nt and arena_end and different sizes — 152 against 40 bucket slots, so
different bucket-table regions (tests/host/topk_layout_check.cpp asserts that they differ) — are made,
used for one mode-0 encode and destroyed in turn on one thread.  Each must report its own size (its recorded fresh-process size minus the
eight regions; the recorded build's cache, keyed by the plan's address, nt and arena_end, could hand a
plan the other's) and select what the oracle (``oracle.topk_ef_step``, mode 0) selects, byte for byte.
"""

import os

import numpy as np
import pytest
import torch

import oracle
import topk_layout_cases as C
import topk_matrix_inputs as M
from omnifed_amd import codec
from omnifed_amd._lib import lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_layout_parent.npz")


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as z:
        return {"rows": {str(k): [int(v) for v in row] for k, row in zip(z["keys"], z["sizes"])},
                "pair_ws": [int(v) for v in z["pair_ws"]], "cus": int(z["cus"])}


def test_sizes_equal_recorded_build(gpu, recorded):
    import ctypes

    assert torch.cuda.get_device_properties(gpu).multi_processor_count == recorded["cus"]
    L = lib()
    plans = {name: codec.Plan(spec.sizes, offsets=spec.offsets, device=gpu) for name, spec in M.PLANS.items()}
    for name, ratio in C.CASES:
        spec, plan = M.PLANS[name], plans[name]
        enc, dec, own, mixed = recorded["rows"][C.case_key(name, ratio)]
        got = int(L.omf_topk_workspace_bytes(plan.handle, float(ratio)))
        assert got == enc - C.dead_bytes(plan.nt), (name, ratio, got, enc)
        assert int(L.omf_topk_decode_workspace_bytes(plan.handle, float(ratio))) == dec, (name, ratio)
        for counts, want in zip(C.count_vectors(spec, ratio), (own, mixed)):
            arr = (ctypes.c_int64 * plan.nt)(*counts)
            assert int(L.omf_topk_decode_counts_workspace_bytes(plan.handle, arr)) == want, (name, ratio, counts[:4])


def test_alternating_plans_keep_their_own_layout(gpu, recorded):
    L = lib()
    want_ws = [w - C.dead_bytes(len(C.PAIR_OFFSETS)) for w in recorded["pair_ws"]]
    assert want_ws[0] != want_ws[1]
    arena_end = C.PAIR_OFFSETS[-1] + C.PAIR_SIZES[0][-1]
    cases = []
    for i, sizes in enumerate(C.PAIR_SIZES):
        assert max(sizes) <= 16385 and C.PAIR_OFFSETS[-1] + sizes[-1] == arena_end
        x = np.zeros(arena_end, np.float32)
        want_v, want_i = [], []
        for t, (o, n) in enumerate(zip(C.PAIR_OFFSETS, sizes)):
            x[o:o + n] = np.random.default_rng([31, i, t]).standard_normal(n).astype(np.float32)
            v, ix, _ = oracle.topk_ef_step(x[o:o + n], None, 0, 1.0, oracle.topk_k(n, C.PAIR_RATIO), "index")
            want_v.append(v)
            want_i.append(ix)
        cases.append((sizes, torch.from_numpy(x).to(gpu), np.concatenate(want_v), np.concatenate(want_i)))
    for turn in range(4):  # a, b, a, b: each plan made where the one before it was destroyed
        i = turn & 1
        sizes, x, want_v, want_i = cases[i]
        plan = codec.Plan(sizes, offsets=C.PAIR_OFFSETS, device=gpu)
        assert plan.nt == len(C.PAIR_OFFSETS) and plan.arena_end == arena_end
        values, indices, ks = plan.topk_encode(x, C.PAIR_RATIO)
        assert plan.check(), turn
        assert ks == [oracle.topk_k(n, C.PAIR_RATIO) for n in sizes]
        assert indices.cpu().numpy().tobytes() == want_i.tobytes(), (turn, "indices")
        assert values.cpu().numpy().tobytes() == want_v.tobytes(), (turn, "values")
        assert int(L.omf_topk_workspace_bytes(plan.handle, C.PAIR_RATIO)) == want_ws[i], turn
        del plan, values, indices
