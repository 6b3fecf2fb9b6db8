"""Which encoder serves a call, and what it writes, across a rewrite of the plan's host side.

``tests/golden/encoder_choice_parent.npz`` holds, for every cell of the sweep below, the encoder
the build before the rewrite launched (``omf_plan_last_encoder``), ``norm_out``'s bit patterns and
the payload's SHA-256 over the tensor ranges (the PS cells' digest also covers the average), as that
build computed them on an MI355X (``tests/golden/make_encoder_choice_parent.py`` wrote the file from
``choice_cells`` below).  The build under test must reproduce every cell exactly.

tests/test_plan_layout_host.py checks the host's pure choice function against the same file.
"""

import hashlib
import os

import numpy as np
import pytest
import torch

from omnifed_amd import codec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_choice_parent.npz")

SIZES = [5, 4100, 16385, 70001]
BITS = (0, 1, 4, 5, 6, 7, 8, 9)
# on-device draws, caller uniforms, caller norms, bf16 / fp16 values, the fused PS step with avg_out
# apart from acc and in place, and the fused last client with an int8 and an int32 payload
MODES = ("dev", "u", "norm_in", "bf16", "fp16", "ps", "ps_inplace", "acc8", "acc32")
SEED, OFFSET, DIVISOR = 41, 3, 3.0
SWEEP = [(st, wide, fb) for st in codec.STRATEGIES for wide in (0, 1) for fb in (0, 1)]


def cell_key(strategy, wide, fb, s, mode):
    return f"{strategy}_w{wide}_f{fb}_s{s}_{mode}"


def _inputs(plan, gpu):
    rng = np.random.default_rng(2024)
    n, nt = plan.arena_end, plan.nt
    x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    xd = torch.from_numpy(x).to(gpu)
    inp = {
        "x": xd,
        "bf16": xd.to(torch.bfloat16).to(torch.float32),
        "fp16": xd.to(torch.float16).to(torch.float32),
        "u": torch.from_numpy(rng.random(n, dtype=np.float32)).to(gpu),
        "norm_in": torch.from_numpy((0.05 + rng.random(nt)).astype(np.float32)).to(gpu),
        "acc": torch.from_numpy((rng.standard_normal(n) * 3e-3).astype(np.float32)).to(gpu),
        "anorm": torch.from_numpy((0.01 + 0.01 * rng.random(nt)).astype(np.float32)).to(gpu),
        "q8": torch.from_numpy(rng.integers(-16, 17, n).astype(np.int8)).to(gpu),
        "q32": torch.from_numpy(rng.integers(-256, 257, n).astype(np.int32)).to(gpu),
    }
    return inp


def _run(plan, inp, s, mode):
    """One encode of `mode`; returns (q, norms, avg or None)."""
    dev = plan.device
    width = codec.storage_width(2 ** s)
    q = torch.zeros(plan.payload_elems(width), dtype=torch.int8 if width == 8 else torch.int32, device=dev)
    norms = torch.zeros(plan.nt, dtype=torch.float32, device=dev)
    kw = dict(q_out=q, norm_out=norms, seed=SEED, offset=OFFSET)
    if mode == "dev":
        plan.qsgd_encode(inp["x"], s, **kw)
    elif mode == "u":
        plan.qsgd_encode(inp["x"], s, u=inp["u"], **kw)
    elif mode == "norm_in":
        plan.qsgd_encode(inp["x"], s, norm_in=inp["norm_in"], **kw)
    elif mode in ("bf16", "fp16"):
        plan.qsgd_encode(inp[mode], s, value_format=1 if mode == "bf16" else 2, **kw)
    elif mode == "ps":
        avg, _, _ = plan.ps_apply_encode(inp["acc"], DIVISOR, s, **kw)
        return q, norms, avg
    elif mode == "ps_inplace":
        acc = inp["acc"].clone()
        plan.ps_apply_encode(acc, DIVISOR, s, avg_out=acc, **kw)
        return q, norms, acc
    else:
        wi, levels = (8, 16) if mode == "acc8" else (32, 256)
        avg, _, _ = plan.ps_accumulate_apply_encode(inp["acc"], inp["q8" if wi == 8 else "q32"], wi, levels,
                                                    inp["anorm"], DIVISOR, s, **kw)
        return q, norms, avg
    return q, norms, None


def choice_cells(gpu):
    """{cell key: [last encoder, norm_out's bit patterns as hex, SHA-256 of the payload's tensor ranges
    (then the average's, for the PS cells)]} of the whole sweep."""
    plan = codec.Plan(SIZES, device=gpu)
    inp = _inputs(plan, gpu)
    out = {}
    for strategy, wide, fb in SWEEP:
        plan.set_encode_strategy(strategy)
        plan.set_wide_levels(bool(wide))
        plan.set_fused_bracket(bool(fb))
        for s in BITS:
            for mode in MODES:
                q, norms, avg = _run(plan, inp, s, mode)
                plan.check()  # raises on an abandoned launch
                qh = q.cpu().numpy()
                h = hashlib.sha256()
                for o, n in zip(plan.offsets, plan.sizes):
                    h.update(qh[o:o + n].tobytes())
                if avg is not None:
                    ah = avg.cpu().numpy()
                    for o, n in zip(plan.offsets, plan.sizes):
                        h.update(ah[o:o + n].tobytes())
                out[cell_key(strategy, wide, fb, s, mode)] = [
                    plan.last_encoder, norms.cpu().numpy().view(np.uint32).tobytes().hex(), h.hexdigest()]
    return out


def pack_cells(cells):
    """The cells as arrays (the fixture file's): keys, encoder names, norm bit patterns, payload digests."""
    keys = sorted(cells)
    return {"sizes": np.array(SIZES, np.int64), "keys": np.array(keys), "encoder": np.array([cells[k][0] for k in keys]),
            "norm": np.array([np.frombuffer(bytes.fromhex(cells[k][1]), np.uint32) for k in keys]),
            "sha": np.array([np.frombuffer(bytes.fromhex(cells[k][2]), np.uint8) for k in keys])}


def unpack_cells(z):
    """{cell key: [encoder, norm hex, digest hex]} of a fixture file's arrays."""
    return {str(k): [str(e), n.tobytes().hex(), h.tobytes().hex()]
            for k, e, n, h in zip(z["keys"], z["encoder"], z["norm"], z["sha"])}


@pytest.fixture(scope="module")
def cells(gpu):
    return choice_cells(gpu)


@pytest.fixture(scope="module")
def parent():
    with np.load(GOLDEN) as z:
        assert z["sizes"].tolist() == SIZES
        return unpack_cells(z)


def test_sweep_is_the_recorded_one(cells, parent):
    assert sorted(cells) == sorted(parent)


@pytest.mark.parametrize("strategy,wide,fb", SWEEP)
def test_cells_equal_parent_build(cells, parent, strategy, wide, fb):
    keys = [cell_key(strategy, wide, fb, s, mode) for s in BITS for mode in MODES]
    for name, col in (("encoder", 0), ("norm_out", 1), ("payload", 2)):
        differ = [(k, parent[k][col], cells[k][col]) for k in keys if cells[k][col] != parent[k][col]]
        assert not differ, f"{name}: {len(differ)} cells differ from the parent build, first {differ[0]}"
