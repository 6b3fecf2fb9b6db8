"""Every Top-K encoder path against the CPU oracle, byte for byte: plan x ratio x call sequence x alpha x
path x tie order on four small plans (tests/golden/topk_matrix_inputs.py: edge sizes, sampled tensors
crafted for the sure-key restore, the big-bin buckets, the redo and the device-decided fallback, 300
tensors for the exact path, and the edge tensors again at starts 4 elements apart at the closest;
tests/test_topk_matrix_host.py checks what the matrix assumes of them).

A cell is never compared with another GPU call or a recorded build; no tolerance appears anywhere.
Per cell and per call (a single mode-0 call, or the error-feedback sequence mode 2, 1, 1 — the oracle
carries its own residual, the GPU's is compared after every call), against ``oracle.topk_ef_step``:

* ``ks`` is ``oracle.topk_k`` per tensor; ``values`` / ``indices`` over ``[0, K)`` equal the oracle's
  (tie order "index": |t'| descending, index ascending; "torch": torch.topk's on the CPU, and the
  oracle's residual then follows torch's selection); the 64 guard elements past ``K`` are untouched;
* the residual equals the oracle's over every tensor and keeps its canary in the padding (no Top-K
  kernel stores outside a tensor's elements: the fused pass, the bucket sort, the planned scatter, the
  zero fill, the gather and the tail index the residual by tensor base + candidate index only);
  the mode-2 call starts from a residual full of the canary, which it must not read;
* ``x`` is unchanged; its padding holds the canary (-3e38: it would be selected if read as data);
* ``plan.check()`` is truthy;
* ``plan.topk_decode_arena(mode=0)`` of the call's selection into a canary-filled arena equals
  ``oracle.topk_desparse`` per tensor and zero in the padding.

Paths: the default, ``set_topk(fallback=1)`` and, on the sampled plan, ``set_topk(sure=(0, 0))``.  After
the cells, the matrix's own coverage is asserted from ``topk_stats()``.
"""

import numpy as np
import pytest
import torch

import oracle
import topk_matrix_inputs as M
from omnifed_amd import codec

pytestmark = pytest.mark.gpu

GUARD = 64
VGUARD, IGUARD = 7.5, -7
SEQS = {"single": (0,), "ef": (2, 1, 1)}
TIES = ("index", "torch")
PATHS = {"default": {}, "fallback": {"fallback": 1}, "sure0": {"sure": (0.0, 0.0)}}
SURE_DEFAULT = (1.5, 2.0)  # omf_common.h TopkKnobs
CASES = [(p, r, path) for p, spec in M.PLANS.items() for r in spec.ratios for path in PATHS
         if path != "sure0" or p == "sampled"]

CELLS = set()
STATS = {}      # (plan, ratio, seq, alpha, tie, call) -> topk_stats() of that call, default path only
REORDERED = {}  # (plan, ratio, path, seq, alpha, call) -> plan.topk_reordered of the "torch" cells


def _cells(plan, ratio, path):
    return [(plan, ratio, path, seq, alpha, tie) for seq in SEQS for alpha in M.ALPHAS for tie in TIES]


class Ctx:
    """One plan: the codec plan, the inputs on the device and the oracle's results (cached per ratio:
    they do not depend on the path)."""

    def __init__(self, gpu, spec):
        self.gpu, self.spec = gpu, spec
        self.plan = codec.Plan(spec.sizes, offsets=spec.offsets, device=gpu)
        assert self.plan.offsets == spec.offsets and self.plan.arena_end == spec.arena_end
        self.plan.set_topk(sample_runs=M.SAMPLE_RUNS)
        self.x_host = [M.make_arena(spec, c) for c in range(M.N_CALLS)]
        self.x_dev = [torch.from_numpy(x).to(gpu) for x in self.x_host]
        self.x_ref = [x.clone() for x in self.x_dev]
        self.pad = M.padding_mask(spec)
        self.ranges = list(zip(spec.offsets, spec.sizes))
        self.want_ratio, self.want = None, {}

    def oracle(self, ratio, seq, alpha, tie):
        """Per call: (values[K], indices[K], residual arena or None, decoded arena)."""
        if self.want_ratio != ratio:
            self.want_ratio, self.want = ratio, {}
        key = (seq, alpha, tie)
        if key in self.want:
            return self.want[key]
        spec = self.spec
        ks = [oracle.topk_k(n, ratio) for n in spec.sizes]
        res = [None] * len(ks)
        calls = []
        for call, mode in enumerate(SEQS[seq]):
            vals, idxs = [], []
            arena = None if mode == 0 else np.full(spec.arena_end, M.CANARY, np.float32)
            dec = np.zeros(spec.arena_end, np.float32)
            for t, (o, n) in enumerate(self.ranges):
                v, i, res[t] = oracle.topk_ef_step(self.x_host[call][o:o + n], res[t], mode, alpha, ks[t], tie)
                vals.append(v)
                idxs.append(i)
                if arena is not None:
                    arena[o:o + n] = res[t]
                dec[o:o + n] = oracle.topk_desparse(torch.from_numpy(v), torch.from_numpy(i), n).numpy()
            calls.append((np.concatenate(vals), np.concatenate(idxs), arena, dec))
        self.want[key] = (ks, calls)
        return self.want[key]


_CTX = {}


@pytest.fixture
def ctx_of(gpu):
    def get(name):
        if name not in _CTX:
            _CTX[name] = Ctx(gpu, M.PLANS[name])
        return _CTX[name]
    return get


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _first_diff(got, want, starts, names):
    """Where two equal-length arrays first differ, by tensor (starts: each tensor's first position)."""
    bad = np.flatnonzero(_bits(got) != _bits(want))
    if not bad.size:
        return None
    i = int(bad[0])
    t = int(np.searchsorted(starts, i, side="right")) - 1
    inside = i - starts[t]
    return (f"{bad.size} differ, first at {i} = {names[t]}[{inside}]: got {got[i]!r} "
            f"(0x{int(_bits(got)[i]) & 0xffffffffffffffff:x}), want {want[i]!r}; tensors "
            f"{sorted({names[int(np.searchsorted(starts, int(b), side='right')) - 1] for b in bad[:2000]})[:6]}")


def run_cell(c, ratio, path, seq, alpha, tie):
    """Run one cell's calls, asserting after each everything the module's docstring lists."""
    plan, gpu, spec = c.plan, c.gpu, c.spec
    ks, want = c.oracle(ratio, seq, alpha, tie)
    K = sum(ks)
    kstart = np.concatenate([[0], np.cumsum(ks)[:-1]])
    astart = np.array(spec.offsets)
    res = torch.full((spec.arena_end,), M.CANARY, dtype=torch.float32, device=gpu) if seq == "ef" else None
    for call, mode in enumerate(SEQS[seq]):
        where = f"call {call} (mode {mode})"
        wv, wi, wres, wdec = want[call]
        values = torch.full((K + GUARD,), VGUARD, dtype=torch.float32, device=gpu)
        indices = torch.full((K + GUARD,), IGUARD, dtype=torch.int64, device=gpu)
        x = c.x_dev[call]
        plan.topk_stats(reset=True)
        _, _, got_ks = plan.topk_encode(x, ratio, residual=res, residual_mode=mode, values=values, indices=indices,
                                        alpha=alpha, tie_order=tie)
        assert plan.check(), where
        st = plan.topk_stats(reset=True)
        if path == "default":
            STATS[(spec.name, ratio, seq, alpha, tie, call)] = st
        if tie == "torch":
            REORDERED[(spec.name, ratio, path, seq, alpha, call)] = plan.topk_reordered
        assert got_ks == ks, where
        vh, ih = values.cpu().numpy(), indices.cpu().numpy()
        assert (_bits(vh[K:]) == _bits(np.full(GUARD, VGUARD, np.float32))).all(), (where, "values written past K")
        assert (ih[K:] == IGUARD).all(), (where, "indices written past K")
        d = _first_diff(ih[:K], wi, kstart, spec.names)
        assert d is None, (where, "indices", st, d)
        d = _first_diff(vh[:K], wv, kstart, spec.names)
        assert d is None, (where, "values", st, d)
        if mode:
            rh = res.cpu().numpy()
            assert (rh[c.pad] == np.float32(M.CANARY)).all(), (where, "the residual's padding was written")
            d = _first_diff(rh, wres, astart, spec.names)
            assert d is None, (where, "residual", st, d)
        assert torch.equal(x.view(torch.int32), c.x_ref[call].view(torch.int32)), (where, "x changed")
        y = torch.full((spec.arena_end,), M.CANARY, dtype=torch.float32, device=gpu)
        plan.topk_decode_arena(values, indices, ratio, y=y, mode=0)
        yh = y.cpu().numpy()
        assert not yh[c.pad].view(np.uint32).any(), (where, "decode: padding is not +0")
        d = _first_diff(yh, wdec, astart, spec.names)
        assert d is None, (where, "decode", d)
    CELLS.add((spec.name, ratio, path, seq, alpha, tie))


@pytest.mark.parametrize("plan,ratio,path", CASES, ids=[f"{p}-{r:.3g}-{path}" for p, r, path in CASES])
def test_cells_equal_oracle(ctx_of, plan, ratio, path):
    c = ctx_of(plan)
    failed = []
    c.plan.set_topk(**PATHS[path])
    try:
        for cell in _cells(plan, ratio, path):
            try:
                run_cell(c, *cell[1:])
            except AssertionError as e:  # every failing cell of the test is named; a RuntimeError ends it at once
                failed.append(f"{cell}: {str(e)[:600]}")
    finally:
        c.plan.set_topk(fallback=0, sure=SURE_DEFAULT)
    assert not failed, f"{len(failed)} of {len(_cells(plan, ratio, path))} cells failed:\n" + "\n".join(failed)


def test_matrix_coverage():
    """Conditions on the matrix itself (the cells above must all have run in this session)."""
    missing = [cell for case in CASES for cell in _cells(*case) if cell not in CELLS]
    assert not missing, f"{len(missing)} cells did not run (or failed), first {missing[:3]}"
    total = {k: sum(st[k] for st in STATS.values()) for k in ("calls", "fast", "zero_fill", "fallback", "redo", "exact")}
    print("unforced calls by path:", total, "reordered tensors:", sum(REORDERED.values()))
    for k in ("fast", "zero_fill", "fallback", "redo", "exact"):
        assert total[k] > 0, (k, total)
    assert any(v > 0 for v in REORDERED.values())
    first = {k: st for k, st in STATS.items() if k[0] == "sampled" and k[5] == 0}
    for (_, ratio, seq, alpha, tie, _), st in first.items():
        if ratio == 0.01:  # the under_sampled tensor's restore ran in the bucket kernels; a big-bin bucket too
            assert st["fast"] == 1 and st["fallback"] == 0 and st["redo"] == 0, (ratio, seq, alpha, tie, st)
        else:  # the cluster tensor's over-full fine bin and the sample_is_top tensor's redo
            assert st["fallback"] == 1 and st["redo"] >= 1, (ratio, seq, alpha, tie, st)
    assert all(st["exact"] == 1 for k, st in STATS.items() if k[0] == "many")
    assert any(st["zero_fill"] > 0 for k, st in STATS.items() if k[0] == "edges")
