"""The Top-K receive side against a CPU oracle, cell by cell: omf_topk_decode, omf_topk_decode_arena,
omf_topk_decode_arena_ws (the tiled one-pass decoder), omf_topk_decode_counts, omf_topk_check_indices
and omf_topk_check_duplicates on messages no encoder made (tests/golden/topk_recv_inputs.py: five
layouts, count vectors with zeros, full and clamped buckets, index profiles that overflow an unstaged
bucket, sit on every tile edge or must be skipped; tests/test_topk_recv_host.py checks what the matrix
assumes of them).

A cell is never compared with another GPU call or a recorded build; no tolerance appears anywhere.
Non-NaN results are compared as uint32 bits; in modes 0 and 1 NaN payloads are bit-equal too, in mode 2
the NaN positions coincide.

Decode cells: layout x count vector x profile x mode x entry point, against ``decode_ref``.  ``y`` is a
16-byte aligned view inside a larger buffer with 4096 guard elements on either side, which must
survive; modes 1 and 2 run once more with ``y`` one element further (4-byte aligned).  Entry points:
``codec.topk_decode`` per tensor; ``plan.topk_decode_arena`` where the counts are a ratio's;
``plan.topk_decode_counts``; and for mode 0 the C calls omf_topk_decode_arena_ws and
omf_topk_decode_counts with ws = NULL (fill + scatter) and with a test-owned workspace: zero-filled
once, exactly ``*_workspace_bytes`` long, a 256-byte canary behind it; after every tiled call its
counters are zero again and the canary is intact.

Then: one workspace reused, uncleared, by a different message (overflowing -> uniform, uniform ->
overflowing, ktot = 0 -> uniform); ten count vectors back to back (the plan keeps the tables of 8);
the EINVAL cases; the index-check and duplicate-check cells; and the matrix's own coverage.
"""

import ctypes
import time

import numpy as np
import pytest
import torch

import topk_recv_inputs as R
from omnifed_amd import _lib, codec

pytestmark = pytest.mark.gpu

GUARD = 4096
GUARD_VAL = -2.5e38       # around y, and y itself before a mode-0 decode
WS_CANARY, WS_TAIL = 0xA5, 256
IGUARD, NIGUARD = -7, 64  # past ktot of a checked index array: in [-n, 0) of most tensors, so a touch shows
LAYOUT_NAMES = list(R.LAYOUTS)

# (entry point, mode, y offset in elements)
PY_ENTRIES = [(e, m, off) for e in ("tensor", "arena", "counts") for m in (0, 1, 2) for off in ((0,) if m == 0 else (0, 1))]
C_ENTRIES = [(e, 0, 0) for e in ("c_arena_null", "c_arena_ws", "c_counts_null", "c_counts_ws")]
ENTRIES = PY_ENTRIES + C_ENTRIES
TILED = ("c_arena_ws", "c_counts_ws")

CELLS = set()        # (layout, counts, profile, entry, mode, yoff)
OTHER = set()        # the cells of the other tests
WALL = {}            # test -> seconds


def _entries_of(msg):
    return [e for e in ENTRIES if msg.ratio is not None or "arena" not in e[0]]


def _all_cells():
    return [(name, c, p, *e) for name, L in R.LAYOUTS.items() for c, p in R.message_keys(L)
            for e in _entries_of(R.message(L, c, p))]


class Ctx:
    """One layout: the plan, its base arena, and per message the device copies and the oracle's arenas."""

    def __init__(self, gpu, L):
        self.gpu, self.L = gpu, L
        self.plan = codec.Plan(L.sizes, offsets=L.offsets, device=gpu)
        assert self.plan.offsets == L.offsets and self.plan.arena_end == L.arena_end
        self.base = R.make_base(L)
        self.base_dev = torch.from_numpy(self.base).to(gpu)
        self.pad = R.padding_mask(L)
        self.starts = np.array(L.offsets)
        self._dev, self._want = {}, {}

    def dev(self, msg):
        if msg.key not in self._dev:
            self._dev = {msg.key: (torch.from_numpy(msg.values).to(self.gpu), torch.from_numpy(msg.indices).to(self.gpu))}
        return self._dev[msg.key]

    def want(self, msg, mode):
        """decode_ref's arena (computed once per message and mode, never written again)."""
        k = (msg.key, mode)
        if k not in self._want:
            if len(self._want) >= 3:
                self._want.clear()
            w = R.decode_ref(mode, self.base, self.L, msg.counts, msg.values, msg.indices)
            w.setflags(write=False)
            self._want[k] = w
        return self._want[k]


_CTX = {}


@pytest.fixture
def ctx_of(gpu):
    def get(name):
        if name not in _CTX:
            _CTX[name] = Ctx(gpu, R.LAYOUTS[name])
        return _CTX[name]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _diff(got, want, c, nan_positions_only):
    """None, or where two arenas first differ (bits; NaN positions only where the sum makes the NaN)."""
    gb, wb = _bits(got), _bits(want)
    ne = gb != wb
    if nan_positions_only:
        ne &= ~(np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(ne)
    if not bad.size:
        return None
    i = int(bad[0])
    t = int(np.searchsorted(c.starts, i, side="right")) - 1
    return (f"{bad.size} differ, first at {i} = {c.L.names[t]}[{i - c.starts[t]}]: got {got[i]!r} (0x{int(gb[i]):08x}), "
            f"want {want[i]!r} (0x{int(wb[i]):08x})")


def _y_buffer(c, mode, yoff):
    buf = torch.full((GUARD + c.L.arena_end + GUARD + 4,), GUARD_VAL, dtype=torch.float32, device=c.gpu)
    assert buf.data_ptr() % 256 == 0
    y = buf[GUARD + yoff:GUARD + yoff + c.L.arena_end]
    if mode:
        y.copy_(c.base_dev)
    return buf, y


def _check_y(c, buf, yoff, want, mode, where, tensor_mode0=False):
    h = buf.cpu().numpy()
    lo, hi = GUARD + yoff, GUARD + yoff + c.L.arena_end
    g = np.float32(GUARD_VAL)
    assert (h[:lo] == g).all() and (h[hi:] == g).all(), (where, "a guard around y was written")
    got = h[lo:hi]
    if tensor_mode0:  # the per-tensor decode zero-fills its tensor, not the arena's padding
        want = want.copy()
        want[c.pad] = g
    d = _diff(got, want, c, nan_positions_only=(mode == 2))
    assert d is None, (where, d)


def _counts_arr(counts):
    return (ctypes.c_int64 * len(counts))(*[int(x) for x in counts])


def _stream(c):
    return ctypes.c_void_p(codec._stream(c.gpu))


class Workspace:
    """A test-owned workspace of the tiled decode: zero-filled once, ``nbytes`` long, then the canary."""

    def __init__(self, c, nbytes):
        assert nbytes > 0
        self.c, self.nbytes = c, int(nbytes)
        self.buf = torch.zeros(self.nbytes + WS_TAIL, dtype=torch.uint8, device=c.gpu)
        self.buf[self.nbytes:] = WS_CANARY
        assert self.buf.data_ptr() % 256 == 0
        torch.cuda.synchronize()

    def ptr(self, shift=0):
        return ctypes.c_void_p(self.buf.data_ptr() + shift)

    def check(self, where):
        """After a tiled call: fill[] and the overflow count are zero, the canary is intact."""
        words = self.c.L.nsuper + 1
        head = self.buf[:4 * words].cpu().numpy().view(np.uint32)
        assert not head.any(), (where, "workspace counters left non-zero", np.flatnonzero(head)[:8].tolist(),
                                head[np.flatnonzero(head)[:8]].tolist())
        assert (self.buf[self.nbytes:].cpu().numpy() == WS_CANARY).all(), (where, "workspace canary overwritten")


def _ws_need(c, msg, keyed):
    L = _lib.lib()
    if keyed == "ratio":
        return int(L.omf_topk_decode_workspace_bytes(c.plan.handle, float(msg.ratio)))
    return int(L.omf_topk_decode_counts_workspace_bytes(c.plan.handle, _counts_arr(msg.counts)))


def _c_decode(c, msg, keyed, y, ws_ptr, ws_bytes, mode=0):
    """omf_topk_decode_arena_ws (keyed "ratio") or omf_topk_decode_counts on the current stream; returns rc."""
    L = _lib.lib()
    v, i = c.dev(msg)
    vp, ip = (codec._ptr(v), codec._ptr(i)) if msg.ktot else (None, None)
    if keyed == "ratio":
        return L.omf_topk_decode_arena_ws(c.plan.handle, float(msg.ratio), vp, ip, codec._ptr(y), mode, ws_ptr,
                                          ctypes.c_size_t(ws_bytes), _stream(c))
    return L.omf_topk_decode_counts(c.plan.handle, _counts_arr(msg.counts), vp, ip, codec._ptr(y), mode, ws_ptr,
                                    ctypes.c_size_t(ws_bytes), _stream(c))


def run_cell(c, msg, entry, mode, yoff):
    L = c.L
    where = (L.name, msg.counts_name, msg.profile, entry, mode, yoff)
    buf, y = _y_buffer(c, mode, yoff)
    v, i = c.dev(msg)
    ws = None
    if entry == "tensor":
        koff = R.koff_of(msg.counts)
        for t, (o, n) in enumerate(zip(L.offsets, L.sizes)):
            codec.topk_decode(v[koff[t]:koff[t + 1]], i[koff[t]:koff[t + 1]], n, y=y[o:o + n], mode=mode)
    elif entry == "arena":
        c.plan.topk_decode_arena(v, i, msg.ratio, y=y, mode=mode)
    elif entry == "counts":
        c.plan.topk_decode_counts(msg.counts, v, i, y=y, mode=mode)
    else:
        keyed = "ratio" if "arena" in entry else "counts"
        if entry in TILED:
            ws = Workspace(c, _ws_need(c, msg, keyed))
            rc = _c_decode(c, msg, keyed, y, ws.ptr(), ws.nbytes)
        else:
            rc = _c_decode(c, msg, keyed, y, None, 0)
        assert rc == _lib.OMF_OK, (where, rc, _lib.lib().omf_last_error())
    torch.cuda.synchronize()
    _check_y(c, buf, yoff, c.want(msg, mode), mode, where, tensor_mode0=(entry == "tensor" and mode == 0))
    if ws is not None:
        ws.check(where)
    CELLS.add(where)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_decode_cells_equal_oracle(ctx_of, layout):
    c = ctx_of(layout)
    t0 = time.perf_counter()
    failed, n = [], 0
    for cname, profile in R.message_keys(c.L):
        msg = R.message(c.L, cname, profile)
        for mode in (0, 1, 2):  # one oracle arena at a time
            for entry, m, yoff in _entries_of(msg):
                if m != mode:
                    continue
                n += 1
                try:
                    run_cell(c, msg, entry, mode, yoff)
                except AssertionError as e:  # every failing cell is named; a RuntimeError ends the test at once
                    failed.append(f"{(cname, profile, entry, mode, yoff)}: {str(e)[:500]}")
    WALL[f"decode[{layout}]"] = time.perf_counter() - t0
    assert not failed, f"{len(failed)} of {n} cells failed:\n" + "\n".join(failed[:40])


SEQUENCES = {  # name -> the two messages (counts name, profile) that share one uncleared workspace
    "overflow_then_uniform": (("clu20k", "clustered"), ("clu20k", "uniform")),
    "uniform_then_overflow": (("clu20k", "uniform"), ("clu20k", "clustered")),
    "empty_then_uniform": (("none", "uniform"), ("r05", "uniform")),
    "ratio_overflow_then_uniform": (("r05", "clustered"), ("r05", "uniform")),
    "full_then_overflow": (("full", "uniform"), ("clu20k", "clustered")),
}


@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_workspace_reused_without_clearing(ctx_of, seq):
    """Every tiled decode leaves the workspace's counters zero: the next message, decoded with the same
    workspace and no memset, equals the oracle too (the buffer is as long as the larger need; each call
    is told its own exact size)."""
    c = ctx_of("aligned")
    t0 = time.perf_counter()
    msgs = [R.message(c.L, *k) for k in SEQUENCES[seq]]
    for keyed in (("counts", "ratio") if all(m.ratio is not None for m in msgs) else ("counts",)):
        needs = [_ws_need(c, m, keyed) for m in msgs]
        ws = Workspace(c, max(needs))
        for step, (m, need) in enumerate(list(zip(msgs, needs)) + [(msgs[0], needs[0])]):
            where = (seq, keyed, step, m.counts_name, m.profile)
            buf, y = _y_buffer(c, 0, 0)
            rc = _c_decode(c, m, keyed, y, ws.ptr(), need)
            assert rc == _lib.OMF_OK, (where, rc, _lib.lib().omf_last_error())
            torch.cuda.synchronize()
            ws.check(where)
            _check_y(c, buf, 0, c.want(m, 0), 0, where)
        OTHER.add(("sequence", seq, keyed))
    WALL[f"sequence[{seq}]"] = time.perf_counter() - t0


N_EVICT = 10


def test_count_tables_evicted_and_remade(ctx_of):
    """The plan keeps the tables of the last 8 count vectors: ten distinct ones back to back, mode 0 then
    mode 2, then the first again (its tables were freed meanwhile)."""
    c = ctx_of("aligned")
    L = c.L
    t0 = time.perf_counter()
    base_counts = R.count_vectors(L)["r01"]
    msgs = []
    for j in range(N_EVICT):
        counts = list(base_counts)
        counts[3] = 10 + j
        counts[6] = 1 + 100 * j
        rng = np.random.default_rng([L.seed, 77, j])
        per = R.uniform_indices(L, counts, rng)
        msgs.append(R.Message(L, f"evict{j}", "uniform", counts, per))
    assert len({tuple(m.counts) for m in msgs}) == N_EVICT > 8
    for mode in (0, 2):
        for j, m in enumerate(msgs + [msgs[0]]):
            where = ("evict", mode, j)
            buf, y = _y_buffer(c, mode, 0)
            v, i = torch.from_numpy(m.values).to(c.gpu), torch.from_numpy(m.indices).to(c.gpu)
            c.plan.topk_decode_counts(m.counts, v, i, y=y, mode=mode)
            torch.cuda.synchronize()
            want = R.decode_ref(mode, c.base, L, m.counts, m.values, m.indices)
            _check_y(c, buf, 0, want, mode, where)
            OTHER.add(where)
    WALL["evict"] = time.perf_counter() - t0


def test_errors_leave_y_alone(ctx_of):
    c = ctx_of("aligned")
    L = c.L
    msg = R.message(L, "r05", "uniform")
    lib = _lib.lib()

    def untouched(buf, where):
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == np.float32(GUARD_VAL)).all(), (where, "y was written by a refused call")

    for keyed in ("counts", "ratio"):
        need = _ws_need(c, msg, keyed)
        ws = Workspace(c, need + 16)
        buf, y = _y_buffer(c, 0, 0)
        assert _c_decode(c, msg, keyed, y, ws.ptr(), need - 1) == _lib.OMF_EINVAL, (keyed, "one byte short")
        untouched(buf, (keyed, "short"))
        assert _c_decode(c, msg, keyed, y, ws.ptr(16), need) == _lib.OMF_EINVAL, (keyed, "workspace at +16")
        untouched(buf, (keyed, "+16"))
        ws.check((keyed, "refused calls"))
        assert _c_decode(c, msg, keyed, y, ws.ptr(), need) == _lib.OMF_OK  # the same buffers are fine
        torch.cuda.synchronize()
        _check_y(c, buf, 0, c.want(msg, 0), 0, (keyed, "accepted"))
        OTHER.add(("errors", keyed))
    v, i = c.dev(msg)
    for t in (0, 2, L.nt - 1):
        counts = list(msg.counts)
        counts[t] = L.sizes[t] + 1
        arr = _counts_arr(counts)
        assert lib.omf_topk_decode_counts_workspace_bytes(c.plan.handle, arr) == 0
        for mode in (0, 1, 2):
            buf, y = _y_buffer(c, 0, 0)
            rc = lib.omf_topk_decode_counts(c.plan.handle, arr, codec._ptr(v), codec._ptr(i), codec._ptr(y), mode, None,
                                            ctypes.c_size_t(0), _stream(c))
            assert rc == _lib.OMF_EINVAL, (t, mode, rc)
            untouched(buf, ("counts over n", t, mode))
        with pytest.raises(ValueError):
            c.plan.topk_decode_counts(counts, v, i, mode=0)
    OTHER.add(("errors", "counts over n"))


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_index_check_cells(ctx_of, layout):
    c = ctx_of(layout)
    L = c.L
    t0 = time.perf_counter()
    failed = []
    for name, (counts, idx) in R.check_messages(L).items():
        try:
            ktot = int(idx.size)
            wrapped, bad = R.check_ref(L, counts, idx)
            host = np.concatenate([idx, np.full(NIGUARD, IGUARD, np.int64)])
            dev = torch.from_numpy(host).to(c.gpu)
            got_bad = int(c.plan.topk_check_indices(counts, dev).cpu()[0])
            got = dev.cpu().numpy()
            assert got_bad == bad, ("bad", got_bad, bad)
            assert (got[ktot:] == IGUARD).all(), "entries past ktot were touched"
            if bad == R.NO_BAD:
                ne = np.flatnonzero(got[:ktot] != wrapped)
                assert not ne.size, ("wrapped", ne[:5].tolist(), got[ne[:5]].tolist(), wrapped[ne[:5]].tolist())
            else:
                out = wrapped == idx  # not wrapped by the oracle: in [0, n) or out of range
                koff = R.koff_of(counts)
                n_of = np.repeat(np.array(L.sizes, np.int64), counts)
                out &= (idx < -n_of) | (idx >= n_of)
                assert out.any() and (got[:ktot][out] == idx[out]).all(), "an out-of-range entry was rewritten"
                assert koff[-1] == ktot
            OTHER.add(("check", layout, name))
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:400]}")
    WALL[f"check[{layout}]"] = time.perf_counter() - t0
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_duplicate_check_cells(ctx_of, layout):
    c = ctx_of(layout)
    L = c.L
    t0 = time.perf_counter()
    failed = []
    side = torch.cuda.Stream(c.gpu)
    for name, (counts, idx, clean) in R.dup_messages(L).items():
        try:
            want = R.dup_ref(L, counts, idx)
            d_idx, d_clean = torch.from_numpy(idx).to(c.gpu), torch.from_numpy(clean).to(c.gpu)
            ref_idx = d_idx.clone()
            torch.cuda.synchronize()
            got = c.plan.topk_check_duplicates(counts, d_idx).cpu().numpy()
            assert got.dtype == np.int32 and (got == want).all(), ("flags", np.flatnonzero(got != want)[:8].tolist())
            # the bitmap is all zero again: the same positions, each once, flag nothing
            after = c.plan.topk_check_duplicates(counts, d_clean).cpu().numpy()
            assert not after.any(), ("a stale bit flags the next, clean message", np.flatnonzero(after)[:8].tolist())
            # and from a second stream, right behind the flagged message on this one
            first = c.plan.topk_check_duplicates(counts, d_idx)
            second = c.plan.topk_check_duplicates(counts, d_clean, stream=side.cuda_stream)
            side.synchronize()
            torch.cuda.synchronize()
            assert (first.cpu().numpy() == want).all() and not second.cpu().numpy().any(), "second stream"
            assert torch.equal(d_idx, ref_idx), "the indices were changed"
            OTHER.add(("dups", layout, name))
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:400]}")
    WALL[f"dups[{layout}]"] = time.perf_counter() - t0
    assert not failed, "\n".join(failed)


def test_matrix_coverage(gpu):
    """Conditions on the matrix itself (the tests above must all have run in this session)."""
    print("wall time by test (s):", {k: round(v, 2) for k, v in WALL.items()}, "total", round(sum(WALL.values()), 2))
    missing = [cell for cell in _all_cells() if cell not in CELLS]
    assert not missing, f"{len(missing)} of {len(_all_cells())} cells did not run (or failed), first {missing[:3]}"
    combos = {(e, m, p) for (_, _, p, e, m, _) in CELLS}
    profiles = ("uniform", "clustered", "edges_of_tiles", "skipped")
    want = {(e, m, p) for e, m, _ in ENTRIES for p in profiles if not ("arena" in e and p == "edges_of_tiles")}
    assert want <= combos, sorted(want - combos)
    assert {(e, m) for (_, _, _, e, m, off) in CELLS if off == 1} == {(e, m) for e, m, off in PY_ENTRIES if off == 1}
    for name, L in R.LAYOUTS.items():
        for cname in R.count_vectors(L):
            assert any(cell[0] == name and cell[1] == cname for cell in CELLS), (name, cname)
    for seq in SEQUENCES:
        assert ("sequence", seq, "counts") in OTHER, seq
    assert ("sequence", "ratio_overflow_then_uniform", "ratio") in OTHER
    assert all(("evict", mode, j) in OTHER for mode in (0, 2) for j in range(N_EVICT + 1))
    assert {("errors", "counts"), ("errors", "ratio"), ("errors", "counts over n")} <= OTHER
    for name, L in R.LAYOUTS.items():
        for m in R.check_messages(L):
            assert ("check", name, m) in OTHER, (name, m)
        for m in R.dup_messages(L):
            assert ("dups", name, m) in OTHER, (name, m)
