"""K clients' QSGD payloads decoded and summed in one pass (omf_qsgd_decode_sum), byte for byte against
(a) numpy's fp32 restatement — qsgd_matrix_inputs.decode_ref terms added in client order from +0.0, then
one IEEE division — and (b) the sequence it replaces on the GPU: zeros, K accumulating decodes, div_.

The arena is the decode matrix's (11 tensors of 1 to 13001 elements, starts at multiples of 4, caller
gaps, boundary blocks and whole blocks).  Client k's payload is dec_payload rolled 7·k elements and negated
for odd k; its norms are FIN shifted by k.  No tolerance anywhere: every comparison is on bytes (NaN
positions for the non-finite norms, as in the decode matrix).
"""

import numpy as np
import pytest
import torch

import qsgd_matrix_inputs as M
from omnifed_amd import _lib, codec, ps, shapes

pytestmark = pytest.mark.gpu

CANARY = np.float32(-12345.5)
FIN = (0.0, -0.0, 1.0, 0.37, 1e-40, 2.5e-3, 7.0)
CASES = [(8, 16), (8, 10), (8, 127), (32, 256), (32, 1000), (32, (1 << 24) + 1)]
KS = (1, 2, 3, 8, 9, 17)
DIVISORS = (None, 3.0, 37.0)


def same_floats(got, want):
    """Bit-equal where the reference is not NaN, NaN exactly where it is."""
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def _first(got, want):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    return None if not bad.size else (int(bad.size), int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


def _qdtype(width):
    return np.int8 if width == 8 else np.int32


class Arena:
    def __init__(self, gpu, sizes=None, offsets=None):
        self.gpu = gpu
        if sizes is None:
            sizes = M.DEC_SIZES
            offsets, _ = M.dec_layout()
        self.plan = codec.Plan(sizes, offsets=offsets, device=gpu)
        self.sizes, self.offsets, self.end = self.plan.sizes, self.plan.offsets, self.plan.arena_end
        self.ranges = list(zip(self.offsets, self.sizes))
        self.pad = np.ones(self.end, bool)
        for o, n in self.ranges:
            self.pad[o:o + n] = False
        self.prev = (np.random.default_rng(5).standard_normal(self.end) * 0.5).astype(np.float32)
        self.prev[self.pad] = CANARY
        self._clients = {}

    def clients(self, width, levels, norm_list=FIN):
        """17 clients' (payload arena of payload_elems, norms, decoded terms with +0 in the padding);
        computed once per (width, levels, norm list) and never changed."""
        key = (width, levels, norm_list)
        if key not in self._clients:
            base = M.dec_payload(width, levels, self.end)
            out = []
            for k in range(max(KS)):
                q = np.roll(base, 7 * k)
                if k % 2:
                    q = np.negative(q)  # wraps at the type's minimum, like the device's integer negate would
                buf = np.full(self.plan.payload_elems(width), 0x55, _qdtype(width))  # bytes past the arena: not the decoder's
                buf[:self.end] = q
                norms = np.array([norm_list[(t + k) % len(norm_list)] for t in range(len(self.sizes))], np.float32)
                term = np.zeros(self.end, np.float32)
                for t, (o, n) in enumerate(self.ranges):
                    term[o:o + n] = M.decode_ref(q[o:o + n], norms[t], levels)
                out.append((buf, norms, term))
            self._clients[key] = out
        return self._clients[key]

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.gpu)

    def tensors_only(self, a):
        return a[~self.pad]


def ref_sum(arena, terms, start=None, divisor=None, order=None):
    """numpy: s = start (or +0); s = fl32(s + term_k) over the tensors' elements in order; then / divisor on
    the tensors' elements, and — from +0 — on the padding too (0 / divisor)."""
    s = np.zeros(arena.end, np.float32) if start is None else start.copy()
    with np.errstate(all="ignore"):
        for k in (range(len(terms)) if order is None else order):
            s[~arena.pad] = s[~arena.pad] + terms[k][~arena.pad]
        if divisor is not None:
            where = np.ones(arena.end, bool) if start is None else ~arena.pad
            s[where] = s[where] / np.float32(divisor)
    return s


def gpu_sequence(arena, cl, width, levels, K, start=None, divisor=None, tensors_only=False):
    """Today's sequence: zeros (or start), K accumulating decodes in order, then the division."""
    y = torch.zeros(arena.end, dtype=torch.float32, device=arena.gpu) if start is None else arena.dev(start)
    for q, norms, _ in cl[:K]:
        arena.plan.qsgd_decode(arena.dev(q), width, levels, arena.dev(norms), y_out=y, accumulate=True)
    if divisor is not None and not tensors_only:
        codec.div_(y, divisor)
    out = y.cpu().numpy()
    if divisor is not None and tensors_only:
        out[~arena.pad] = out[~arena.pad] / np.float32(divisor)  # IEEE fp32 division, as div_
    return out


def fused(arena, cl, width, levels, K, y=None, init=False, divisor=None):
    qs = [arena.dev(c[0]) for c in cl[:K]]
    ns = [arena.dev(c[1]) for c in cl[:K]]
    return arena.plan.qsgd_decode_sum(qs, width, levels, ns, y_out=y, init=init, divisor=divisor).cpu().numpy()


@pytest.fixture(scope="module")
def arena(gpu):
    return Arena(gpu)


# ------------------------------------------------------------------ 1. the matrix

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("width,levels", CASES)
def test_sum_matrix(arena, width, levels, K):
    cl = arena.clients(width, levels)
    terms = [c[2] for c in cl[:K]]
    for divisor in DIVISORS:
        want = ref_sum(arena, terms, divisor=divisor)
        assert np.isfinite(want).all()
        # A sum can tell an order from its reverse only with three or more terms that take part in the
        # rounding: fp32 addition commutes (K <= 2), and any three consecutive norms of FIN hold at most two
        # that are neither a zero nor 1e-40, whose term the others absorb whole (K = 3).  From K = 8 on every
        # tensor meets every norm.
        if K >= 8:
            back = ref_sum(arena, terms, divisor=divisor, order=range(K - 1, -1, -1))
            assert (back.view(np.uint32) != want.view(np.uint32)).any(), "the reversed order gives the same bytes"
        y = torch.full((arena.end,), float(CANARY), dtype=torch.float32, device=arena.gpu)  # init=False never reads it
        got = fused(arena, cl, width, levels, K, y=y, divisor=divisor)
        assert got.tobytes() == want.tobytes(), (width, levels, K, divisor, "numpy", _first(got, want))
        seq = gpu_sequence(arena, cl, width, levels, K, divisor=divisor)
        assert got.tobytes() == seq.tobytes(), (width, levels, K, divisor, "gpu sequence", _first(got, seq))


@pytest.mark.parametrize("width,levels", [(8, 16), (8, 10), (32, 256), (32, 1000)])
def test_lone_negative_zero_term_gives_positive_zero(arena, width, levels):
    """zero the arena, then accumulate: +0 + -0 = +0, where the plain decode stores -0."""
    q = arena.dev(np.zeros(arena.plan.payload_elems(width), _qdtype(width)))
    nd = arena.dev(np.full(len(arena.sizes), -0.0, np.float32))
    plain = arena.plan.qsgd_decode(q, width, levels, nd).cpu().numpy()
    got = arena.plan.qsgd_decode_sum([q], width, levels, [nd]).cpu().numpy()
    t = ~arena.pad
    assert (plain[t].view(np.uint32) == 0x80000000).all()
    assert (got.view(np.uint32) == 0).all()


# ------------------------------------------------------------------ 2. non-finite norms

@pytest.mark.parametrize("width,levels", [(8, 10), (32, 1000)])
def test_non_finite_norms(arena, width, levels):
    """DEC_NORMS as they are (inf, NaN, 3e38 among them): NaN where the reference has NaN, bits elsewhere."""
    cl = arena.clients(width, levels, M.DEC_NORMS)
    for K, divisor in ((3, None), (2, 3.0)):  # nine clients would bring a NaN norm to every tensor
        want = ref_sum(arena, [c[2] for c in cl[:K]], divisor=divisor)
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want[~arena.pad]).any()
        got = fused(arena, cl, width, levels, K, divisor=divisor)
        assert same_floats(got, want), (width, levels, K, divisor)
        assert same_floats(got, gpu_sequence(arena, cl, width, levels, K, divisor=divisor)), (width, levels, K, divisor)


# ------------------------------------------------------------------ 3. init=True

@pytest.mark.parametrize("divisor", [None, 3.0])
@pytest.mark.parametrize("K", [1, 8, 9, 17])  # 17 = 8 + 8 + 1: a middle group (from y, no fill, no division)
@pytest.mark.parametrize("width,levels", [(8, 16), (8, 10), (32, 256), (32, 1000)])
def test_init_extends_y_and_keeps_padding(arena, width, levels, K, divisor):
    cl = arena.clients(width, levels)
    want = ref_sum(arena, [c[2] for c in cl[:K]], start=arena.prev, divisor=divisor)
    seq = gpu_sequence(arena, cl, width, levels, K, start=arena.prev, divisor=divisor, tensors_only=True)
    assert seq.tobytes() == want.tobytes()
    got = fused(arena, cl, width, levels, K, y=arena.dev(arena.prev), init=True, divisor=divisor)
    assert (got[arena.pad] == CANARY).all(), "a padding element was written"
    assert got.tobytes() == want.tobytes(), (width, levels, K, divisor, _first(got, want))


# ------------------------------------------------------------------ 4. tiny arenas

@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("width,levels", [(8, 16), (8, 10), (32, 256), (32, 1000)])
@pytest.mark.parametrize("sizes", [[3], [1, 2]])
def test_tiny_arenas(gpu, sizes, width, levels, init):
    """[3]: fewer than 4 elements, the byte-load path.  [1, 2]: two tensors and a gap in one boundary block."""
    ar = Arena(gpu, sizes)
    assert (ar.end < 4) == (sizes == [3])
    cl = ar.clients(width, levels)
    K = 3
    for divisor in (None, 3.0):
        start = ar.prev if init else None
        want = ref_sum(ar, [c[2] for c in cl[:K]], start=start, divisor=divisor)
        y = ar.dev(ar.prev) if init else None
        got = fused(ar, cl, width, levels, K, y=y, init=init, divisor=divisor)
        assert got.tobytes() == want.tobytes(), (sizes, width, levels, init, divisor, got, want)
        seq = gpu_sequence(ar, cl, width, levels, K, start=start, divisor=divisor, tensors_only=init)
        assert got.tobytes() == seq.tobytes(), (sizes, width, levels, init, divisor)


# ------------------------------------------------------------------ 5. refusals

@pytest.mark.parametrize("width,levels", [(8, 16), (32, 1000)])
def test_refusals_leave_y_untouched(arena, width, levels):
    cl = arena.clients(width, levels)
    qs = [arena.dev(c[0]) for c in cl[:3]]
    ns = [arena.dev(c[1]) for c in cl[:3]]
    y = arena.dev(arena.prev)
    plan = arena.plan
    with pytest.raises(ValueError):  # K = 0
        plan.qsgd_decode_sum([], width, levels, [], y_out=y)
    with pytest.raises((TypeError, ValueError)):  # a None entry
        plan.qsgd_decode_sum([qs[0], None, qs[2]], width, levels, ns, y_out=y)
    with pytest.raises((TypeError, ValueError)):
        plan.qsgd_decode_sum(qs, width, levels, [ns[0], ns[1], None], y_out=y)
    with pytest.raises(ValueError):  # a payload one element short
        plan.qsgd_decode_sum([qs[0], qs[1][:plan.payload_elems(width) - 1], qs[2]], width, levels, ns, y_out=y)
    with pytest.raises(ValueError):
        plan.qsgd_decode_sum(qs, 16, levels, ns, y_out=y)
    with pytest.raises(ValueError):
        plan.qsgd_decode_sum(qs, width, 0, ns, y_out=y)
    # the C ABI's own checks (the binding stops most of them earlier): K = 0, a NULL entry, y_out over a payload
    import ctypes
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(arena.gpu).cuda_stream)
    qp = (ctypes.c_void_p * 3)(*[q.data_ptr() for q in qs])
    npp = (ctypes.c_void_p * 3)(*[n.data_ptr() for n in ns])
    yp = ctypes.c_void_p(y.data_ptr())
    assert L.omf_qsgd_decode_sum(plan.handle, qp, npp, 0, width, levels, yp, 0, 0.0, st) == _lib.OMF_EINVAL
    hole = (ctypes.c_void_p * 3)(qs[0].data_ptr(), None, qs[2].data_ptr())
    assert L.omf_qsgd_decode_sum(plan.handle, hole, npp, 3, width, levels, yp, 0, 0.0, st) == _lib.OMF_EINVAL
    assert L.omf_qsgd_decode_sum(plan.handle, qp, hole, 3, width, levels, yp, 0, 0.0, st) == _lib.OMF_EINVAL
    big = torch.zeros(arena.end + 8, dtype=torch.float32, device=arena.gpu)  # y_out aliasing a payload
    alias_q = big.view(torch.int8 if width == 8 else torch.int32)[:plan.payload_elems(width)]
    with pytest.raises(ValueError):
        plan.qsgd_decode_sum([qs[0], alias_q], width, levels, ns[:2], y_out=big[:arena.end])
    with pytest.raises(ValueError):  # ... ending inside it
        plan.qsgd_decode_sum([qs[0], alias_q], width, levels, ns[:2], y_out=big[4:arena.end + 4])
    with pytest.raises(ValueError):  # ... and a norm buffer
        plan.qsgd_decode_sum(qs[:1], width, levels, [big[8:8 + len(arena.sizes)]], y_out=big[:arena.end])
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == arena.prev.tobytes()
    assert not big.cpu().numpy().any()


# ------------------------------------------------------------------ 6. graph capture

def test_graph_capture_two_chained_launches(arena):
    """K = 9 is two launches, one after the other: captured once, replayed twice, the eager bytes each time."""
    width, levels, K, divisor = 8, 16, 9, 3.0
    cl = arena.clients(width, levels)
    qs = [arena.dev(c[0]) for c in cl[:K]]
    ns = [arena.dev(c[1]) for c in cl[:K]]
    eager = arena.plan.qsgd_decode_sum(qs, width, levels, ns, divisor=divisor).cpu().numpy()
    y = torch.empty(arena.end, dtype=torch.float32, device=arena.gpu)
    s = torch.cuda.Stream(arena.gpu)
    s.wait_stream(torch.cuda.current_stream(arena.gpu))
    with torch.cuda.stream(s):  # warm on the capture stream
        arena.plan.qsgd_decode_sum(qs, width, levels, ns, y_out=y, divisor=divisor)
    torch.cuda.current_stream(arena.gpu).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        arena.plan.qsgd_decode_sum(qs, width, levels, ns, y_out=y, divisor=divisor)
    for _ in range(2):
        y.fill_(float(CANARY))
        graph.replay()
        torch.cuda.synchronize()
        assert y.cpu().numpy().tobytes() == eager.tobytes()


# ------------------------------------------------------------------ 7. ps.sum_payloads

class LoopOps:
    """GpuOps without decode_sum: sum_payloads takes today's zero / decode loop / divide."""

    def __init__(self, ops):
        self.plan = ops.plan
        self.decode = ops.decode
        self.div_ = ops.div_


class NoDecodeOps(ps.GpuOps):
    def decode(self, *a, **k):
        raise AssertionError("the per-client decode ran")


@pytest.mark.parametrize("bits", [4, 8])
def test_sum_payloads_equals_the_loop(gpu, bits):
    named = shapes.model_shapes("resnet18")
    plan = codec.Plan.get([shapes.numel(s) for _, s in named], device=gpu)
    levels = 2 ** bits
    width = codec.storage_width(levels)
    g = torch.Generator(device=gpu).manual_seed(31 + bits)
    bufs = []
    for k in range(4):
        x = torch.randn(plan.arena_end, device=gpu, generator=g) * 1e-2
        bufs.append(ps.GpuOps(plan, seed=9, rank=k).encode(x, bits, float(k + 1), 5))
    assert plan.check()
    total = 10.0
    canary = lambda: torch.full((plan.arena_end,), float(CANARY), dtype=torch.float32, device=gpu)
    ops = ps.GpuOps(plan, seed=9, rank=0)
    one = ps.sum_payloads(bufs, width, levels, canary(), total, ops).cpu().numpy()
    loop = ps.sum_payloads(bufs, width, levels, canary(), total, LoopOps(ops)).cpu().numpy()
    assert one.tobytes() == loop.tobytes(), _first(one, loop)
    assert np.abs(one).max() > 0
    took = ps.sum_payloads(bufs, width, levels, canary(), total, NoDecodeOps(plan, seed=9, rank=0)).cpu().numpy()
    assert took.tobytes() == loop.tobytes()
    with pytest.raises(AssertionError):  # and the wrapper's loop does go through decode
        lo = LoopOps(ops)
        lo.decode = NoDecodeOps(plan, seed=9, rank=0).decode
        ps.sum_payloads(bufs, width, levels, canary(), total, lo)


# ------------------------------------------------------------------ 8. DeviceAggregator.accumulate_many

NAMED = [("a", (5,)), ("b", (64,)), ("c", (1000,)), ("d", (4097,)), ("e", (13001,)), ("f", (9,))]


def _client(gpu, k, comp):
    from omnifed_amd.hybrid.communicator.global_grpc_compression import encode_updates_dict

    g = torch.Generator().manual_seed(100 + k)
    upd = {n: (torch.randn(s, generator=g) * (0.1 + k)).to(gpu) for n, s in NAMED}
    return encode_updates_dict(upd, comp, weight=k + 2)


def _qsgd(bits, k):
    from omnifed_amd.hybrid.compression.qsgd import QSGDQuantCompression

    torch.manual_seed(500 + k)
    return QSGDQuantCompression(bit_width=bits)


def _pair(gpu):
    return ps.DeviceAggregator(NAMED, device=gpu), ps.DeviceAggregator(NAMED, device=gpu)


def _same_state(many, one):
    assert many.acc.cpu().numpy().tobytes() == one.acc.cpu().numpy().tobytes()
    assert (many.update_count, many.total_samples) == (one.update_count, one.total_samples)
    assert np.abs(one.acc.cpu().numpy()).max() > 0


@pytest.mark.parametrize("bits", [(4, 4, 4), (4, 4, 8, 4)], ids=["one-run", "mixed-runs"])
def test_accumulate_many_qsgd_runs(gpu, bits, monkeypatch):
    updates = [(_client(gpu, k, _qsgd(b, k)), 10 + k) for k, b in enumerate(bits)]
    many, one = _pair(gpu)
    for layers, ns in updates:
        one.accumulate_layers(layers, ns)
    calls = []
    real = many.plan.qsgd_decode_sum
    monkeypatch.setattr(many.plan, "qsgd_decode_sum", lambda qs, *a, **k: (calls.append(len(qs)), real(qs, *a, **k))[1])
    many.accumulate_many(updates)
    _same_state(many, one)
    assert calls == ([3] if len(bits) == 3 else [2, 1, 1])
    many.reset()
    calls.clear()
    many.accumulate_many(updates, max_batch=2)  # a run is at most max_batch long
    _same_state(many, one)
    assert calls == ([2, 1] if len(bits) == 3 else [2, 1, 1])


def test_accumulate_many_topk_between_qsgd(gpu):
    from omnifed_amd.hybrid.compression.topk import TopKCompression

    updates = [(_client(gpu, 0, _qsgd(4, 0)), 3), (_client(gpu, 1, TopKCompression(device=gpu, compress_ratio=0.05)), 4),
               (_client(gpu, 2, _qsgd(4, 2)), 5)]
    many, one = _pair(gpu)
    for layers, ns in updates:
        one.accumulate_layers(layers, ns)
    many.accumulate_many(updates)
    _same_state(many, one)


def test_accumulate_many_bad_update_applies_what_came_before(gpu):
    from omnifed_amd.hybrid.communicator import global_grpc_pb2 as pb

    updates = [(_client(gpu, k, _qsgd(4, k)), 10 + k) for k in range(4)]
    bad = []
    for L in updates[2][0]:
        C = pb.LayerState()
        C.CopyFrom(L)
        if L.layer_name == "d":
            C.values_data = L.values_data[:-1]
        bad.append(C)
    updates[2] = (bad, updates[2][1])
    many, one = _pair(gpu)
    for layers, ns in updates[:2]:
        one.accumulate_layers(layers, ns)
    with pytest.raises(ValueError):
        one.accumulate_layers(*updates[2])
    with pytest.raises(ValueError):
        many.accumulate_many(updates)
    _same_state(many, one)  # two applied, the third refused, the fourth not applied
    assert many.update_count == 2


def test_accumulate_many_missing_layer_and_stale(gpu):
    updates = [(_client(gpu, k, _qsgd(4, k)), 10 + k) for k in range(3)]
    updates[1] = ([L for L in updates[1][0] if L.layer_name != "c"], updates[1][1])  # norm 0 for it
    many, one = _pair(gpu)
    for layers, ns in updates:
        one.accumulate_layers(layers, ns)
    many.accumulate_many(updates)
    _same_state(many, one)
    many._stale = True  # as accumulate_apply_encode(keep_sum=False) leaves it
    with pytest.raises(RuntimeError):
        many.accumulate_many(updates)
