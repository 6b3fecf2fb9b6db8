"""K clients' PACKED QSGD payloads decoded and summed in one pass (omf_qsgd_decode_sum_packed), byte for
byte against (i) numpy's fp32 restatement — qsgd_matrix_inputs.decode_ref terms added in client order from
+0.0, then one IEEE division —, (ii) the sequence it replaces on the GPU: zeros, K accumulating packed
decodes, div_, and (iii) omf_qsgd_decode_sum on the same levels unpacked.

The arena is this file's own: offsets that are multiples of 32 (the packed wire's rule), 77673 elements,
tensors of 1, 31, 32, 33, 5, 4097, 1000, 40000, 8192, 8193 and 13001 elements.  The 40000 hold 8 Ki blocks
wholly inside one tensor and blocks that cross out of it; there is a caller gap of exactly one 32-group
(96..128), a gap of whole groups on both sides of the 8 Ki boundary at 8192 (8104..8256), a larger one
(4321..7104), and arena_end is no multiple of 32.

Client k's levels are dec_payload's, brought into [-L, L] (the packed wire has no code for anything else:
values outside are wrapped modulo 2L + 1, values inside stay), rolled 7·k elements and negated for odd k;
its norms are FIN shifted by k.  Each tensor is packed on the CPU by oracle.bitpack.pack and laid at byte
offsets[t]·b/8 of the packed arena; every other byte of it is 0x55.  No tolerance anywhere: every
comparison is on bytes (NaN positions for the non-finite norms).
"""

import ctypes

import numpy as np
import pytest
import torch

import qsgd_matrix_inputs as M
from oracle import bitpack
from omnifed_amd import _lib, codec

pytestmark = pytest.mark.gpu

CANARY = np.float32(-12345.5)
FIN = (0.0, -0.0, 1.0, 0.37, 1e-40, 2.5e-3, 7.0)
CASES = [(8, 16), (8, 10), (8, 127), (32, 256), (32, 1000), (32, (1 << 24) + 1)]  # b = 6, 5, 8, 10, 11, 26
KS = (1, 2, 3, 8, 9, 17)
DIVISORS = (None, 3.0, 37.0)

SIZES = [1, 31, 32, 33, 5, 4097, 1000, 40000, 8192, 8193, 13001]
OFFSETS = [0, 32, 64, 128, 192, 224, 7104, 8256, 48256, 56448, 64672]


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
    def __init__(self, gpu, sizes=SIZES, offsets=OFFSETS):
        self.gpu = gpu
        self.plan = codec.Plan(sizes, offsets=offsets, device=gpu)
        self.sizes, self.offsets, self.end = self.plan.sizes, self.plan.offsets, self.plan.arena_end
        assert all(o % 32 == 0 for o in self.offsets)
        self.ranges = list(zip(self.offsets, self.sizes))
        self.pad = np.ones(self.end, bool)
        for o, n in self.ranges:
            self.pad[o:o + n] = False
        self.prev = (np.random.default_rng(5).standard_normal(self.end) * 0.5).astype(np.float32)
        self.prev[self.pad] = CANARY
        self._clients = {}

    def pack(self, q, levels):
        """The packed arena (int32 words) of the levels q: per tensor bitpack.pack, 0x55 elsewhere."""
        b = bitpack.packed_bits(levels)
        raw = np.full(4 * self.plan.packed_words(levels), 0x55, np.uint8)
        for o, n in self.ranges:
            stream = np.frombuffer(bitpack.pack(q[o:o + n], levels), np.uint8)
            assert stream.size == (n * b + 7) // 8
            raw[o * b // 8:o * b // 8 + stream.size] = stream
        return raw.view(np.int32)

    def clients(self, width, levels, norm_list=FIN, count=max(KS)):
        """``count`` clients' (packed arena, norms, decoded terms with +0 in the padding, unpacked payload
        arena); computed once per (width, levels, norm list, count) and never changed."""
        key = (width, levels, norm_list, count)
        if key not in self._clients:
            raw = M.dec_payload(width, levels, self.end).astype(np.int64)
            base = ((raw + levels) % (2 * levels + 1) - levels).astype(_qdtype(width))  # inside [-L, L] unchanged
            out = []
            for k in range(count):
                q = np.roll(base, 7 * k)
                if k % 2:
                    q = np.negative(q)
                buf = np.full(self.plan.payload_elems(width), 0x55, _qdtype(width))
                buf[:self.end] = q
                norms = np.array([norm_list[(t + k) % len(norm_list)] for t in range(len(self.sizes))], np.float32)
                term = np.zeros(self.end, np.float32)
                for t, (o, n) in enumerate(self.ranges):
                    term[o:o + n] = M.decode_ref(q[o:o + n], norms[t], levels)
                out.append((self.pack(q, levels), norms, term, buf))
            self._clients[key] = out
        return self._clients[key]

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.gpu)


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


def gpu_sequence(arena, cl, levels, K, start=None, divisor=None, tensors_only=False):
    """Today's sequence: zeros (or start), K accumulating packed decodes in order, then the division."""
    y = torch.zeros(arena.end, dtype=torch.float32, device=arena.gpu) if start is None else arena.dev(start)
    for c in cl[:K]:
        arena.plan.qsgd_decode_packed(arena.dev(c[0]), levels, arena.dev(c[1]), y_out=y, accumulate=True)
    if divisor is not None and not tensors_only:
        codec.div_(y, divisor)
    out = y.cpu().numpy()
    if divisor is not None and tensors_only:
        out[~arena.pad] = out[~arena.pad] / np.float32(divisor)  # IEEE fp32 division, as div_
    return out


def fused(arena, cl, levels, K, y=None, init=False, divisor=None):
    ps = [arena.dev(c[0]) for c in cl[:K]]
    ns = [arena.dev(c[1]) for c in cl[:K]]
    return arena.plan.qsgd_decode_sum_packed(ps, levels, ns, y_out=y, init=init, divisor=divisor).cpu().numpy()


def unpacked_sum(arena, cl, width, levels, K, y=None, init=False, divisor=None):
    qs = [arena.dev(c[3]) for c in cl[:K]]
    ns = [arena.dev(c[1]) for c in cl[:K]]
    return arena.plan.qsgd_decode_sum(qs, width, levels, ns, y_out=y, init=init, divisor=divisor).cpu().numpy()


@pytest.fixture(scope="module")
def arena(gpu):
    return Arena(gpu)


def test_layout_has_the_cases(arena):
    assert arena.end == 77673 and arena.end % 32
    gaps = [(o + n, o2) for (o, n), o2 in zip(arena.ranges, arena.offsets[1:])]
    assert (96, 128) in gaps  # exactly one 32-group
    assert (8104, 8256) in gaps  # whole padding groups on both sides of the block boundary at 8192
    o, n = arena.ranges[SIZES.index(40000)]
    assert o % 8192 and (o + n) % 8192 and n >= 3 * 8192  # blocks wholly inside, blocks that cross out


# ------------------------------------------------------------------ 1. the matrix

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("width,levels", CASES)
def test_sum_matrix(arena, width, levels, K):
    cl = arena.clients(width, levels)
    terms = [c[2] for c in cl[:K]]
    for divisor in DIVISORS:
        want = ref_sum(arena, terms, divisor=divisor)
        assert np.isfinite(want).all()
        if K >= 8:  # from K = 8 on every tensor meets every norm: the order shows in the bytes
            back = ref_sum(arena, terms, divisor=divisor, order=range(K - 1, -1, -1))
            assert (back.view(np.uint32) != want.view(np.uint32)).any(), "the reversed order gives the same bytes"
        y = torch.full((arena.end,), float(CANARY), dtype=torch.float32, device=arena.gpu)  # init=False never reads it
        got = fused(arena, cl, levels, K, y=y, divisor=divisor)
        assert got.tobytes() == want.tobytes(), (width, levels, K, divisor, "numpy", _first(got, want))
        seq = gpu_sequence(arena, cl, levels, K, divisor=divisor)
        assert got.tobytes() == seq.tobytes(), (width, levels, K, divisor, "gpu sequence", _first(got, seq))
        unp = unpacked_sum(arena, cl, width, levels, K, divisor=divisor)
        assert got.tobytes() == unp.tobytes(), (width, levels, K, divisor, "unpacked sum", _first(got, unp))


@pytest.mark.parametrize("width,levels", [(8, 16), (8, 10), (32, 256), (32, 1000)])
def test_lone_negative_zero_term_gives_positive_zero(arena, width, levels):
    """zero the arena, then accumulate: +0 + -0 = +0, where the plain packed decode stores -0."""
    p = arena.dev(arena.pack(np.zeros(arena.end, _qdtype(width)), levels))
    nd = arena.dev(np.full(len(arena.sizes), -0.0, np.float32))
    plain = arena.plan.qsgd_decode_packed(p, levels, nd).cpu().numpy()
    got = arena.plan.qsgd_decode_sum_packed([p], levels, [nd]).cpu().numpy()
    t = ~arena.pad
    assert (plain[t].view(np.uint32) == 0x80000000).all()
    assert (got.view(np.uint32) == 0).all()


# ------------------------------------------------------------------ 2. non-finite norms

@pytest.mark.parametrize("width,levels", [(8, 10), (32, 1000)])
def test_non_finite_norms(arena, width, levels):
    """DEC_NORMS as they are (inf, NaN, 3e38 among them): NaN where the reference has NaN, bits elsewhere."""
    cl = arena.clients(width, levels, M.DEC_NORMS, count=3)
    for K, divisor in ((3, None), (2, 3.0)):
        want = ref_sum(arena, [c[2] for c in cl[:K]], divisor=divisor)
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want[~arena.pad]).any()
        got = fused(arena, cl, levels, K, divisor=divisor)
        assert same_floats(got, want), (width, levels, K, divisor)
        assert same_floats(got, gpu_sequence(arena, cl, levels, K, divisor=divisor)), (width, levels, K, divisor)
        assert same_floats(got, unpacked_sum(arena, cl, width, levels, K, divisor=divisor)), (width, levels, K, divisor)


# ------------------------------------------------------------------ 3. init=True

@pytest.mark.parametrize("divisor", [None, 3.0])
@pytest.mark.parametrize("K", [1, 8, 9])
@pytest.mark.parametrize("width,levels", [(8, 16), (8, 10), (32, 256), (32, 1000)])
def test_init_extends_y_and_keeps_padding(arena, width, levels, K, divisor):
    cl = arena.clients(width, levels)
    want = ref_sum(arena, [c[2] for c in cl[:K]], start=arena.prev, divisor=divisor)
    seq = gpu_sequence(arena, cl, levels, K, start=arena.prev, divisor=divisor, tensors_only=True)
    assert seq.tobytes() == want.tobytes()
    got = fused(arena, cl, levels, K, y=arena.dev(arena.prev), init=True, divisor=divisor)
    assert (got[arena.pad] == CANARY).all(), "a padding element was written"
    assert got.tobytes() == want.tobytes(), (width, levels, K, divisor, _first(got, want))
    unp = unpacked_sum(arena, cl, width, levels, K, y=arena.dev(arena.prev), init=True, divisor=divisor)
    assert got.tobytes() == unp.tobytes(), (width, levels, K, divisor, _first(got, unp))


# ------------------------------------------------------------------ 4. tiny arenas

@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("width,levels", [(8, 16), (8, 10), (32, 256), (32, 1000)])
@pytest.mark.parametrize("sizes,offsets", [([3], [0]), ([1, 2], [0, 32])])
def test_tiny_arenas(gpu, sizes, offsets, width, levels, init):
    """[3]: less than one group.  [1, 2] at 0 and 32: two partial groups, the second ending the arena."""
    ar = Arena(gpu, sizes, offsets)
    cl = ar.clients(width, levels, count=3)
    K = 3
    for divisor in (None, 3.0):
        start = ar.prev if init else None
        want = ref_sum(ar, [c[2] for c in cl[:K]], start=start, divisor=divisor)
        y = ar.dev(ar.prev) if init else None
        got = fused(ar, cl, levels, K, y=y, init=init, divisor=divisor)
        assert got.tobytes() == want.tobytes(), (sizes, width, levels, init, divisor, got, want)
        seq = gpu_sequence(ar, cl, levels, K, start=start, divisor=divisor, tensors_only=init)
        assert got.tobytes() == seq.tobytes(), (sizes, width, levels, init, divisor)


# ------------------------------------------------------------------ 5. refusals

@pytest.mark.parametrize("width,levels", [(8, 16), (32, 1000)])
def test_refusals_leave_y_untouched(arena, width, levels):
    cl = arena.clients(width, levels)
    ps = [arena.dev(c[0]) for c in cl[:3]]
    ns = [arena.dev(c[1]) for c in cl[:3]]
    y = arena.dev(arena.prev)
    plan = arena.plan
    words = plan.packed_words(levels)
    with pytest.raises(ValueError):  # K = 0
        plan.qsgd_decode_sum_packed([], levels, [], y_out=y)
    with pytest.raises((TypeError, ValueError)):  # a None entry
        plan.qsgd_decode_sum_packed([ps[0], None, ps[2]], levels, ns, y_out=y)
    with pytest.raises((TypeError, ValueError)):
        plan.qsgd_decode_sum_packed(ps, levels, [ns[0], ns[1], None], y_out=y)
    with pytest.raises(ValueError):  # a packed arena one word short
        plan.qsgd_decode_sum_packed([ps[0], ps[1][:words - 1], ps[2]], levels, ns, y_out=y)
    with pytest.raises(ValueError):
        plan.qsgd_decode_sum_packed(ps, 0, ns, y_out=y)
    # a valid plan that is no packed arena: an offset of 4
    odd = codec.Plan([3, 5], offsets=[0, 4], device=arena.gpu)
    yo = torch.full((odd.arena_end,), float(CANARY), dtype=torch.float32, device=arena.gpu)
    po = torch.zeros(odd.packed_words(levels), dtype=torch.int32, device=arena.gpu)
    no = torch.ones(2, dtype=torch.float32, device=arena.gpu)
    with pytest.raises(ValueError):
        odd.qsgd_decode_sum_packed([po], levels, [no], y_out=yo)
    # y_out aliasing a packed arena, ending inside it, and a norm buffer
    big = torch.zeros(arena.end + 8, dtype=torch.float32, device=arena.gpu)
    alias_p = big.view(torch.int32)[:words]
    with pytest.raises(ValueError):
        plan.qsgd_decode_sum_packed([ps[0], alias_p], levels, ns[:2], y_out=big[:arena.end])
    with pytest.raises(ValueError):
        plan.qsgd_decode_sum_packed([ps[0], alias_p], levels, ns[:2], y_out=big[4:arena.end + 4])
    with pytest.raises(ValueError):
        plan.qsgd_decode_sum_packed(ps[:1], levels, [big[8:8 + len(arena.sizes)]], y_out=big[:arena.end])
    # the same through the C ABI alone (the binding stops most of them earlier)
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream(arena.gpu).cuda_stream)
    pp = (ctypes.c_void_p * 3)(*[p.data_ptr() for p in ps])
    npp = (ctypes.c_void_p * 3)(*[n.data_ptr() for n in ns])
    yp = ctypes.c_void_p(y.data_ptr())
    call = L.omf_qsgd_decode_sum_packed
    assert call(plan.handle, pp, npp, 0, levels, yp, 0, 0.0, st) == _lib.OMF_EINVAL
    hole = (ctypes.c_void_p * 3)(ps[0].data_ptr(), None, ps[2].data_ptr())
    assert call(plan.handle, hole, npp, 3, levels, yp, 0, 0.0, st) == _lib.OMF_EINVAL
    assert call(plan.handle, pp, hole, 3, levels, yp, 0, 0.0, st) == _lib.OMF_EINVAL
    assert call(plan.handle, pp, npp, 3, 0, yp, 0, 0.0, st) == _lib.OMF_EINVAL
    assert call(plan.handle, pp, npp, 3, levels, ctypes.c_void_p(y.data_ptr() + 4), 0, 0.0, st) == _lib.OMF_EINVAL
    one_p = (ctypes.c_void_p * 1)(po.data_ptr())
    one_n = (ctypes.c_void_p * 1)(no.data_ptr())
    assert call(odd.handle, one_p, one_n, 1, levels, ctypes.c_void_p(yo.data_ptr()), 0, 0.0, st) == _lib.OMF_EINVAL
    bp = ctypes.c_void_p(big.data_ptr())
    alias = (ctypes.c_void_p * 2)(ps[0].data_ptr(), big.data_ptr() + 4 * (arena.end - 1))  # y_out's last element
    assert call(plan.handle, alias, npp, 2, levels, bp, 0, 0.0, st) == _lib.OMF_EINVAL
    alias_n = (ctypes.c_void_p * 1)(big.data_ptr() + 32)
    assert call(plan.handle, pp, alias_n, 1, levels, bp, 0, 0.0, st) == _lib.OMF_EINVAL
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == arena.prev.tobytes()
    assert not big.cpu().numpy().any()
    assert (yo.cpu().numpy() == CANARY).all()


# ------------------------------------------------------------------ 6. graph capture

def test_graph_capture_two_chained_launches(arena):
    """K = 9 is two launches, one after the other: captured once, replayed twice, the eager bytes each time."""
    width, levels, K, divisor = 8, 16, 9, 3.0
    cl = arena.clients(width, levels)
    ps = [arena.dev(c[0]) for c in cl[:K]]
    ns = [arena.dev(c[1]) for c in cl[:K]]
    eager = arena.plan.qsgd_decode_sum_packed(ps, levels, ns, divisor=divisor).cpu().numpy()
    y = torch.empty(arena.end, dtype=torch.float32, device=arena.gpu)
    s = torch.cuda.Stream(arena.gpu)
    s.wait_stream(torch.cuda.current_stream(arena.gpu))
    with torch.cuda.stream(s):  # warm on the capture stream
        arena.plan.qsgd_decode_sum_packed(ps, levels, ns, y_out=y, divisor=divisor)
    torch.cuda.current_stream(arena.gpu).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        arena.plan.qsgd_decode_sum_packed(ps, levels, ns, y_out=y, divisor=divisor)
    for _ in range(2):
        y.fill_(float(CANARY))
        graph.replay()
        torch.cuda.synchronize()
        assert y.cpu().numpy().tobytes() == eager.tobytes()
