"""The QSGD decoder's edges against numpy's fp32 arithmetic (qsgd_matrix_inputs.decode_ref: the op
sequence of oracle.qsgd_dequantize; tests/test_qsgd_matrix_host.py holds the two together and to the
reference-generated fixtures).

The arena has tiny and odd tensors, caller-chosen gaps, starts at multiples of 4, one tensor with whole
4096-blocks inside it and six table blocks.  Levels that fp32 cannot represent, int32 payload values
above 2^24 and INT32_MIN, int8 -128, norms of 0, -0.0, 1e-40, 3e38, inf and NaN; plain and accumulating;
the whole arena, block ranges called directly (``elems``), and arenas of fewer than 4 elements (the
byte-load item decoder), for which each encoder is also held to the oracle.

Non-NaN results are compared bit for bit (signed zeros count); NaN positions must coincide.  The padding
holds a canary that must survive.
"""

import numpy as np
import pytest
import torch

import oracle
import qsgd_matrix_inputs as M
from omnifed_amd import codec

pytestmark = pytest.mark.gpu

CANARY = np.float32(-12345.5)
BLK = codec.DECODE_BLOCK
CASES = [(w, lv) for w in (8, 32) for lv in M.DEC_LEVELS[w]]


def same_floats(got, want):
    """Bit-equal where the reference is not NaN, NaN exactly where it is."""
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all())


def _first(got, want):
    nan = np.isnan(want)
    bad = np.flatnonzero((np.isnan(got) != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32))))
    return None if not bad.size else (int(bad.size), int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


class Arena:
    def __init__(self, gpu):
        self.gpu = gpu
        self.offsets, self.end = M.dec_layout()
        self.sizes = M.DEC_SIZES
        self.plan = codec.Plan(self.sizes, offsets=self.offsets, device=gpu)
        assert self.plan.arena_end == self.end and -(-self.end // BLK) >= 5
        self.ranges = list(zip(self.offsets, self.sizes))
        self.pad = np.ones(self.end, bool)
        for o, n in self.ranges:
            self.pad[o:o + n] = False
        self.prev = (np.random.default_rng(5).standard_normal(self.end) * 0.5).astype(np.float32)
        self.prev[self.pad] = CANARY

    def case(self, width, levels, k=0):
        """(q, norms, the plain decode, prev + decode), padding a canary in both references."""
        q = M.dec_payload(width, levels, self.end)
        norms = np.array([M.DEC_NORMS[(t + k) % len(M.DEC_NORMS)] for t in range(len(self.sizes))], np.float32)
        plain = np.full(self.end, CANARY, np.float32)
        acc = self.prev.copy()
        with np.errstate(all="ignore"):
            for t, (o, n) in enumerate(self.ranges):
                plain[o:o + n] = M.decode_ref(q[o:o + n], norms[t], levels)
                acc[o:o + n] = self.prev[o:o + n] + plain[o:o + n]
        return q, norms, plain, acc

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.gpu)

    def canaries(self):
        return torch.full((self.end,), float(CANARY), dtype=torch.float32, device=self.gpu)


@pytest.fixture(scope="module")
def arena(gpu):
    return Arena(gpu)


@pytest.mark.parametrize("width,levels", CASES)
def test_decode_levels_payloads_norms(arena, width, levels):
    """Every norm of DEC_NORMS meets every tensor (the cycle is shifted eight times), plain and accumulating."""
    for k in range(len(M.DEC_NORMS)):
        q, norms, plain, acc = arena.case(width, levels, k)
        qd, nd = arena.dev(q), arena.dev(norms)
        y = arena.canaries()
        arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y)
        got = y.cpu().numpy()
        assert same_floats(got, plain), (width, levels, k, _first(got, plain))
        y = arena.dev(arena.prev)
        arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y, accumulate=True)
        got = y.cpu().numpy()
        assert same_floats(got, acc), (width, levels, k, "accumulate", _first(got, acc))


CUTS = (0, 1, 4095, 4097, 12288, 20000)


@pytest.mark.parametrize("width,levels", [(8, 10), (8, 16), (32, 1000), (32, 1 << 24)])
def test_decode_range_partition_off_block_boundaries(arena, width, levels):
    """Decoded piece by piece at cuts that are not block boundaries: after each piece every block that
    overlaps [0, cut) holds the full decode's bytes and every block wholly beyond it the canary."""
    q, norms, plain, _ = arena.case(width, levels, 2)
    qd, nd = arena.dev(q), arena.dev(norms)
    cuts = CUTS + (arena.end,)
    assert cuts[-2] < arena.end
    y = arena.canaries()
    for b, e in zip(cuts[:-1], cuts[1:]):
        arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y, elems=(b, e))
        done = min(-(-e // BLK) * BLK, arena.end)
        got = y.cpu().numpy()
        assert same_floats(got[:done], plain[:done]), (b, e, _first(got[:done], plain[:done]))
        assert (got[done:] == CANARY).all(), (b, e)


@pytest.mark.parametrize("width,levels", [(8, 10), (32, 256)])
def test_decode_range_accumulate_clip_and_bad_ranges(arena, width, levels):
    q, norms, plain, acc = arena.case(width, levels, 3)
    qd, nd = arena.dev(q), arena.dev(norms)
    # accumulate over a partition at multiples of 4096 equals one full accumulate
    y = arena.dev(arena.prev)
    for b in range(0, arena.end, 2 * BLK):
        arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y, accumulate=True, elems=(b, b + 2 * BLK))  # the last is clipped
    got = y.cpu().numpy()
    assert same_floats(got, acc), _first(got, acc)
    # a range past arena_end is clipped; one wholly beyond it decodes nothing
    y = arena.canaries()
    arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y, elems=(arena.end + BLK, arena.end + 3 * BLK))
    assert (y.cpu().numpy() == CANARY).all()
    last = (arena.end - 1) // BLK * BLK
    arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y, elems=(last + 1, 1 << 40))
    got = y.cpu().numpy()
    assert (got[:last] == CANARY).all() and same_floats(got[last:], plain[last:])
    for bad in ((-1, 5), (5, 4), (-8, -4), (BLK, 0)):
        with pytest.raises(ValueError):
            arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y, elems=bad)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("width,levels", [(8, 16), (8, 10), (32, 256), (32, 1000)])
def test_decode_empty_range_writes_nothing(arena, width, levels, accumulate):
    """An empty range overlaps no block wherever it lies, on a block boundary or not."""
    q, norms, _, _ = arena.case(width, levels, 2)
    qd, nd = arena.dev(q), arena.dev(norms)
    y = arena.dev(arena.prev)
    for b in (0, 1, 5, BLK - 1, BLK, BLK + 1, 3 * BLK + 77, arena.end - 1, arena.end, arena.end + 5, 10 * BLK + 3):
        arena.plan.qsgd_decode(qd, width, levels, nd, y_out=y, accumulate=accumulate, elems=(b, b))
    assert y.cpu().numpy().tobytes() == arena.prev.tobytes()


# ------------------------------------------------------------------ arenas of fewer than 4 elements

@pytest.mark.parametrize("n", [3, 1])
def test_tiny_arena_decode(gpu, n):
    """Plans [3] and [1]: the byte-load item decoder, both widths, plain, accumulating and with elems."""
    plan = codec.Plan([n], device=gpu)
    assert plan.arena_end == n < 4
    prev = np.array([0.25, -1.5, 3.0][:n], np.float32)
    for width, levels, qs in ((8, 16, [-128, 127, -7]), (8, 10, [5, -128, 0]), (32, 256, [-(1 << 31), 300, -1]),
                              (32, 1000, [(1 << 24) + 1, -1000, 0])):
        q = np.array(qs[:n], np.int8 if width == 8 else np.int32)
        qbuf = np.full(plan.payload_elems(width), 0x55, q.dtype)  # bytes past the payload are not the decoder's
        qbuf[:n] = q
        qd = torch.from_numpy(qbuf).to(gpu)
        for norm in (0.37, -0.0, 3e38, float("nan")):
            nd = torch.tensor([norm], dtype=torch.float32, device=gpu)
            want = M.decode_ref(q, norm, levels)
            with np.errstate(all="ignore"):
                want_acc = prev + want
            for elems in (None, (0, n), (1, 2), (0, 10 * BLK)):
                y = torch.from_numpy(prev.copy()).to(gpu)
                plan.qsgd_decode(qd, width, levels, nd, y_out=y, elems=elems)
                assert same_floats(y.cpu().numpy(), want), (width, levels, norm, elems)
                plan.qsgd_decode(qd, width, levels, nd, y_out=y, accumulate=True, elems=elems)
                with np.errstate(all="ignore"):
                    assert same_floats(y.cpu().numpy(), want + want), (width, levels, norm, elems, "accumulate")
                y = torch.from_numpy(prev.copy()).to(gpu)
                plan.qsgd_decode(qd, width, levels, nd, y_out=y, accumulate=True, elems=elems)
                assert same_floats(y.cpu().numpy(), want_acc), (width, levels, norm, elems, "accumulate on prev")
            y = torch.from_numpy(prev.copy()).to(gpu)
            for empty in ((0, 0), (2, 2), (BLK, BLK)):
                plan.qsgd_decode(qd, width, levels, nd, y_out=y, accumulate=True, elems=empty)
            assert y.cpu().numpy().tobytes() == prev.tobytes(), (width, levels, norm, "an empty range wrote")
    with pytest.raises(ValueError):
        plan.qsgd_decode(qd, 32, 1000, nd, y_out=y, elems=(2, 1))


@pytest.mark.parametrize("strategy", codec.STRATEGIES)
@pytest.mark.parametrize("n", [3, 1])
def test_tiny_arena_encode_equals_oracle(gpu, n, strategy):
    """Plans [3] and [1], every strategy, s = 4 (int8, one partial dword) and s = 8 (int32)."""
    plan = codec.Plan([n], device=gpu)
    plan.set_encode_strategy(strategy)
    x = np.array([0.3, -0.0, -0.45][:n], np.float32)
    xd = torch.from_numpy(x).to(gpu)
    seed, off = 0x0123_4567_89AB_CDEF, 11
    u = torch.from_numpy(oracle.philox_uniforms(seed, off, 0, n))
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for s in (4, 8):
            width = codec.storage_width(2 ** s)
            q = torch.full((plan.payload_elems(width),), 0x55 if width == 8 else 0x55555555,
                           dtype=torch.int8 if width == 8 else torch.int32, device=gpu)
            _, norms = plan.qsgd_encode(xd, s, q_out=q, seed=seed, offset=off)
            assert plan.check()
            norm = float(norms.cpu()[0])
            ref = M.norm64(x)
            assert abs(norm - ref) <= 2e-6 * ref, (s, norm, ref)
            want, *_ = oracle.qsgd_quantize(torch.from_numpy(x.copy()), s, norm=norm, u=u)
            qh = q.cpu().numpy()
            assert qh[:n].tobytes() == want.numpy().tobytes(), (s, qh[:n], want)
            if width == 8:  # the rest of the one dword: untouched or zero
                assert all(v in (0x55, 0) for v in qh[n:].tolist()), (s, qh)
    finally:
        torch.set_num_threads(old)
