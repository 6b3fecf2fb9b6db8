"""Bucketed QSGD held to the CPU oracle (oracle/qsgd_bucket.py) at every bucket size: the norm bits of every unit
that computes a bucket norm, the levels, packed bytes and decode, the isolation of a bucket from an overflowing,
underflowing or NaN neighbour, every client-count instance of the decode sums and of the PS step, and the PS step
across bucket sizes.

One plan and arena per d in codec.BUCKET_SIZES from tests/golden/qsgd_bucket_inputs.py (the host test
tests/test_qsgd_bucket_oracle_host.py checks what the recipe promises, and that a change of summation order moves
the norm bits of its buckets).  Canaries in the padding (NaN in a 16-bit arena: a padding element that reaches a sum
makes the norm NaN), guards round every output.  The norms are compared by their int32 view — the header of
omf_qsgd_bucket.h promises the bits — except the NaN bucket's, which compares as "is NaN"; its levels are not
asserted.  The oracle has levels for the inf bucket (v / inf = 0: all zero), so they are held like any other."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
import qsgd_bucket_inputs as inp
from omnifed_amd import codec
from oracle import bitpack

pytestmark = pytest.mark.gpu

SIZES = codec.BUCKET_SIZES
SEED, OFF = inp.SEED, inp.OFFSET
GUARD = 64
FCANARY, ICANARY = 3e4, 0x5A5A5A5A
FORMATS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
F32 = np.float32


@pytest.fixture(scope="module")
def arenas(gpu):
    """d -> the plan of the recipe's tensors and, on the host, the canary-padded arena x, a start arena (finite,
    tensor 3 and the first half of ``many`` all -0.0), the mask of the tensors' elements and every element's index
    into the bucket-norm arena."""
    out = {}
    for d in SIZES:
        sizes = inp.sizes(d)
        plan = codec.Plan(sizes, device=gpu)
        boff, nb = plan.bucket_layout(d)
        A = plan.arena_end
        x = np.full(A, FCANARY, dtype=F32)
        start = np.full(A, FCANARY, dtype=F32)
        mask = np.zeros(A, dtype=bool)
        rng = np.random.default_rng(d)
        for t, (o, n) in enumerate(zip(plan.offsets, sizes)):
            x[o:o + n] = inp.make_tensor(d, t)
            start[o:o + n] = (rng.standard_normal(n) * 1e-3).astype(F32)
            mask[o:o + n] = True
        start[plan.offsets[3]:plan.offsets[3] + sizes[3]] = -0.0
        start[plan.offsets[inp.MANY_T]:plan.offsets[inp.MANY_T] + 32 * d] = -0.0
        out[d] = SimpleNamespace(d=d, plan=plan, sizes=sizes, offs=list(plan.offsets), boff=boff, nb=nb, A=A, x=x,
                                 start=start, mask=mask, x_gpu={}, cache={})
    return out


def _bidx(a, d):
    """Every arena element's index into the bucket-norm arena of size d (padding: 0)."""
    key = ("bidx", d)
    if key not in a.cache:
        bidx = np.zeros(a.A, dtype=np.int64)
        for o, n, b in zip(a.offs, a.sizes, a.plan.bucket_layout(d)[0]):
            bidx[o:o + n] = b + np.arange(n) // d
        a.cache[key] = bidx
    return a.cache[key]


def _source(a, fmt, gpu):
    """The arena on the GPU in the format, and its exact fp32 upcast on the host."""
    if fmt not in a.x_gpu:
        x = torch.from_numpy(a.x).to(gpu)
        if fmt != "fp32":
            x = x.to(FORMATS[fmt])
            x[torch.from_numpy(~a.mask).to(gpu)] = float("nan")
        a.x_gpu[fmt] = (x, x.float().cpu().numpy())
    return a.x_gpu[fmt]


def _oracle_norms(a, arena, alpha, d=None):
    """oracle.bucket_norms of fl32(alpha arena), tensor by tensor, as the plan's bucket-norm arena of size d."""
    d = d or a.d
    boff, nb = a.plan.bucket_layout(d)
    out = np.empty(nb, dtype=F32)
    for o, n, b in zip(a.offs, a.sizes, boff):
        out[b:b + -(-n // d)] = oracle.bucket_norms((arena[o:o + n] * F32(alpha)).astype(F32), d)
    return out


def _norms_of(a, fmt, alpha, gpu):
    key = ("norms", fmt, alpha)
    if key not in a.cache:
        a.cache[key] = _oracle_norms(a, _source(a, fmt, gpu)[1], alpha)
    return a.cache[key]


def _oracle_levels(a, arena, s, d=None, bnorm=None, u=None):
    """oracle.encode_bucketed tensor by tensor (alpha 1, the Philox draws of (SEED, OFF) or the arena u): the
    levels as an int64 arena (0 in the padding) and the norms."""
    d = d or a.d
    boff, nb = a.plan.bucket_layout(d)
    lv, bn = np.zeros(a.A, dtype=np.int64), np.empty(nb, dtype=F32)
    for t, (o, n, b) in enumerate(zip(a.offs, a.sizes, boff)):
        ut = oracle.philox_uniforms(SEED, OFF, t, n) if u is None else u[o:o + n]
        q, bt = oracle.encode_bucketed(arena[o:o + n], 1.0, s, d, ut, bnorm=None if bnorm is None else bnorm[b:b + -(-n // d)])
        lv[o:o + n], bn[b:b + bt.size] = q.numpy(), bt
    return lv, bn


def _levels_of(a, s):
    key = ("levels", s)
    if key not in a.cache:
        a.cache[key] = _oracle_levels(a, a.x, s)
    return a.cache[key]


def _nan_elems(a):
    """The mask of the NaN bucket's elements: their levels are not asserted."""
    m = np.zeros(a.A, dtype=bool)
    o = a.offs[inp.NAN_T]
    m[o + a.d:o + 2 * a.d] = True
    return m


def _same_norm_bits(got, want, what):
    g = got.cpu().numpy()
    nan = np.isnan(want)
    assert g.shape == want.shape and np.isnan(g[nan]).all(), what
    diff = np.flatnonzero(g.view(np.int32)[~nan] != want.view(np.int32)[~nan])
    assert diff.size == 0, (what, diff[:8], g[~nan][diff[:8]], want[~nan][diff[:8]])


def _banded(n, fill, dtype, gpu):
    """A guard-banded buffer and the view a call writes."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=gpu)
    return buf, buf[GUARD:GUARD + n]


def _guards_kept(*bufs):
    return all(bool((b[:GUARD] == b[0]).all()) and bool((b[-GUARD:] == b[0]).all()) for b in bufs)


def _written(a, b):
    """The mask of the packed arena's words whose 32-element group holds a tensor element."""
    groups = -(-a.A // 32)
    m = np.zeros(groups * 32, dtype=bool)
    m[:a.A] = a.mask
    return np.repeat(m.reshape(groups, 32).any(axis=1), b)


def _encode(a, x, wire, s, gpu, **kw):
    """One encode into guard-banded canary outputs: (payload on the host, norms, the guards were kept)."""
    L, packed = 2 ** s, wire == "packed"
    n_out = a.plan.packed_words(L) if packed else a.plan.payload_elems(codec.storage_width(L))
    qdt = torch.int8 if wire == "int8" else torch.int32
    qbuf, q = _banded(n_out, 0x55 if wire == "int8" else ICANARY, qdt, gpu)
    nbuf, bn = _banded(a.nb, -7.0, torch.float32, gpu)
    if packed:
        a.plan.qsgd_encode_bucketed_packed(x, s, a.d, packed_out=q, bnorm_out=bn, **kw)
    else:
        assert codec.storage_width(L) == (8 if wire == "int8" else 32)
        a.plan.qsgd_encode_bucketed(x, s, a.d, q_out=q, bnorm_out=bn, **kw)
    torch.cuda.synchronize()
    return q.cpu().numpy(), bn, _guards_kept(qbuf, nbuf)


def _payload_is(a, wire, s, qh, lv, skip):
    """The kernel's payload (host array) holds the levels lv on every tensor element outside `skip`, canaries
    in the padding; on the packed wire: oracle.bitpack's bytes tensor by tensor."""
    L, b = 2 ** s, s + 2
    if wire != "packed":
        canary = 0x55 if wire == "int8" else ICANARY
        assert (qh[:a.A][~a.mask] == canary).all() and (qh[a.A:] == canary).all()
        check = a.mask & ~skip
        bad = np.flatnonzero(qh[:a.A][check].astype(np.int64) != lv[check])
        assert bad.size == 0, (wire, s, np.flatnonzero(check)[bad[:8]])
        return
    assert (qh[~_written(a, b)] == ICANARY).all()
    ph = qh.view(np.uint8)
    for t, (o, n) in enumerate(zip(a.offs, a.sizes)):
        # a bucket begins at a whole byte (d b / 8); the NaN bucket's bytes are left out
        spans = [(0, n)] if not skip[o:o + n].any() else [(j * a.d, (j + 1) * a.d) for j in range(n // a.d) if not skip[o + j * a.d]]
        for lo, hi in spans:
            at = (o + lo) * b // 8
            assert ph[at:at + ((hi - lo) * b + 7) // 8].tobytes() == bitpack.pack(lv[o + lo:o + hi], L), (t, lo)


# ---------------------------------------------------------------- norm bits

@pytest.mark.parametrize("alpha", (1.0, 3.0))
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("d", SIZES)
def test_norm_bits_of_every_encoder_equal_the_oracle(gpu, arenas, d, fmt, alpha):
    a = arenas[d]
    x, _ = _source(a, fmt, gpu)
    before = x.clone()
    want = _norms_of(a, fmt, alpha, gpu)
    assert int(np.isnan(want).sum()) == 1 and np.isnan(want[a.boff[inp.NAN_T] + 1])
    nbuf, bn = _banded(a.nb, -7.0, torch.float32, gpu)
    a.plan.qsgd_norms_bucketed(x, d, alpha=alpha, bnorm_out=bn)
    _same_norm_bits(bn, want, "qsgd_norms_bucketed")
    assert _guards_kept(nbuf)
    for wire, s in (("int8", 4), ("int32", 8), ("packed", 4)):
        _, bn, kept = _encode(a, x, wire, s, gpu, alpha=alpha, seed=SEED, offset=OFF)
        _same_norm_bits(bn, want, wire)
        assert kept, wire
        suffix = "" if fmt == "fp32" else "_h16"
        assert a.plan.last_encoder == ("bucketed_packed" if wire == "packed" else "bucketed") + suffix
    assert torch.equal(x.view(torch.int16 if fmt != "fp32" else torch.int32), before.view(torch.int16 if fmt != "fp32" else torch.int32))


def _messages(a, d_in, L, N, seed0=20):
    """N foreign messages (inp.message) for the plan at bucket size d_in."""
    _, nb = a.plan.bucket_layout(d_in)
    return [inp.message(a.A, nb, L, seed0 + k) for k in range(N)]


def _pack_arena(a, q, L):
    """The packed arena of an arena of levels, by oracle.bitpack (element i at bits [i b, (i + 1) b))."""
    full = np.zeros(-(-a.A // 32) * 32, dtype=np.int64)
    full[:a.A] = q[:a.A]
    return torch.from_numpy(np.frombuffer(bitpack.pack(full, L), dtype=np.int32).copy())


def _upload(a, msgs, width, L, gpu):
    qs = [(_pack_arena(a, q, L) if width == 0 else torch.from_numpy(q.astype(np.int8 if width == 8 else np.int32))).to(gpu)
          for q, _ in msgs]
    return qs, [torch.from_numpy(bn).to(gpu) for _, bn in msgs]


def _sequential_sum(a, msgs, d_in, L, start):
    """The plain fp32 numpy sum in client order."""
    bi = _bidx(a, d_in)
    s = start.copy() if start is not None else np.zeros(a.A, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q, bn in msgs:
            s = (s + inp.decode_np(q, bn, bi, L)).astype(F32)
    return s


def _ps_check(gpu, a, acc_h, d_in, d_out, width_in, L_in, N, start, divisor, s_out, packed):
    """One ps_sum_encode_bucketed call held to the numpy sum, the oracle's norms of the numpy average and the
    oracle's levels; canaries in the padding and the unwritten groups, guards, inputs unchanged."""
    plan, m = a.plan, a.mask
    msgs = _messages(a, d_in, L_in, N)
    qs, bns = _upload(a, msgs, width_in, L_in, gpu)
    keep = [t.clone() for t in qs + bns]
    acc0 = torch.from_numpy(acc_h).to(gpu)
    acc = acc0.clone()
    L, b = 2 ** s_out, s_out + 2
    width = codec.storage_width(L)
    nb = plan.bucket_layout(d_out)[1]
    n_q = plan.packed_words(L) if packed else plan.payload_elems(width)
    wide = packed or width == 32
    abuf, avg_out = _banded(a.A, FCANARY, torch.float32, gpu)
    sbuf, sum_view = _banded(a.A, FCANARY, torch.float32, gpu)
    qbuf, q_out = _banded(n_q, ICANARY if wide else 0x55, torch.int32 if wide else torch.int8, gpu)
    nbuf, bn_out = _banded(nb, -7.0, torch.float32, gpu)
    in_place = start and N % 2 == 1  # sum_out is the accumulator itself
    avg, q, bn = plan.ps_sum_encode_bucketed(
        acc if start else None, qs, bns, width_in, L_in, d_in, divisor, s_out, d_out, pack_out=packed,
        sum_out=acc if in_place else sum_view, avg_out=avg_out, seed=SEED, offset=OFF, q_out=q_out, bnorm_out=bn_out)
    assert plan.last_encoder == "bucketed_ps"
    torch.cuda.synchronize()
    s = _sequential_sum(a, msgs, d_in, L_in, acc_h if start else None)
    with np.errstate(invalid="ignore", over="ignore"):
        want_avg = s if divisor is None else (s / F32(divisor)).astype(F32)
    got_sum, got_avg = (acc if in_place else sum_view).cpu().numpy(), avg.cpu().numpy()
    nan = np.isnan(s)
    assert (np.isnan(got_sum) == nan)[m].all() and (np.isnan(got_avg) == nan)[m].all()
    ok = m & ~nan
    assert np.array_equal(got_sum.view(np.int32)[ok], s.view(np.int32)[ok])
    assert np.array_equal(got_avg.view(np.int32)[ok], want_avg.view(np.int32)[ok])
    assert (got_avg[~m] == F32(FCANARY)).all() and (got_sum[~m] == F32(FCANARY)).all()
    assert _guards_kept(abuf, sbuf, qbuf, nbuf)
    if not in_place:
        assert torch.equal(acc.view(torch.int32), acc0.view(torch.int32))
    assert all(torch.equal(t, k) for t, k in zip(qs + bns, keep))
    _same_norm_bits(bn, _oracle_norms(a, want_avg, 1.0, d_out), ("ps", d_in, d_out, N))
    return want_avg, q.cpu().numpy(), bn.cpu().numpy()


@pytest.mark.parametrize("mode", ("acc_only", "two_clients"))
@pytest.mark.parametrize("d", SIZES)
def test_norm_bits_of_the_ps_step_equal_the_oracle(gpu, arenas, d, mode):
    """The accumulator is the recipe's arena, special buckets included: halved they stay subnormal, zero, inf and NaN."""
    a = arenas[d]
    if mode == "acc_only":
        _ps_check(gpu, a, a.x, d, d, 8, 16, 0, True, 2.0, 4, False)
    else:
        _ps_check(gpu, a, a.x, d, d, 8, 16, 2, True, 7.0, 4, True)


@pytest.mark.parametrize("d", SIZES)
def test_variants_give_the_oracles_bits(gpu, arenas, d):
    a = arenas[d]
    x, _ = _source(a, "fp32", gpu)
    want, (lv, _), skip = _norms_of(a, "fp32", 1.0, gpu), _levels_of(a, 4), _nan_elems(a)
    kw = {"seed": SEED, "offset": OFF}
    for rows, static_d in ((8, True), (16, True), (4, False)):
        try:
            a.plan.set_bucket_rows(rows, static_d)
            qh, bn, kept = _encode(a, x, "int8", 4, gpu, **kw)
            h16 = [(f, _encode(a, _source(a, f, gpu)[0], "int8", 4, gpu, **kw)[1]) for f in ("bf16", "fp16")] if rows == 8 else []
        finally:
            a.plan.set_bucket_rows(4)
        _same_norm_bits(bn, want, ("rows", rows, static_d))
        _payload_is(a, "int8", 4, qh, lv, skip)
        assert kept
        for f, bn16 in h16:
            _same_norm_bits(bn16, _norms_of(a, f, 1.0, gpu), ("rows", rows, f))
    try:
        a.plan.set_bucket_pack(1)
        qh, bn, kept = _encode(a, x, "packed", 4, gpu, **kw)
    finally:
        a.plan.set_bucket_pack(0)
    _same_norm_bits(bn, want, "pack 1")
    _payload_is(a, "packed", 4, qh, lv, skip)
    assert kept


# ---------------------------------------------------------------- levels, bytes, decode

@pytest.mark.parametrize("wire,s", (("int8", 4), ("int32", 8), ("packed", 4), ("packed", 12)))
@pytest.mark.parametrize("d", SIZES)
def test_levels_bytes_and_decode_equal_the_oracle(gpu, arenas, d, wire, s):
    a = arenas[d]
    x, _ = _source(a, "fp32", gpu)
    L = 2 ** s
    lv, want_bn = _levels_of(a, s)
    skip = _nan_elems(a)
    qh, bn, kept = _encode(a, x, wire, s, gpu, seed=SEED, offset=OFF)
    assert kept
    _same_norm_bits(bn, want_bn, wire)
    _payload_is(a, wire, s, qh, lv, skip)
    # the kernel's decode of its own payload: the oracle's decode of the oracle's levels
    q = torch.from_numpy(qh).to(gpu)
    ybuf, y = _banded(a.A, FCANARY, torch.float32, gpu)
    if wire == "packed":
        a.plan.qsgd_decode_bucketed_packed(q, L, d, bn, y_out=y)
    else:
        a.plan.qsgd_decode_bucketed(q, codec.storage_width(L), L, d, bn, y_out=y)
    got = y.cpu().numpy()
    assert _guards_kept(ybuf) and (got[~a.mask] == F32(FCANARY)).all()
    for o, n, b in zip(a.offs, a.sizes, a.boff):
        with np.errstate(invalid="ignore"):
            dec = oracle.decode_bucketed(lv[o:o + n], want_bn[b:b + -(-n // d)], L, d).numpy()
        g, nan = got[o:o + n], np.isnan(dec) | skip[o:o + n]  # inf 0 = NaN in the inf bucket; the NaN bucket
        assert np.isnan(g[nan]).all()
        assert np.array_equal(g.view(np.int32)[~nan], dec.view(np.int32)[~nan])


# ---------------------------------------------------------------- isolation

@pytest.mark.parametrize("d", SIZES)
def test_neighbours_of_zero_underflow_inf_and_nan_buckets_are_their_own(gpu, arenas, d):
    """Each bucket beside one of those, encoded alone in a one-tensor plan with its own draws: the same norm bits
    and the same levels as in the arena."""
    a = arenas[d]
    x, _ = _source(a, "fp32", gpu)
    u = torch.rand(a.A, device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    q, bn = a.plan.qsgd_encode_bucketed(x, 4, d, u=u)
    p, pbn = a.plan.qsgd_encode_bucketed_packed(x, 4, d, u=u)
    solo = codec.Plan([d], device=gpu)
    b = 6
    for t, j in inp.NEIGHBOURS:
        o = a.offs[t] + j * d
        xs, us = x[o:o + d].clone(), u[o:o + d].clone()
        q1, bn1 = solo.qsgd_encode_bucketed(xs, 4, d, u=us)
        p1, pbn1 = solo.qsgd_encode_bucketed_packed(xs, 4, d, u=us)
        at = a.boff[t] + j
        for alone, arena in ((bn1, bn), (pbn1, pbn)):
            assert torch.equal(alone.view(torch.int32), arena[at:at + 1].view(torch.int32)), (t, j)
        assert torch.equal(q1[:d], q[o:o + d]), (t, j)
        assert torch.equal(p1[:d * b // 32], p[o * b // 32:(o + d) * b // 32]), (t, j)
        if (t, j) != (inp.SPECIAL_T, inp.S_INF):
            assert bool(torch.isfinite(bn1).all())
        if (t, j) not in ((inp.SPECIAL_T, inp.S_INF), (inp.SPECIAL_T, inp.S_UNDERFLOW)):
            assert bool(q1[:d].any()), (t, j)


# ---------------------------------------------------------------- client counts (the exact-N instances)

KS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)
MODES = ((False, None), (True, 7.0), (True, None), (False, 7.0))  # (init, divisor)
D_K = 128


def _sum_is_sequential(gpu, a, K, width, L, init, divisor):
    msgs = _messages(a, D_K, L, K)
    qs, bns = _upload(a, msgs, width, L, gpu)
    ybuf, y = _banded(a.A, FCANARY, torch.float32, gpu)
    y.copy_(torch.from_numpy(a.start))
    if width == 0:
        a.plan.qsgd_decode_sum_bucketed_packed(qs, L, D_K, bns, y_out=y, init=init, divisor=divisor)
    else:
        a.plan.qsgd_decode_sum_bucketed(qs, width, L, D_K, bns, y_out=y, init=init, divisor=divisor)
    s = _sequential_sum(a, msgs, D_K, L, a.start if init else None)
    if divisor is not None:
        s = (s / F32(divisor)).astype(F32)
    want = np.where(a.mask, s, F32(FCANARY) if init else F32(0.0))  # init: padding kept; else written (+0 / divisor)
    assert np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32))
    assert _guards_kept(ybuf)
    if init:  # the -0.0 of the start arena survives exactly where every client's term is -0
        neg = np.signbit(want) & (want == 0) & a.mask
        assert neg.any() or K > 5  # ~600 such elements, each -0 with probability 2^-K


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("width,L", ((8, 100), (32, 256)))
def test_decode_sum_at_every_client_count(gpu, arenas, width, L, K):
    init, divisor = MODES[(K + width // 32) % 4]
    _sum_is_sequential(gpu, arenas[D_K], K, width, L, init, divisor)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("L", (16, 256))  # b = 6 and b = 10
def test_packed_decode_sum_at_every_client_count(gpu, arenas, L, K):
    init, divisor = MODES[(K + 2 + (L > 16)) % 4]
    _sum_is_sequential(gpu, arenas[D_K], K, 0, L, init, divisor)


OUTS = ((4, False), (8, False), (4, True), (8, True), (12, True))  # (s_out, packed)
PS_N = [(width, L, N) for width, L, top in ((8, 16, 9), (0, 16, 9), (32, 256, 5), (0, 256, 5)) for N in range(top + 1)]


def _ps_levels_check(a, d_out, s_out, packed, want_avg, qh, bn_h):
    lv, _ = _oracle_levels(a, want_avg, s_out, d=d_out, bnorm=bn_h)
    wire = "packed" if packed else ("int8" if s_out < 7 else "int32")
    _payload_is(a, wire, s_out, qh, lv, np.zeros(a.A, dtype=bool))


@pytest.mark.parametrize("width,L,N", PS_N)
def test_ps_step_at_every_client_count(gpu, arenas, width, L, N):
    """N = 0 .. one past the most clients of one launch (8 on int8 and packed b <= 8 input, 4 on int32 and packed
    b > 8), so every exact-N instance and the chained path run."""
    a = arenas[D_K]
    i = N + (width == 32) + 2 * (width == 0)
    start = N == 0 or i % 3 != 1
    divisor = None if i % 4 == 2 else 7.0
    s_out, packed = OUTS[i % 5]
    want_avg, qh, bn_h = _ps_check(gpu, a, a.start, D_K, D_K, width, L, N, start, divisor, s_out, packed)
    _ps_levels_check(a, D_K, s_out, packed, want_avg, qh, bn_h)


# ---------------------------------------------------------------- the PS step across bucket sizes

@pytest.mark.parametrize("packed", (False, True))
@pytest.mark.parametrize("d_in,d_out", ((2048, 128), (128, 2048), (512, 64), (4096, 512)))
def test_ps_step_across_bucket_sizes(gpu, arenas, d_in, d_out, packed):
    a = arenas[d_out]
    width, N, s_out = (0, 3, 8) if packed else (8, 2, 4)
    want_avg, qh, bn_h = _ps_check(gpu, a, a.start, d_in, d_out, width, 16, N, True, 7.0, s_out, packed)
    _ps_levels_check(a, d_out, s_out, packed, want_avg, qh, bn_h)
