"""The bucketed-QSGD oracle (oracle/qsgd_bucket.py) and the inputs of its GPU matrix (tests/golden/qsgd_bucket_inputs.py),
checked without a GPU: the fma helper against exact rational arithmetic, the norms against float64, the special
buckets' promises, and that the inputs make a bit-exact norm comparison see a change of summation order."""

from fractions import Fraction

import numpy as np
import pytest
import torch

import oracle
import qsgd_bucket_inputs as inp
from oracle import qsgd_bucket as ob

SIZES = tuple(1 << l for l in range(6, 13))  # omnifed_amd.codec.BUCKET_SIZES (checked below)
F32 = np.float32


def test_sizes_and_layouts_are_the_codecs():
    from omnifed_amd import codec
    assert SIZES == codec.BUCKET_SIZES
    for d in SIZES:
        sz = inp.sizes(d)
        assert inp.arena_layout(sz) == codec.arena_layout(sz)
        assert inp.bucket_layout(sz, d) == codec.bucket_layout(sz, d)
        assert [t.size for t in inp.tensors(d)] == sz and all(t.dtype == F32 for t in inp.tensors(d))


def _fl32(fr):
    """A Fraction rounded to the nearest fp32, ties to even, subnormals included (finite results only)."""
    if fr == 0:
        return F32(0.0)
    sign, a = (-1 if fr < 0 else 1), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = max(e, -126) - 23  # the exponent of one ulp
    m = a / Fraction(2) ** q
    r = m.numerator // m.denominator
    rem = m - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and r & 1):
        r += 1
    return F32(sign * float(Fraction(r) * Fraction(2) ** q))  # r < 2^25: exact in float64, and in fp32 after rounding


def _fma_cases():
    rng = np.random.default_rng(11)
    a = np.concatenate([rng.standard_normal(1500) * 10.0 ** rng.uniform(-22, 3, 1500), [0.0, -0.0, 1.0, 1e-20, 3e-23]])
    a = a.astype(F32)
    c = (np.abs(rng.standard_normal(a.size)) * 10.0 ** rng.uniform(-44, 6, a.size)).astype(F32)
    c[::5] = (a[::5].astype(np.float64) ** 2 * rng.uniform(0.5, 4.0, a[::5].size)).astype(F32)  # of the square's size
    c[::11] = -c[::11]
    # halfway cases: a = 1 + k 2^-12 has a^2 = 1 + k 2^-11 + k^2 2^-24, whose last bit is half an fp32 ulp for odd k
    # (|k| < 2^11 keeps a^2 in [1, 2)); c = 0 and c = 2^-23 steer the tie, c = +-2^-40 breaks it either way, and a
    # float64 sum rounded to nearest first would lose that
    k = np.arange(1, 1400, 2, dtype=np.float64)
    ha = (1.0 + k * 2.0 ** -12).astype(F32)
    hc = np.tile(np.array([0.0, 2.0 ** -23, 2.0 ** -40, -2.0 ** -40, 2.0 ** -60, -2.0 ** -60], dtype=F32), ha.size // 6 + 1)[:ha.size]
    # subnormal results: squares and sums below 2^-126
    sa = (rng.uniform(1.0, 8.0, 700) * 1e-21).astype(F32)
    sc = (rng.uniform(0.0, 4.0, 700) * 1e-41).astype(F32)
    return np.concatenate([a, ha, sa]), np.concatenate([c, hc, sc])


def test_fma_helper_equals_exact_rational_arithmetic():
    a, c = _fma_cases()
    assert a.size >= 2500
    got = ob.fma_sq(a, c)
    want = np.array([_fl32(Fraction(float(x)) * Fraction(float(x)) + Fraction(float(y))) for x, y in zip(a, c)], dtype=F32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # the cases do include ones a float64 sum rounded to nearest and then to fp32 gets wrong
    naive = (a.astype(np.float64) ** 2 + c.astype(np.float64)).astype(F32)
    assert int((naive.view(np.int32) != want.view(np.int32)).sum()) >= 50
    # inf and NaN pass through
    assert np.isinf(ob.fma_sq(np.array([3e19], dtype=F32), np.array([0.0], dtype=F32)))[0]
    assert np.isnan(ob.fma_sq(np.array([np.nan, 1.0], dtype=F32), np.array([0.0, np.nan], dtype=F32))).all()
    assert np.isinf(ob.fma_sq(np.array([1.0], dtype=F32), np.array([np.inf], dtype=F32)))[0]


def test_the_written_order_on_a_bucket_written_out():
    """d = 64 by hand: 16 quads, the tree ((((q0 + q1) + (q2 + q3)) + ...): lane ^ 1, 2, 4, 8."""
    v = inp.make_tensor(64, inp.MANY_T)[:64]
    f = lambda a, c: ob.fma_sq(np.array([a], dtype=F32), np.array([c], dtype=F32))[0]
    q = [f(v[4 * i + 3], f(v[4 * i + 2], f(v[4 * i + 1], f(v[4 * i], F32(0.0))))) for i in range(16)]
    for o in (1, 2, 4, 8):
        q = [F32(q[l] + q[l ^ o]) for l in range(16)]  # the butterfly as the kernel runs it
    assert len({x.tobytes() for x in q}) == 1
    assert oracle.bucket_norms(v, 64)[0].tobytes() == np.sqrt(q[0]).astype(F32).tobytes()
    # absent elements count as +0, and a bucket's norm does not depend on what follows it
    whole = inp.make_tensor(64, inp.MANY_T)
    assert oracle.bucket_norms(v[:61], 64).tobytes() == oracle.bucket_norms(np.concatenate([v[:61], np.zeros(3, F32)]), 64).tobytes()
    assert oracle.bucket_norms(whole, 64)[0].tobytes() == oracle.bucket_norms(v, 64)[0].tobytes()


def test_rows_before_lanes_on_a_bucket_written_out():
    """d = 4096 by hand: quad 256 r + lane; rows (r0 + r1) + (r2 + r3) of one lane, then lanes, then waves."""
    v = inp.make_tensor(4096, inp.MANY_T)[:4096]
    qs = ob.quad_sums(v, 4096)[0]
    lane = [F32(F32(qs[l] + qs[256 + l]) + F32(qs[512 + l] + qs[768 + l])) for l in range(256)]
    for o in (1, 2, 4, 8, 16, 32):
        lane = [F32(lane[l] + lane[l ^ o]) for l in range(256)]
    total = F32(F32(lane[0] + lane[64]) + F32(lane[128] + lane[192]))
    assert oracle.bucket_norms(v, 4096)[0].tobytes() == np.sqrt(total).astype(F32).tobytes()
    v2 = v[:2048]
    qs = ob.quad_sums(v2, 2048)[0]
    lane = [F32(qs[l] + qs[256 + l]) for l in range(256)]
    for o in (1, 2, 4, 8, 16, 32):
        lane = [F32(lane[l] + lane[l ^ o]) for l in range(256)]
    total = F32(F32(lane[0] + lane[64]) + F32(lane[128] + lane[192]))
    assert oracle.bucket_norms(v2, 2048)[0].tobytes() == np.sqrt(total).astype(F32).tobytes()


@pytest.mark.parametrize("d", SIZES)
def test_special_buckets_keep_their_promises(d):
    x = inp.make_tensor(d, inp.SPECIAL_T)
    bn = oracle.bucket_norms(x, d)
    b = lambda j: x[j * d:(j + 1) * d]
    assert bn.dtype == F32 and bn.size == 8
    assert bn[inp.S_ZERO] == 0 and bn[inp.S_ZERO].tobytes() == F32(0.0).tobytes() and np.signbit(b(inp.S_ZERO)).any()
    assert bn[inp.S_ONE] == F32(abs(inp.ONE_VALUE))
    sq = b(inp.S_SUBNORMAL).astype(np.float64) ** 2
    assert (sq >= 2.0 ** -149).all() and (sq < 2.0 ** -126).all() and bn[inp.S_SUBNORMAL] > 0
    assert (b(inp.S_UNDERFLOW) != 0).all() and bn[inp.S_UNDERFLOW] == 0
    assert np.isfinite(b(inp.S_INF)).all() and np.isposinf(bn[inp.S_INF])
    # levels: +-L exactly for the lone element, zeros under the zero norms, finite under the inf norm
    u = np.random.default_rng(3).random(x.size).astype(F32)
    for s in (4, 8, 12):
        q, bn2 = oracle.encode_bucketed(x, 1.0, s, d, u)
        assert bn2.tobytes() == bn.tobytes()
        q = q.numpy().reshape(8, d)
        assert q[inp.S_ONE, inp.ONE_AT] == -2 ** s and np.count_nonzero(q[inp.S_ONE]) == 1
        assert not q[inp.S_ZERO].any() and not q[inp.S_UNDERFLOW].any()
        assert not q[inp.S_INF].any()  # v / inf = 0: the oracle has levels for the inf bucket, the GPU test holds them
        assert (np.abs(q) <= 2 ** s).all() and q[0].any() and q[inp.S_SUBNORMAL].any()
    # the neighbours of the inf and NaN buckets: finite, and the norm of the bucket alone
    y = inp.make_tensor(d, inp.NAN_T)
    bny = oracle.bucket_norms(y, d)
    assert np.isnan(bny[1]) and int(np.isnan(y).sum()) == 1
    for t, j in inp.NEIGHBOURS:
        src, norms = (x, bn) if t == inp.SPECIAL_T else (y, bny)
        alone = oracle.bucket_norms(src[j * d:(j + 1) * d].copy(), d)
        assert alone.size == 1 and alone.tobytes() == norms[j].tobytes()
        assert np.isfinite(norms[j]) or (t, j) == (inp.SPECIAL_T, inp.S_INF)


@pytest.mark.parametrize("alpha", (1.0, 3.0))
@pytest.mark.parametrize("d", SIZES)
def test_norms_stay_within_the_derived_bound_of_float64(d, alpha):
    """Any fp32 summation order of d non-negative squares has relative error <= d 2^-24, the square root halves it
    and rounds once more: (d + 4) 2^-25 (the bound of tests/test_gpu_qsgd_bucketed.py)."""
    worst = 0.0
    for x in inp.tensors(d):
        v = (x * F32(alpha)).astype(F32)
        bn = oracle.bucket_norms(v, d)
        nb = bn.size
        pad = np.zeros(nb * d)
        pad[:v.size] = v.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            exact = np.sqrt((pad.reshape(nb, d) ** 2).sum(axis=1))
        ok = np.isfinite(bn) & (bn != 0)
        assert (np.abs(bn[ok] - exact[ok]) <= (d + 4) * 2.0 ** -25 * exact[ok]).all()
        worst = max(worst, float((np.abs(bn[ok] - exact[ok]) / exact[ok]).max()))
    print(f"d={d} alpha={alpha}: worst relative error {worst:.3g}, bound {(d + 4) * 2.0 ** -25:.3g}")


def _sequential(v, d):
    """Step 1 kept, steps 2-4 replaced by a sequential fp32 sum of the quad sums in element order (the narrower
    change: a sequential sum of the squares themselves moves more buckets still)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(np.cumsum(ob.quad_sums(v, d), axis=1, dtype=F32)[:, -1])


def _lanes_before_rows(v, d):
    """Steps 3-4 on every row, then the rows' sums added r ^ 1, r ^ 2."""
    s = ob.quad_sums(v, d)
    rows = ob.pair_tree(s.reshape(s.shape[0], d // 1024, 256))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(ob.pair_tree(rows))


def order_sensitivity(d):
    """(buckets, changed by a sequential sum, changed by lanes before rows or None) over the recipe's buckets."""
    n = seq = lbr = 0
    for x in inp.tensors(d):
        bn = oracle.bucket_norms(x, d).view(np.int32)
        n += bn.size
        seq += int((bn != _sequential(x, d).view(np.int32)).sum())
        if d > 1024:
            lbr += int((bn != _lanes_before_rows(x, d).view(np.int32)).sum())
    return n, seq, (lbr if d > 1024 else None)


@pytest.mark.parametrize("d", SIZES)
def test_a_bit_exact_norm_check_sees_an_order_change(d):
    """A condition on the inputs: another summation order moves the norm bits of at least 4 of the recipe's buckets."""
    n, seq, lbr = order_sensitivity(d)
    print(f"d={d}: {n} buckets, sequential sum changes {seq}, lanes before rows changes {lbr}")
    assert seq >= 4
    assert lbr is None or lbr >= 4


def test_encode_and_decode_loops_are_the_per_tensor_oracle_per_bucket():
    d, s = 128, 4
    x = torch.from_numpy(inp.make_tensor(d, 7))  # 2 d + 5 elements
    u = torch.from_numpy(np.random.default_rng(5).random(x.numel()).astype(F32))
    q, bn = oracle.encode_bucketed(x, 3.0, s, d, u)
    v = x * torch.tensor(3.0)
    assert bn.size == 3 and q.dtype == torch.int64
    for j in range(3):
        want, *_ = oracle.qsgd_quantize(v[j * d:(j + 1) * d], s, norm=float(bn[j]), u=u[j * d:(j + 1) * d])
        assert torch.equal(q[j * d:(j + 1) * d], want.long())
    y = oracle.decode_bucketed(q, bn, 16, d)
    assert y.dtype == torch.float32 and float((y - v).abs().max()) <= float(bn.max()) / 16
    # the caller's norms replace the computed ones
    q2, bn2 = oracle.encode_bucketed(x, 3.0, s, d, u, bnorm=bn * F32(1.25))
    assert bn2.tobytes() == (bn * F32(1.25)).tobytes() and not torch.equal(q, q2)
    with pytest.raises(ValueError):
        oracle.bucket_norms(x.numpy(), 96)
