"""Max-scaled bucketed QSGD and its Hadamard rotation (csrc/omf_qsgd_bucket_rot.hip) against float64 numpy.

Per bucket size d the plan holds tensors of (d, d + 1, 2d - 1, 5, 4096 + d, 3 * 4096 + 7) elements: full buckets, short
tails, a tensor below one bucket, a workgroup boundary inside a tensor, several blocks.  Inputs are seeded N(0, 1) with
a few elements x 100 and one all-zero bucket.  The transform's bound is the standard one for logd levels of fp32 adds:
gamma sum |v_j| per element, gamma = logd u / (1 - logd u), u = 2^-24 (addition has no underflow error).
"""

import numpy as np
import pytest
import torch

from omnifed_amd import codec

pytestmark = pytest.mark.gpu

DS = [64, 128, 256, 512, 1024, 2048, 4096]
RS = 20171  # rotation seed


def _wht(rows):
    """H_d of every row, float64."""
    r, n, h = rows.astype(np.float64), rows.shape[1], 1
    while h < n:
        r = r.reshape(-1, n // (2 * h), 2, h)
        r = np.stack([r[:, :, 0] + r[:, :, 1], r[:, :, 0] - r[:, :, 1]], 2)
        h *= 2
    return r.reshape(-1, n)


class Case:
    def __init__(self, gpu, d):
        self.d, self.gpu = d, gpu
        self.sizes = [d, d + 1, 2 * d - 1, 5, 4096 + d, 3 * 4096 + 7]
        self.plan = p = codec.Plan(self.sizes, device=gpu)
        self.gamma = (d.bit_length() - 1) * 2.0 ** -24 / (1 - (d.bit_length() - 1) * 2.0 ** -24)
        boff, self.nb = p.bucket_layout(d)
        rng = np.random.default_rng(d)
        self.x = np.zeros(p.arena_end, np.float32)
        self.bidx = np.full(p.arena_end, -1, np.int64)  # the element's bucket; -1: padding
        self.sig = np.ones(p.arena_end)
        full = np.zeros(self.nb, bool)
        for t, (o, n) in enumerate(zip(p.offsets, self.sizes)):
            self.x[o:o + n] = rng.standard_normal(n)
            self.bidx[o:o + n] = boff[t] + np.arange(n) // d
            self.sig[o:o + n] = codec.rotation_signs(RS, t, 0, n).numpy()
            full[boff[t]:boff[t] + n // d] = True
        self.live = self.bidx >= 0
        self.x[rng.choice(np.flatnonzero(self.live), 6, replace=False)] *= 100
        self.x[p.offsets[4]:p.offsets[4] + d] = 0  # an all-zero bucket
        self.rot = self.live & full[self.bidx]  # elements of full buckets
        self.xg = torch.from_numpy(self.x).to(gpu)

    def rows(self, a):
        """The full buckets of arena ``a`` as rows, in arena order."""
        return a[self.rot].reshape(-1, self.d)

    def forward(self, v):
        """float64 H_d (sigma . v) on full buckets, v elsewhere; and the bound per element (0 off full buckets)."""
        z, bound = v.astype(np.float64), np.zeros(v.shape)
        z[self.rot] = _wht(self.rows(v * self.sig)).ravel()
        bound[self.rot] = np.repeat(self.gamma * np.abs(self.rows(v)).astype(np.float64).sum(1), self.d)
        return z, bound

    def inverse(self, s):
        x, bound = s.astype(np.float64), np.zeros(s.shape)
        x[self.rot] = _wht(self.rows(s)).ravel() / self.d * self.sig[self.rot]
        bound[self.rot] = np.repeat(self.gamma * np.abs(self.rows(s)).astype(np.float64).sum(1), self.d) / self.d
        return x, bound

    def bucket_max(self, z):
        m = np.zeros(self.nb, np.float32)
        np.maximum.at(m, self.bidx[self.live], np.abs(z[self.live]))
        return m


@pytest.fixture(scope="module")
def case(gpu):
    made = {}
    return lambda d: made[d] if d in made else made.setdefault(d, Case(gpu, d))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("d", DS)
def test_transform_against_float64(case, d):
    c = case(d)
    z = c.plan.qsgd_rotate_bucketed(c.xg, d, RS)
    zh = z.cpu().numpy()
    want, bound = c.forward(c.x)
    err = np.abs(zh - want)
    print(f"d={d}: worst error / bound {np.max(err[c.rot] / np.maximum(bound[c.rot], 1e-300)):.3f}")
    assert np.all(err[c.rot] <= bound[c.rot])
    tail = c.live & ~c.rot
    assert tail.any() and np.array_equal(_bits(zh[tail]), _bits(c.x[tail]))  # short last buckets: copies
    back = c.plan.qsgd_rotate_bucketed(z, d, RS, inverse=True).cpu().numpy()
    assert np.all(np.abs(back - c.x.astype(np.float64))[c.rot] <= 2 * bound[c.rot])
    assert np.array_equal(_bits(back[tail]), _bits(c.x[tail]))


@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("d", DS)
def test_scale_bits_and_levels(case, d, rot, s):
    """The scale arena is max |z| per bucket, exactly, and the payload is the existing bucketed encoder's on the z
    arena with those scales and the same draws."""
    c, alpha = case(d), 0.75
    v = c.xg * alpha  # fl32(alpha x)
    z = c.plan.qsgd_rotate_bucketed(v, d, RS) if rot else v
    q, m = c.plan.qsgd_encode_bucketed_max(c.xg, s, d, rotate=rot, rotation_seed=RS, alpha=alpha, seed=7, offset=3)
    assert c.plan.last_encoder == ("bucketed_max_rot" if rot else "bucketed_max")
    want = c.bucket_max(z.cpu().numpy())
    assert np.array_equal(_bits(m.cpu().numpy()), _bits(want))
    assert want[c.bidx[c.plan.offsets[4]]] == 0  # the all-zero bucket
    assert torch.equal(c.plan.qsgd_scales_bucketed_max(c.xg, d, rotate=rot, rotation_seed=RS, alpha=alpha), m)
    q_ref, _ = c.plan.qsgd_encode_bucketed(z, s, d, seed=7, offset=3, bnorm_in=m)
    live = torch.from_numpy(c.live).to(c.gpu)
    assert q.dtype == (torch.int8 if s == 4 else torch.int32)
    assert torch.equal(q[:c.plan.arena_end][live], q_ref[:c.plan.arena_end][live])
    assert int(q[:c.plan.arena_end][live].abs().max()) == 2 ** s  # the max element sits on the top level


def _clients(c, K, s):
    """K clients' rotated payloads and scales, and the fp32 client-order sum of fl32(fl32(m q) / L)."""
    L, qs, ms = np.float32(2 ** s), [], []
    total = np.zeros(c.plan.arena_end, np.float32)
    for k in range(K):
        q, m = c.plan.qsgd_encode_bucketed_max(c.xg * (1 + 0.25 * k), s, c.d, rotate=True, rotation_seed=RS, seed=k)
        qs.append(q), ms.append(m)
        mq = m.cpu().numpy()[c.bidx[c.live]] * q.cpu().numpy()[:c.plan.arena_end][c.live].astype(np.float32)
        total[c.live] = total[c.live] + mq / L
    return qs, ms, total


@pytest.mark.parametrize("d", [64, 1024, 4096])
def test_decode_sum_of_nine_onto_y(case, d):
    """init with more than 8 clients: each group of 8 is inverted and added to y in turn, then the divisor — the bytes
    of the two calls it chains."""
    c, p = case(d), case(d).plan
    qs, ms, _ = _clients(c, 9, 4)
    y0 = torch.from_numpy(np.random.default_rng(9).standard_normal(p.arena_end).astype(np.float32)).to(c.gpu)
    got = p.qsgd_decode_sum_bucketed_rot(qs, 8, 16, d, RS, ms, y_out=y0.clone(), init=True, divisor=9.0)
    want = p.qsgd_decode_sum_bucketed_rot(qs[:8], 8, 16, d, RS, ms[:8], y_out=y0.clone(), init=True)
    p.qsgd_decode_sum_bucketed_rot(qs[8:], 8, 16, d, RS, ms[8:], y_out=want, init=True, divisor=9.0)
    assert torch.equal(got, want)
    # and without y: the running sum crosses the launches in the rotated domain, then one inverse and the divisor
    plain = p.qsgd_decode_sum_bucketed_rot(qs, 8, 16, d, RS, ms).cpu().numpy()
    div = p.qsgd_decode_sum_bucketed_rot(qs, 8, 16, d, RS, ms, divisor=9.0).cpu().numpy()
    assert np.array_equal(_bits(div), _bits(plain / np.float32(9)))


@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("d", DS)
def test_decode_sum(case, d, s, K):
    c = case(d)
    p, width, L = c.plan, 8 if s == 4 else 32, 2 ** s
    qs, ms, total = _clients(c, K, s)
    y = torch.full((p.arena_end,), 7.0, device=c.gpu)
    p.qsgd_decode_sum_bucketed_rot(qs, width, L, d, RS, ms, y_out=y)
    yh = y.cpu().numpy()
    want, bound = c.inverse(total)
    err = np.abs(yh - want)
    print(f"d={d} s={s} K={K}: worst error / bound {np.max(err[c.rot] / np.maximum(bound[c.rot], 1e-300)):.3f}")
    assert np.all(err[c.live] <= bound[c.live])  # exact on the unrotated tails
    assert np.all(yh[~c.live] == 0)  # the padding is filled
    if K == 1:
        assert torch.equal(p.qsgd_decode_bucketed_rot(qs[0], width, L, d, RS, ms[0])[torch.from_numpy(c.live).to(c.gpu)],
                           y[torch.from_numpy(c.live).to(c.gpu)])
    # init and divisor, as qsgd_decode_sum_bucketed: fl32(fl32(y0 + xh) / divisor), padding untouched
    y0 = torch.from_numpy(np.random.default_rng(K).standard_normal(p.arena_end).astype(np.float32)).to(c.gpu)
    y1 = p.qsgd_decode_sum_bucketed_rot(qs[:3], width, L, d, RS, ms[:3], y_out=y0.clone(), init=True, divisor=3.0)
    xh = p.qsgd_decode_sum_bucketed_rot(qs[:3], width, L, d, RS, ms[:3])
    y0, y1, xh = y0.cpu().numpy(), y1.cpu().numpy(), xh.cpu().numpy()
    assert np.array_equal(_bits(y1[c.live]), _bits(((y0 + xh) / np.float32(3))[c.live]))
    assert np.array_equal(_bits(y1[~c.live]), _bits(y0[~c.live]))


def _wire(c, s, rot):
    from omnifed_amd.hybrid.communicator.global_grpc_compression import build_global_compressor
    return build_global_compressor(enabled=True, scheme="qsgd", bit_width=s, device=c.gpu, bucket_size=c.d,
                                   bucket_norm="max", rotate=rot, rotation_seed=RS)


def _updates(c, scale=1.0):
    return {f"t{t}": c.xg[o:o + n] * scale for t, (o, n) in enumerate(zip(c.plan.offsets, c.sizes))}


def _round_trip_ok(c, ups, layers, got, s, rot):
    """Per layer: the type and param_shape, and x^ against x.  Stochastic rounding moves a coordinate of z less than
    one step m / L (+ 4 u m for the division's and the decode's roundings).  Unrotated, that is the bound per
    element.  Rotated, H / sqrt(d) is orthogonal, so a full bucket's ||x^ - x||_2 <= ||z^ - z||_2 / sqrt(d) <= that
    step, plus the transform's slack: gamma sum |x_j| forward (per coordinate of z) and gamma sum |z^_j| / d <=
    gamma m (1 + 1 / L) per element back, i.e. gamma (sum |x_j| + 2 sqrt(d) m) on the norm."""
    d, u = c.d, 2.0 ** -24
    for name, L in zip(ups, layers):
        x = ups[name].cpu().numpy().astype(np.float64)
        m = np.frombuffer(L.meta_tensor, np.float32).astype(np.float64)
        assert L.compression_type == ("QSGDRotatedBucketedCompression" if rot else "QSGDBucketedCompression")
        assert list(L.param_shape) == ([d, RS] if rot else [d]) and len(m) == -(-len(x) // d)
        err = got[name].cpu().numpy().astype(np.float64) - x
        step = m * (2.0 ** -s + 4 * u)
        nfull = len(x) // d if rot else 0
        rows = np.abs(x[:nfull * d]).reshape(nfull, d)
        slack = c.gamma * (rows.sum(1) + 2 * np.sqrt(d) * m[:nfull])
        assert np.all(np.linalg.norm(err[:nfull * d].reshape(nfull, d), axis=1) <= step[:nfull] + slack)
        assert np.all(np.abs(err[nfull * d:]) <= np.repeat(step[nfull:], d)[:len(x) - nfull * d])


@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("d", DS)
def test_public_path(case, d, rot, s):
    """encode_updates_dict -> decode_updates_dict with bucket_norm="max", both rotations; max-only layers are ordinary
    bucketed ones and decode through the unchanged bucketed decoder; a single layer decodes alone to the same bits."""
    from omnifed_amd.hybrid.communicator.global_grpc_compression import (decode_layer_tensor, decode_updates_dict,
                                                                          encode_updates_dict)
    c = case(d)
    ups = _updates(c)
    layers = encode_updates_dict(ups, _wire(c, s, rot))
    got = decode_updates_dict(layers, device=c.gpu)
    _round_trip_ok(c, ups, layers, got, s, rot)
    assert torch.equal(decode_layer_tensor(layers[4], device=c.gpu), got["t4"])


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("d", [64, 512, 4096])
def test_aggregator_round(case, d, rot):
    """Three clients' max-scaled updates through DeviceAggregator: accumulate_layers one by one and accumulate_many in
    one run both hold sum_k decode(update k) — within the fp32 sums' and the transforms' bound of the float64 sum of
    the single decodes — and apply_and_encode's downlink is the average through the same encoder."""
    from omnifed_amd.hybrid.communicator.global_grpc_compression import decode_updates_dict, encode_updates_dict
    from omnifed_amd.ps import DeviceAggregator
    c, s, K = case(d), 4, 3
    comp = _wire(c, s, rot)
    msgs = [encode_updates_dict(_updates(c, 1 + 0.25 * k), comp) for k in range(K)]
    singles = [decode_updates_dict(m, device=c.gpu) for m in msgs]
    shapes = [(f"t{t}", (n,)) for t, n in enumerate(c.sizes)]
    one, many = DeviceAggregator(shapes, device=c.gpu), DeviceAggregator(shapes, device=c.gpu)
    for m in msgs:
        one.accumulate_layers(m, 1)
    many.accumulate_many([(m, 1) for m in msgs])
    u = 2.0 ** -24
    for t, (name, _) in enumerate(shapes):
        terms = np.stack([sg[name].cpu().numpy().astype(np.float64) for sg in singles])
        # per client the inverse errs by at most gamma sum |z^_j| / d <= gamma max |z^|; the sums add (K - 1) u each
        mz = sum(np.frombuffer(m[t].meta_tensor, np.float32).astype(np.float64).max() * (1 + 2.0 ** -s) for m in msgs)
        bound = (K - 1) * u * np.abs(terms).sum(0) + (2 * c.gamma + K * u) * mz
        for agg in (one, many):
            assert np.all(np.abs(agg._slice(name).cpu().numpy() - terms.sum(0)) <= bound)
    avg, down = many.apply_and_encode(comp)
    assert many.plan.last_encoder == ("bucketed_max_rot" if rot else "bucketed_max")  # divide, then the max encoder
    _round_trip_ok(c, avg, down, decode_updates_dict(down, device=c.gpu), s, rot)
