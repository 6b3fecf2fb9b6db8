"""The max-scaled bucketed PS step (omf_ps_sum_encode_bucketed_max, csrc/omf_qsgd_bucket_ps_max.hip): its bytes against
the three calls it replaces, its average against float64, the rotated-domain downlink against a numpy sum, and the
aggregator's routing.  The plan is the rotation tests' (tests/test_gpu_qsgd_bucket_rot.py): per bucket size d tensors
of (d, d + 1, 2d - 1, 5, 4096 + d, 3 * 4096 + 7) elements, seeded N(0, 1) with a few elements x 100 and one all-zero
bucket; d = 64 (DPP only), 256 (the last size without LDS), 512 (the LDS tile), 4096 (own rows)."""

import numpy as np
import pytest
import torch

from omnifed_amd import codec

pytestmark = pytest.mark.gpu

DS = [64, 256, 512, 4096]
RS, DIV, SEED, OFF = 20171, 7.0, 11, 5


class Case:
    def __init__(self, gpu, d):
        self.d, self.gpu = d, gpu
        self.sizes = [d, d + 1, 2 * d - 1, 5, 4096 + d, 3 * 4096 + 7]
        self.plan = p = codec.Plan(self.sizes, device=gpu)
        boff, self.nb = p.bucket_layout(d)
        rng = np.random.default_rng(d)
        x = np.zeros(p.arena_end, np.float32)
        self.bidx = np.full(p.arena_end, -1, np.int64)  # the element's bucket; -1: padding
        for t, (o, n) in enumerate(zip(p.offsets, self.sizes)):
            x[o:o + n] = rng.standard_normal(n)
            self.bidx[o:o + n] = boff[t] + np.arange(n) // d
        self.live_h = self.bidx >= 0
        x[rng.choice(np.flatnonzero(self.live_h), 6, replace=False)] *= 100
        x[p.offsets[4]:p.offsets[4] + d] = 0  # an all-zero bucket
        self.xg = torch.from_numpy(x).to(gpu)
        self.live = torch.from_numpy(self.live_h).to(gpu)
        self.acc = torch.from_numpy(rng.standard_normal(p.arena_end).astype(np.float32)).to(gpu)
        self.made = {}

    def clients(self, rot, s, K):
        """K clients' payloads and scales of scaled copies of x."""
        for k in range(K):
            if (rot, s, k) not in self.made:
                self.made[rot, s, k] = self.plan.qsgd_encode_bucketed_max(self.xg * (1 + 0.25 * k), s, self.d, rotate=rot,
                                                                          rotation_seed=RS, seed=k)
        return [self.made[rot, s, k][0] for k in range(K)], [self.made[rot, s, k][1] for k in range(K)]

    def decode_sum(self, rot, qs, ms, width, L, **kw):
        if rot:
            return self.plan.qsgd_decode_sum_bucketed_rot(qs, width, L, self.d, RS, ms, **kw)
        return self.plan.qsgd_decode_sum_bucketed(qs, width, L, self.d, ms, **kw)


@pytest.fixture(scope="module")
def case(gpu):
    made = {}
    return lambda d: made[d] if d in made else made.setdefault(d, Case(gpu, d))


@pytest.mark.parametrize("sum_given", [False, True])
@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("width,s,L", [(8, 4, 16), (32, 8, 256), (8, 4, 12)])  # 12: decoded by the division
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("rot", [False, True])
def test_bytes_of_the_sequence(case, rot, d, width, s, L, K, with_acc, sum_given):
    c, p = case(d), case(d).plan
    qs, ms = c.clients(rot, s, K)
    want_sum = c.decode_sum(rot, qs, ms, width, L, y_out=c.acc.clone() if with_acc else None, init=with_acc)
    want_avg = codec.div_(want_sum.clone(), DIV)
    want_q, want_m = p.qsgd_encode_bucketed_max(want_avg, s, d, rotate=rot, rotation_seed=RS, seed=SEED, offset=OFF)
    acc = c.acc.clone() if with_acc else None
    sum_out = (acc if with_acc else torch.full_like(c.acc, 7.0)) if sum_given else None
    avg, q, m = p.ps_sum_encode_bucketed_max(acc, qs, ms, width, L, d, DIV, s, rotate=rot, rotation_seed=RS, sum_out=sum_out,
                                             avg_out=torch.full_like(c.acc, 7.0), seed=SEED, offset=OFF)
    assert p.last_encoder == "bucketed_ps_max"
    assert torch.equal(avg.view(torch.int32)[c.live], want_avg.view(torch.int32)[c.live])
    assert bool((avg[~c.live] == 7.0).all())  # the poisoned padding
    if sum_given:
        assert torch.equal(sum_out.view(torch.int32)[c.live], want_sum.view(torch.int32)[c.live])
    elif with_acc:
        assert torch.equal(acc, c.acc)
    assert torch.equal(q[:p.arena_end][c.live], want_q[:p.arena_end][c.live])
    assert torch.equal(m.view(torch.int32), want_m.view(torch.int32))


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("rot", [False, True])
def test_average_against_float64(case, rot, d):
    """The bound test_aggregator_round (tests/test_gpu_qsgd_bucket_rot.py) derives for the sum — (K - 1) u sum |terms| for
    the fp32 adds, (2 gamma + K u) max |z^| per client for the inverse, gamma = logd u / (1 - logd u) — over the
    divisor, plus the division's rounding."""
    c, p, K, s, u = case(d), case(d).plan, 3, 4, 2.0 ** -24
    logd = d.bit_length() - 1
    gamma = logd * u / (1 - logd * u)
    qs, ms = c.clients(rot, s, K)
    avg, _, _ = p.ps_sum_encode_bucketed_max(None, qs, ms, 8, 16, d, DIV, s, rotate=rot, rotation_seed=RS)
    terms = np.stack([(p.qsgd_decode_bucketed_rot(q, 8, 16, d, RS, m) if rot else p.qsgd_decode_bucketed(q, 8, 16, d, m))
                      .cpu().numpy().astype(np.float64) for q, m in zip(qs, ms)])
    boff, got = p.bucket_layout(d)[0] + [c.nb], avg.cpu().numpy()
    for t, (o, n) in enumerate(zip(p.offsets, c.sizes)):
        mz = sum(float(m[boff[t]:boff[t + 1]].max()) * (1 + 2.0 ** -s) for m in ms)
        want = terms[:, o:o + n].sum(0) / DIV
        bound = ((K - 1) * u * np.abs(terms[:, o:o + n]).sum(0) + (2 * gamma + K * u) * mz) / DIV
        err = np.abs(got[o:o + n] - want)
        print(f"rot={rot} d={d} t={t}: worst error / bound {np.max(err / (bound + u * np.abs(want) + 1e-300)):.3f}")
        assert np.all(err <= bound + u * np.abs(want))


@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("d", DS)
def test_requantised_in_the_rotated_domain(case, d, K):
    """Z, the clients' sum in the rotated domain, rebuilt in numpy fp32 by the decode rule fl32(fl32(m q) / L) in client
    order; the downlink is the unrotated max encoder's on W = Z / divisor."""
    c, p, s, L = case(d), case(d).plan, 4, np.float32(16)
    qs, ms = c.clients(True, s, K)
    Z = np.zeros(p.arena_end, np.float32)
    for q, m in zip(qs, ms):
        mq = m.cpu().numpy()[c.bidx[c.live_h]] * q.cpu().numpy()[:p.arena_end][c.live_h].astype(np.float32)
        Z[c.live_h] = Z[c.live_h] + mq / L
    W = torch.from_numpy(Z / np.float32(DIV)).to(c.gpu)
    want_q, want_m = p.qsgd_encode_bucketed_max(W, s, d, rotate=False, seed=SEED, offset=OFF)
    kw = dict(rotate=True, rotation_seed=RS, requantise_rotated=True, seed=SEED, offset=OFF)
    avg, q, m = p.ps_sum_encode_bucketed_max(None, qs, ms, 8, 16, d, DIV, s, **kw)
    assert p.last_encoder == "bucketed_ps_max"
    assert torch.equal(q[:p.arena_end][c.live], want_q[:p.arena_end][c.live])
    assert torch.equal(m.view(torch.int32), want_m.view(torch.int32))
    want_avg = p.qsgd_decode_sum_bucketed_rot(qs, 8, 16, d, RS, ms, divisor=DIV)
    assert torch.equal(avg.view(torch.int32)[c.live], want_avg.view(torch.int32)[c.live])
    for bad in (dict(kw, rotate=False), dict(kw, acc=c.acc)):
        with pytest.raises(ValueError):
            p.ps_sum_encode_bucketed_max(bad.pop("acc", None), qs, ms, 8, 16, d, DIV, s, **bad)


@pytest.mark.parametrize("d", [64, 4096])
@pytest.mark.parametrize("rot", [False, True])
def test_aggregator_takes_the_step(case, rot, d):
    from omnifed_amd.hybrid.communicator.global_grpc_compression import build_global_compressor, encode_updates_dict
    from omnifed_amd.ps import DeviceAggregator
    c, s = case(d), 4

    def comp(norm="max"):
        w = build_global_compressor(enabled=True, scheme="qsgd", bit_width=s, device=c.gpu, bucket_size=d, bucket_norm=norm,
                                    rotate=rot and norm == "max", rotation_seed=RS)
        w.client_id, w._instance = 77, 0  # every compressor draws the same Philox stream
        return w

    msgs = [(encode_updates_dict({f"t{t}": c.xg[o:o + n] * (1 + 0.25 * k) for t, (o, n) in enumerate(zip(c.plan.offsets, c.sizes))},
                                 comp()), 10 + k) for k in range(3)]
    shapes = [(f"t{t}", (n,)) for t, n in enumerate(c.sizes)]
    twin, agg, l2 = (DeviceAggregator(shapes, device=c.gpu) for _ in range(3))
    twin.accumulate_many(msgs)
    want_avg, want = twin.apply_and_encode(comp())
    agg.fuse_bucketed_max_step = True
    avg, layers = agg.sum_apply_encode(msgs, comp())
    assert agg.plan.last_encoder == "bucketed_ps_max"
    assert [L.SerializeToString() for L in layers] == [L.SerializeToString() for L in want]  # every field of every LayerState
    assert all(torch.equal(avg[n].view(torch.int32), want_avg[n].view(torch.int32)) for n, _ in shapes)
    assert torch.equal(agg.acc.view(torch.int32), twin.acc.view(torch.int32))
    assert (agg.update_count, agg.total_samples) == (twin.update_count, twin.total_samples)
    l2.fuse_bucketed_max_step = True  # an L2 compressor keeps today's route, which ends in the L2 step either way
    l2.sum_apply_encode(msgs, comp("l2"))
    assert l2.plan.last_encoder == "bucketed_ps"


@pytest.mark.parametrize("bad", ["bucket_size", "no_client_no_acc", "avg_overlaps_payload"])
def test_refused_with_the_outputs_untouched(case, bad):
    c, p = case(512), case(512).plan
    qs, ms = c.clients(True, 8, 2)
    q_out, m_out = torch.full_like(qs[0], 3), torch.full_like(ms[0], 3.0)
    avg_out = qs[1].view(torch.float32) if bad == "avg_overlaps_payload" else torch.full_like(c.acc, 7.0)
    before = avg_out.clone()
    with pytest.raises(ValueError):
        p.ps_sum_encode_bucketed_max(None, [] if bad == "no_client_no_acc" else qs, [] if bad == "no_client_no_acc" else ms, 32,
                                     256, 500 if bad == "bucket_size" else 512, DIV, 8, rotate=True, rotation_seed=RS,
                                     avg_out=avg_out, q_out=q_out, bnorm_out=m_out)
    torch.cuda.synchronize()
    assert torch.equal(avg_out.view(torch.int32), before.view(torch.int32))  # bit patterns: a payload read as fp32 holds NaNs
    assert bool((q_out == 3).all()) and bool((m_out == 3.0).all())
