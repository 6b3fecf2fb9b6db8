"""Bucketed QSGD on the bit-packed wire (omf_qsgd_*_bucketed_packed): the encoder that packs inside the encode
pass held to the CPU oracle (levels bucket by bucket, then oracle.bitpack) and to the two-call path it replaces,
the packed bucketed decoder and K-client sum held to the numpy rule, and the public path.

One plan per bucket size d with tensors of less than a quad, one less / exactly / one more than a 32-element
group, a bucket and a 4 Ki block, a partial group inside a partial bucket in a block's second row and more than
one 16 Ki item; an all-zero bucket, a bucket with one non-zero element; canary words in the packed arena and
guards round both outputs."""

import numpy as np
import pytest
import torch

import oracle
from omnifed_amd import codec
from omnifed_amd.hybrid.communicator.global_grpc_compression import (build_global_compressor, decode_layer_tensor,
                                                                     decode_updates_dict, decode_updates_into,
                                                                     encode_layer_state, encode_updates_dict,
                                                                     wire_size)
from omnifed_amd.hybrid.compression import QSGD_BUCKETED_PACKED_COMPRESSION_NAME
from omnifed_amd.ps import DeviceAggregator
from oracle import bitpack

pytestmark = pytest.mark.gpu

SIZES = codec.BUCKET_SIZES
SEED, OFF = 0xB0C, 3
GUARD = 64
CANARY = 0x5A5A5A5A


def _sizes(d):
    return [1, 3, 31, 32, 33, d - 1, d, d + 1, 2 * d + 5, 4095, 4096, 4097, 4096 + d + 1, 16384 - 1,
            16384 + d // 2 + 3]


@pytest.fixture(scope="module")
def arenas(gpu):
    """d -> (plan, x, mask, bidx): the arena, the mask of its tensors' elements and every element's index into
    the bucket-norm arena."""
    out = {}
    for d in SIZES:
        sizes = _sizes(d)
        plan = codec.Plan(sizes, device=gpu)
        boff, _ = plan.bucket_layout(d)
        g = torch.Generator(device=gpu).manual_seed(d)
        x = torch.full((plan.arena_end,), 3e4, device=gpu)
        mask = torch.zeros(plan.arena_end, dtype=torch.bool)
        bidx = np.zeros(plan.arena_end, dtype=np.int64)
        for o, n, b in zip(plan.offsets, sizes, boff):
            x[o:o + n] = torch.randn(n, device=gpu, generator=g) * 1e-3
            mask[o:o + n] = True
            bidx[o:o + n] = b + np.arange(n) // d
        o = plan.offsets[8]  # 2 d + 5 elements: bucket 0 all zero, bucket 1 one non-zero element
        x[o:o + 2 * d] = 0.0
        x[o + d + 7] = -2.5e-3
        out[d] = (plan, x, mask, bidx)
    return out


def _written(plan, mask, b):
    """The mask of the packed arena's words whose 32-element group holds a tensor element."""
    groups = -(-plan.arena_end // 32)
    m = torch.zeros(groups * 32, dtype=torch.bool)
    m[:plan.arena_end] = mask
    return m.view(groups, 32).any(dim=1).repeat_interleave(b)


def _draw_kw(plan, x, d, draws, gpu):
    kw = {"seed": SEED, "offset": OFF}
    if draws == "u":
        kw["u"] = torch.rand(plan.arena_end, device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    if draws == "bnorm_in":
        kw["bnorm_in"] = plan.qsgd_norms_bucketed(x, d) * 1.25
    return kw


ENC_CASES = [(s, "philox") for s in (0, 3, 4, 8, 12, 20)] + [(4, "u"), (4, "bnorm_in")]


@pytest.mark.parametrize("s,draws", ENC_CASES)
@pytest.mark.parametrize("d", SIZES)
def test_fused_encode_equals_oracle_and_the_two_call_path(gpu, arenas, d, s, draws):
    plan, x, mask, _ = arenas[d]
    boff, nb = plan.bucket_layout(d)
    x_before = x.clone()
    L = 2 ** s
    b = codec.packed_bits(L)
    assert b == s + 2
    kw = _draw_kw(plan, x, d, draws, gpu)
    words = plan.packed_words(L)
    pbuf = torch.full((words + 2 * GUARD,), CANARY, dtype=torch.int32, device=gpu)
    nbuf = torch.full((nb + 2 * GUARD,), -7.0, device=gpu)
    packed, bn = plan.qsgd_encode_bucketed_packed(x, s, d, packed_out=pbuf[GUARD:GUARD + words],
                                                  bnorm_out=nbuf[GUARD:GUARD + nb], **kw)
    assert plan.last_encoder == "bucketed_packed"
    torch.cuda.synchronize()
    wr = _written(plan, mask, b).to(gpu)
    assert bool((packed[~wr] == CANARY).all())  # untouched groups
    assert bool((pbuf[:GUARD] == CANARY).all()) and bool((pbuf[GUARD + words:] == CANARY).all())
    assert bool((nbuf[:GUARD] == -7.0).all()) and bool((nbuf[GUARD + nb:] == -7.0).all())
    assert torch.equal(x.view(torch.int32), x_before.view(torch.int32))
    # the norms: the bucketed encoder's bits
    want_bn = kw["bnorm_in"] if draws == "bnorm_in" else plan.qsgd_norms_bucketed(x, d)
    assert torch.equal(bn.view(torch.int32), want_bn.view(torch.int32))
    # the two-call path's words on every written group, from either output assignment
    width = codec.storage_width(L)
    q, bn2 = plan.qsgd_encode_bucketed(x, s, d, **kw)
    two = plan.qsgd_pack(q, width, L, packed_out=torch.full((words,), CANARY, dtype=torch.int32, device=gpu))
    assert torch.equal(bn2.view(torch.int32), bn.view(torch.int32))
    assert torch.equal(packed[wr], two[wr])
    try:
        plan.set_bucket_pack(1)
        other, _ = plan.qsgd_encode_bucketed_packed(
            x, s, d, packed_out=torch.full((words,), CANARY, dtype=torch.int32, device=gpu), **kw)
    finally:
        plan.set_bucket_pack(0)
    assert torch.equal(other, packed)
    # the oracle: levels bucket by bucket against the kernel's own norm, then the tensor's packed stream
    xs, bn_h = x.cpu(), bn.cpu()
    ph = packed.cpu().numpy().view(np.uint8)
    for t, (o, n) in enumerate(zip(plan.offsets, plan.sizes)):
        u = kw["u"].cpu()[o:o + n] if "u" in kw else torch.from_numpy(oracle.philox_uniforms(SEED, OFF, t, n))
        lv = [oracle.qsgd_quantize(xs[o + j * d:o + min((j + 1) * d, n)], s, norm=float(bn_h[boff[t] + j]),
                                   u=u[j * d:min((j + 1) * d, n)])[0].long().numpy() for j in range(-(-n // d))]
        assert ph[o * b // 8:o * b // 8 + (n * b + 7) // 8].tobytes() == bitpack.pack(np.concatenate(lv), L), t


def _message(plan, d, gpu, L, seed):
    """A message no encoder made: codes uniform in [0, 2 L], bucket norms with zeros and infinities."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    _, nb = plan.bucket_layout(d)
    width = codec.storage_width(L)
    q = torch.randint(-L, L + 1, (plan.payload_elems(width),), device=gpu, generator=g,
                      dtype=torch.int32).to(torch.int8 if width == 8 else torch.int32)
    bn = torch.rand(nb, device=gpu, generator=g) * 4.0
    bn[::7] = 0.0
    bn[3::11] = float("inf")
    return q, plan.qsgd_pack(q, width, L), bn


def _decode_np(q, bn, bidx, L):
    with np.errstate(invalid="ignore", over="ignore"):
        n = bidx.size
        return ((bn.cpu().numpy()[bidx] * q.cpu().numpy()[:n].astype(np.float32)).astype(np.float32)
                / np.float32(L)).astype(np.float32)


@pytest.mark.parametrize("accumulate", (False, True))
@pytest.mark.parametrize("L", (16, 100, 256))
@pytest.mark.parametrize("d", SIZES)
def test_packed_bucketed_decode_of_foreign_messages(gpu, arenas, d, L, accumulate):
    plan, _, mask, bidx = arenas[d]
    q, packed, bn = _message(plan, d, gpu, L, 11)
    y = torch.full((plan.arena_end + GUARD,), 0.375, device=gpu)
    plan.qsgd_decode_bucketed_packed(packed, L, d, bn, y_out=y[:plan.arena_end], accumulate=accumulate)
    want = _decode_np(q, bn, bidx, L)
    if accumulate:
        with np.errstate(invalid="ignore"):
            want = np.float32(0.375) + want
    want = np.where(mask.numpy(), want, np.float32(0.375))  # padding keeps its bytes
    got = y.cpu().numpy()
    assert np.array_equal(got[:plan.arena_end], want, equal_nan=True)
    assert (got[plan.arena_end:] == 0.375).all()


@pytest.mark.parametrize("divisor", (None, 7.0))
@pytest.mark.parametrize("init", (False, True))
@pytest.mark.parametrize("K", (1, 3, 9))
@pytest.mark.parametrize("d,L", ((64, 16), (1024, 256), (4096, 100), (128, 256), (512, 100), (2048, 16)))
def test_packed_bucketed_decode_sum_is_the_sequential_sum(gpu, arenas, d, L, K, init, divisor):
    plan, _, mask, bidx = arenas[d]
    msgs = [_message(plan, d, gpu, L, 20 + k) for k in range(K)]
    for m in msgs:
        m[2][3::11] = 0.5  # finite terms: the sum's order is what is checked
    y = torch.full((plan.arena_end + GUARD,), 0.375, device=gpu)
    plan.qsgd_decode_sum_bucketed_packed([m[1] for m in msgs], L, d, [m[2] for m in msgs], y_out=y[:plan.arena_end],
                                         init=init, divisor=divisor)
    s = np.full(plan.arena_end, 0.375 if init else 0.0, dtype=np.float32)
    for q, _, bn in msgs:
        s = (s + _decode_np(q, bn, bidx, L)).astype(np.float32)
    if divisor is not None:
        s = (s / np.float32(divisor)).astype(np.float32)
    pad = np.float32(0.375) if init else np.float32(0.0)  # init: padding kept; else written (+0 / divisor)
    want = np.where(mask.numpy(), s, pad)
    got = y.cpu().numpy()
    assert np.array_equal(got[:plan.arena_end].view(np.int32), want.view(np.int32))
    assert (got[plan.arena_end:] == 0.375).all()


def test_an_arena_of_less_than_a_group(gpu):
    plan = codec.Plan([7], device=gpu)
    x = torch.randn(plan.arena_end, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    packed, bn = plan.qsgd_encode_bucketed_packed(x, 4, 64, seed=SEED)
    q, _ = plan.qsgd_encode_bucketed(x, 4, 64, seed=SEED)
    assert torch.equal(packed, plan.qsgd_pack(q, 8, 16))
    want = plan.qsgd_decode_bucketed(q, 8, 16, 64, bn)
    assert torch.equal(plan.qsgd_decode_bucketed_packed(packed, 16, 64, bn)[:7], want[:7])
    assert torch.equal(plan.qsgd_decode_sum_bucketed_packed([packed, packed], 16, 64, [bn, bn])[:7], (want + want)[:7])


def test_public_path_wire_and_aggregator(gpu):
    d, s = 256, 4
    shapes = {"w": (37, 129), "zero": (300,), "b": (1000,)}
    mk = lambda **kw: build_global_compressor(enabled=True, scheme="qsgd", bit_width=s, bucket_size=d, device=gpu, **kw)
    g = torch.Generator(device=gpu).manual_seed(5)
    decoded, updates = [], []
    for c in range(3):
        comp, plain = mk(bucket_packed=True), mk()
        comp.client_id = plain.client_id = c
        plain._instance = comp._instance  # one Philox key, and both at their first call: the same draws
        upd = {k: torch.randn(sh, device=gpu, generator=g) * 1e-3 for k, sh in shapes.items()}
        upd["zero"].zero_()
        layers = encode_updates_dict(upd, comp)
        assert [L.compression_type for L in layers] == [QSGD_BUCKETED_PACKED_COMPRESSION_NAME, "",
                                                        QSGD_BUCKETED_PACKED_COMPRESSION_NAME]
        for L in (layers[0], layers[2]):
            n = int(np.prod(shapes[L.layer_name]))
            assert (list(L.param_shape), L.width, L.level, L.values_dtype) == ([d], 6, 16, "packed.u6")
            assert list(L.original_shape) == list(shapes[L.layer_name])
            assert len(L.values_data) == -(-n * 6 // 8) and len(L.meta_tensor) == 4 * -(-n // d)
        assert wire_size(layers)["payload_bytes"] == sum(
            len(L.values_data) + len(L.meta_tensor) + 4 * len(L.param_update) for L in layers)
        # the same client on the unpacked bucketed wire (same seeds): the same floats
        dec, ref = decode_updates_dict(layers, device=gpu), decode_updates_dict(encode_updates_dict(upd, plain), device=gpu)
        for k in shapes:
            assert torch.equal(dec[k].view(torch.int32), ref[k].view(torch.int32)), k
        assert bool(dec["w"].any()) and not bool(dec["zero"].any())
        decoded.append(dec)
        updates.append((layers, 10 + c))
    agg = DeviceAggregator(list(shapes.items()), device=gpu)
    agg.accumulate_many(updates)
    per = DeviceAggregator(list(shapes.items()), device=gpu)
    for layers, ns in updates:
        per.accumulate_layers(layers, ns)
    assert agg.update_count == 3 and agg.total_samples == 33
    assert torch.equal(agg.acc.view(torch.int32), per.acc.view(torch.int32)) and bool(agg.acc.any())
    # without the dense layers the three updates are one run: a single qsgd_decode_sum_bucketed_packed
    run = DeviceAggregator(list(shapes.items()), device=gpu)
    run.accumulate_many([([L for L in layers if L.compression_type], ns) for layers, ns in updates])
    assert torch.equal(run.acc.view(torch.int32), agg.acc.view(torch.int32))
    # single-tensor entry points and the PS downlink stay on the new wire
    comp = mk(bucket_packed=True)
    layer = encode_layer_state("w", upd["w"], comp)
    assert layer.compression_type == QSGD_BUCKETED_PACKED_COMPRESSION_NAME
    one = decode_layer_tensor(layer, device=gpu)
    target = {"w": torch.zeros(shapes["w"], device=gpu)}
    decode_updates_into([layer], target)
    assert torch.equal(target["w"].view(torch.int32), one.view(torch.int32)) and bool(one.any())
    _, down = agg.apply_and_encode(comp)
    assert {L.compression_type for L in down if L.compression_type} == {QSGD_BUCKETED_PACKED_COMPRESSION_NAME}
