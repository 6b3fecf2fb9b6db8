"""Packed QSGD updates (the opt-in bit-packed wire, ``QSGDBitPackedCompression``) through the parameter
server: ``DeviceAggregator`` accepts them and leaves, byte for byte, what the plain QSGD twins of the same
levels leave; ``accumulate_many`` sums a run of packed updates with one ``qsgd_decode_sum_packed`` call.

Each client's plain layers come from ``encode_updates_dict``; the packed twin of a layer is derived on the
CPU (``oracle.bitpack.pack`` of the plain layer's levels), so the two carry identical levels whatever the
compressors would draw.
"""

import os
import sys

import numpy as np
import pytest
import torch

from oracle import bitpack
from omnifed_amd import ps
from omnifed_amd.hybrid.communicator import global_grpc_pb2 as pb
from omnifed_amd.hybrid.communicator.global_grpc_compression import (encode_updates_dict,
                                                                     qsgd_packed_layer_from_payload)
from omnifed_amd.hybrid.compression import QSGD_PACKED_COMPRESSION_NAME
from omnifed_amd.hybrid.compression.qsgd import QSGDQuantCompression

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMED = [("a", (5,)), ("b", (64,)), ("c", (1000,)), ("d", (4097,)), ("e", (13001,)), ("f", (9,))]  # test_gpu_decode_sum's


def _qsgd(bits, k, **kw):
    torch.manual_seed(500 + k)
    return QSGDQuantCompression(bit_width=bits, **kw)


def _updates(gpu, k, named=NAMED):
    g = torch.Generator().manual_seed(100 + k)
    return {n: (torch.randn(s, generator=g) * (0.1 + k)).to(gpu) for n, s in named}


def _plain(gpu, k, bits=4, named=NAMED):
    layers = encode_updates_dict(_updates(gpu, k, named), _qsgd(bits, k), weight=k + 2)
    assert all(L.compression_type == "QSGDQuantCompression" for L in layers)
    return layers


def _twin(L):
    """The packed layer carrying the plain QSGD layer's levels and norm."""
    q = np.frombuffer(L.values_data, np.int8 if L.width == 8 else np.int32)
    norm = np.frombuffer(L.meta_tensor, np.float32)[0]
    T = qsgd_packed_layer_from_payload(L.layer_name, tuple(L.original_shape), bitpack.pack(q, L.level), norm, L.level)
    assert T.compression_type == QSGD_PACKED_COMPRESSION_NAME and T.meta_tensor == L.meta_tensor
    return T


def _packed(layers):
    return [_twin(L) for L in layers]


def _pair(gpu):
    return ps.DeviceAggregator(NAMED, device=gpu), ps.DeviceAggregator(NAMED, device=gpu)


def _same_state(a, b):
    assert a.acc.cpu().numpy().tobytes() == b.acc.cpu().numpy().tobytes()
    assert (a.update_count, a.total_samples) == (b.update_count, b.total_samples)
    assert np.abs(b.acc.cpu().numpy()).max() > 0


def _count(monkeypatch, agg):
    calls = []
    for name in ("qsgd_decode_sum_packed", "qsgd_decode_sum"):
        real = getattr(agg.plan, name)
        monkeypatch.setattr(agg.plan, name,
                            lambda xs, *a, _r=real, _n=name, **k: (calls.append((_n, len(xs))), _r(xs, *a, **k))[1])
    return calls


@pytest.mark.parametrize("bits", [4, 8])
def test_accumulate_layers_packed_equals_plain(gpu, bits):
    packed, plain = _pair(gpu)
    for k in range(3):
        layers = _plain(gpu, k, bits)
        plain.accumulate_layers(layers, 10 + k)
        packed.accumulate_layers(_packed(layers), 10 + k)
    _same_state(packed, plain)
    assert packed.update_count == 3


def test_accumulate_many_one_packed_run(gpu, monkeypatch):
    updates = [(_packed(_plain(gpu, k)), 10 + k) for k in range(3)]
    many, one = _pair(gpu)
    for layers, ns in updates:
        one.accumulate_layers(layers, ns)
    calls = _count(monkeypatch, many)
    many.accumulate_many(updates)
    _same_state(many, one)
    assert calls == [("qsgd_decode_sum_packed", 3)]
    many.reset()
    calls.clear()
    many.accumulate_many(updates, max_batch=2)
    _same_state(many, one)
    assert calls == [("qsgd_decode_sum_packed", 2), ("qsgd_decode_sum_packed", 1)]


def test_accumulate_many_packed_and_plain_runs_never_merge(gpu, monkeypatch):
    plain = [_plain(gpu, k) for k in range(4)]
    updates = [(_packed(plain[0]), 10), (_packed(plain[1]), 11), (plain[2], 12), (_packed(plain[3]), 13)]
    many, one, twins = ps.DeviceAggregator(NAMED, device=gpu), *_pair(gpu)
    for layers, ns in updates:
        one.accumulate_layers(layers, ns)
    for k, layers in enumerate(plain):
        twins.accumulate_layers(layers, 10 + k)
    calls = _count(monkeypatch, many)
    many.accumulate_many(updates)
    _same_state(many, one)
    _same_state(many, twins)
    assert calls == [("qsgd_decode_sum_packed", 2), ("qsgd_decode_sum", 1), ("qsgd_decode_sum_packed", 1)]


def test_packed_8_bit_codes_do_not_join_an_int8_run(gpu, monkeypatch):
    """s = 6: 64 levels are 8-bit codes on the packed wire and int8 on the plain one, so a packed and a
    plain update agree in (width, level); the runs still split, on the wire form alone."""
    plain = [_plain(gpu, k, 6) for k in range(2)]
    updates = [(_packed(plain[0]), 1), (plain[1], 2)]
    assert {L.width for L in updates[0][0]} == {L.width for L in updates[1][0]} == {8}
    many, one = _pair(gpu)
    for layers, ns in updates:
        one.accumulate_layers(layers, ns)
    calls = _count(monkeypatch, many)
    many.accumulate_many(updates)
    _same_state(many, one)
    assert calls == [("qsgd_decode_sum_packed", 1), ("qsgd_decode_sum", 1)]


def test_mixed_packed_and_plain_layers_in_one_update_are_refused(gpu):
    layers = _plain(gpu, 0)
    mixed = [_twin(L) if L.layer_name in ("c", "e") else L for L in layers]
    agg, ref = _pair(gpu)
    before = _plain(gpu, 1)
    agg.accumulate_layers(_packed(before), 7)
    ref.accumulate_layers(before, 7)
    with pytest.raises(ValueError, match="mixed QSGD width/level"):
        agg.accumulate_layers(mixed, 3)
    _same_state(agg, ref)  # untouched by the refused update


def test_unknown_compression_type_still_refused(gpu):
    agg = ps.DeviceAggregator(NAMED, device=gpu)
    L = _twin(_plain(gpu, 0)[2])
    L.compression_type = "NoSuchCompression"
    with pytest.raises(ValueError, match="Unsupported compression_type"):
        agg.accumulate_layers([L], 1)
    assert agg.update_count == 0 and not agg.acc.cpu().numpy().any()


def test_packed_layer_one_byte_short(gpu):
    updates = [(_packed(_plain(gpu, k)), 10 + k) for k in range(4)]
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


def test_missing_layer_adds_positive_zero(gpu):
    plain = [_plain(gpu, k) for k in range(3)]
    plain[1] = [L for L in plain[1] if L.layer_name != "c"]  # norm 0 for it
    many, one, twins = ps.DeviceAggregator(NAMED, device=gpu), *_pair(gpu)
    for k, layers in enumerate(plain):
        twins.accumulate_layers(layers, 10 + k)
        one.accumulate_layers(_packed(layers), 10 + k)
    many.accumulate_many([(_packed(layers), 10 + k) for k, layers in enumerate(plain)])
    _same_state(one, twins)
    _same_state(many, twins)
    # a lone update without "c" leaves +0 there
    lone = ps.DeviceAggregator(NAMED, device=gpu)
    lone.accumulate_layers(_packed(plain[1]), 1)
    assert not lone._slice("c").cpu().numpy().view(np.uint32).any()


def test_accumulate_updates_with_a_packed_wire_compressor(gpu):
    agg = ps.DeviceAggregator(NAMED, device=gpu)
    comp = _qsgd(4, 0, device=gpu, packed_wire=True)
    agg.accumulate_updates(_updates(gpu, 0), comp, number_samples=6, weight=2)
    assert (agg.update_count, agg.total_samples) == (1, 6)
    acc = agg.acc.cpu().numpy()
    assert np.isfinite(acc).all() and np.abs(acc).max() > 0


def test_servicer_takes_packed_updates(gpu):
    from omnifed_amd.hybrid.communicator.global_grpc_server import CentralServerServicer

    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))
    from grpc_loopback import nested_model

    shapes = [("a", (100, 10)), ("b", (7,)), ("c", (4097,))]
    servers = []
    for _ in range(2):
        model = nested_model(shapes, gpu)
        servers.append((CentralServerServicer(num_clients=2, model=model, device=gpu), model))
    named = [(n, tuple(p.shape)) for n, p in servers[0][1].named_parameters()]
    for k in range(2):
        layers = _plain(gpu, k, 4, named)
        for (srv, _), msg in zip(servers, (_packed(layers), layers)):
            r = srv.SendUpdate(pb.ModelUpdate(client_id=f"c{k}", round_number=1, layers=msg, number_samples=5 + k), None)
            assert r.success and r.updates_received == k + 1, r.message
    (ps_srv, packed_model), (pl_srv, plain_model) = servers
    assert ps_srv.current_round == 1 and pl_srv.current_round == 1
    for (n, a), (_, b) in zip(packed_model.named_parameters(), plain_model.named_parameters()):
        assert a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes(), n
        assert a.detach().abs().max() > 0
