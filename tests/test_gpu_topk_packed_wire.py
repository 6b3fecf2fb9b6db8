"""The opt-in bit-packed Top-K wire (``TopKBitPackedCompression``) end to end against the plain Top-K wire.

A packed compressor and a plain one run two error-feedback calls of ``encode_updates_dict`` on equal inputs, a
dict of fp32 tensors of 1 000 003, 70 000, 4 097, 33 and 1 elements at ratio 0.01.  The packed wire changes how
the indices are written and nothing else: values, residuals and every decode give the plain wire's bytes, and a
packed layer's ``indices_data`` is the numpy oracle's packing (tests/golden/topk_packed_inputs.py) of the plain
layer's int64 indices.  No tolerance anywhere.
"""

import numpy as np
import pytest
import torch

import topk_packed_inputs as P
from omnifed_amd.hybrid.communicator import global_grpc_pb2 as pb
from omnifed_amd.hybrid.communicator.global_grpc_compression import (
    build_global_compressor,
    decode_layer_tensor,
    decode_updates_dict,
    decode_updates_into,
    encode_layer_state,
    encode_updates_dict,
    topk_layer_from_payload,
)
from omnifed_amd.hybrid.compression import TOPK_COMPRESSION_NAME, TOPK_PACKED_COMPRESSION_NAME
from omnifed_amd.ps import DeviceAggregator

pytestmark = pytest.mark.gpu

SHAPES = [(1_000_003,), (700, 100), (4_097,), (33,), (1,)]
NAMES = [f"t{i}" for i in range(len(SHAPES))]
assert [int(np.prod(s)) for s in SHAPES] == P.WIRE_SIZES


def _updates(gpu, call, dtype=torch.float32):
    g = torch.Generator().manual_seed(100 + call)
    return {n: (torch.randn(*s, generator=g) * 1e-3).to(dtype).to(gpu) for n, s in zip(NAMES, SHAPES)}


def _compressors(gpu):
    return (build_global_compressor(enabled=True, scheme="topk", compress_ratio=P.WIRE_RATIO, device=gpu, packed_wire=True),
            build_global_compressor(enabled=True, scheme="topk", compress_ratio=P.WIRE_RATIO, device=gpu))


@pytest.fixture(scope="module")
def rounds(gpu):
    """Two error-feedback calls: per call the inputs, the packed and the plain layers, the packed wire's stats
    and both compressors' residual bytes."""
    packed, plain = _compressors(gpu)
    out = []
    for call in range(2):
        upd = _updates(gpu, call)
        stats = {}
        lp = encode_updates_dict(upd, packed, stats=stats)
        ll = encode_updates_dict(upd, plain)
        res = [(packed.residual.residuals[n].cpu().numpy().tobytes(), plain.residual.residuals[n].cpu().numpy().tobytes())
               for n in NAMES]
        out.append(dict(upd=upd, packed=lp, plain=ll, stats=stats, res=res))
    return out


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same_dicts(a, b):
    assert list(a) == list(b)
    for n in a:
        assert a[n].shape == b[n].shape and a[n].dtype == b[n].dtype and a[n].device == b[n].device, n
        assert _bytes(a[n]) == _bytes(b[n]), n


def test_encodes_agree(rounds):
    for call, r in enumerate(rounds):
        total = 0
        for Lp, Ll, n, (rp, rl) in zip(r["packed"], r["plain"], P.WIRE_SIZES, r["res"]):
            key = (call, Lp.layer_name)
            b = P.index_bits(n)
            k = max(1, int(n * P.WIRE_RATIO))
            assert Lp.layer_name == Ll.layer_name and list(Lp.original_shape) == list(Ll.original_shape), key
            assert (Lp.compression_type, Ll.compression_type) == (TOPK_PACKED_COMPRESSION_NAME, TOPK_COMPRESSION_NAME)
            assert (Lp.values_dtype, Lp.indices_dtype, Lp.width) == ("torch.float32", f"packed.u{b}", b), key
            assert Lp.values_data == Ll.values_data and len(Lp.values_data) == 4 * k, key
            idx = np.frombuffer(Ll.indices_data, np.int64)
            assert Lp.indices_data == P.pack_indices(idx, n), key
            assert len(Lp.indices_data) == (k * b + 7) // 8, key
            assert rp == rl, key
            total += 4 * k + (k * b + 7) // 8
        assert r["stats"]["payload_bytes"] == total and r["stats"]["layers"] == len(NAMES)
    assert rounds[0]["res"] != rounds[1]["res"]  # the second call ran on the first one's residual


@pytest.mark.parametrize("device", ["cpu", "cuda"])
def test_decode_updates_dict(rounds, device):
    for r in rounds:
        _same_dicts(decode_updates_dict(r["packed"], device=device), decode_updates_dict(r["plain"], device=device))
    # a message holding both wires: each kind decoded in its own batch
    r = rounds[1]
    mixed = [r["packed"][0], r["plain"][1], r["packed"][2], r["plain"][3], r["packed"][4]]
    _same_dicts(decode_updates_dict(mixed, device=device), decode_updates_dict(r["plain"], device=device))


def test_decode_layer_tensor_with_and_without_base(gpu, rounds):
    r = rounds[1]
    g = torch.Generator().manual_seed(5)
    for Lp, Ll, shape in zip(r["packed"], r["plain"], SHAPES):
        for dev in (None, gpu):
            a, b = decode_layer_tensor(Lp, device=dev), decode_layer_tensor(Ll, device=dev)
            assert a.device == b.device and a.shape == b.shape == torch.Size(shape) and _bytes(a) == _bytes(b)
        for base in (torch.randn(*shape, generator=g).to(gpu), torch.randn(*shape, generator=g).half()):
            a, b = decode_layer_tensor(Lp, base_tensor=base), decode_layer_tensor(Ll, base_tensor=base)
            assert a.device == b.device == base.device and a.dtype == b.dtype == base.dtype
            assert _bytes(a) == _bytes(b) and _bytes(a) != _bytes(base)
    both = decode_updates_dict(r["packed"], base_updates={"t1": torch.ones(700, 100, device=gpu)}, device=gpu)
    want = decode_updates_dict(r["plain"], base_updates={"t1": torch.ones(700, 100, device=gpu)}, device=gpu)
    _same_dicts(both, want)


def test_decode_updates_into_nonzero_targets(gpu, rounds):
    from omnifed_amd import codec

    r = rounds[1]
    g = torch.Generator().manual_seed(6)
    start = {n: torch.randn(*s, generator=g).to(gpu) for n, s in zip(NAMES, SHAPES)}
    plan = codec.Plan.get(P.WIRE_SIZES, device=gpu)

    def targets(kind):
        if kind == "arena":  # views of one arena in the plan's layout: one launch
            arena = torch.zeros(plan.arena_end, device=gpu)
            out = {n: arena[o:o + k].view(s) for n, s, o, k in zip(NAMES, SHAPES, plan.offsets, plan.sizes)}
            for n in NAMES:
                out[n].copy_(start[n])
            return out
        return {n: (t.clone() if kind == "separate" else t.cpu().clone()) for n, t in start.items()}

    for kind in ("arena", "separate", "cpu"):
        a, b = targets(kind), targets(kind)
        decode_updates_into(r["packed"], a)
        decode_updates_into(r["plain"], b)
        _same_dicts(a, b)
        assert all(_bytes(a[n]) != _bytes(start[n]) for n in NAMES), kind


def _aggregate(gpu, updates):
    agg = DeviceAggregator(list(zip(NAMES, SHAPES)), device=gpu)
    for layers in updates:
        agg.accumulate_layers(layers, number_samples=3)
    return agg, agg.apply()


def test_ps_two_clients(gpu, rounds):
    _, a = _aggregate(gpu, [rounds[0]["packed"], rounds[1]["packed"]])
    _, b = _aggregate(gpu, [rounds[0]["plain"], rounds[1]["plain"]])
    _same_dicts(a, b)
    assert all(a[n].abs().sum() > 0 for n in NAMES)


def _raw_packed_layer(name, shape, values, codes):
    """A packed layer whose codes need not be below n (no encoder writes one)."""
    n = int(np.prod(shape))
    b = P.index_bits(n)
    L = pb.layer_state(layer_name=name)
    L.compression_type = TOPK_PACKED_COMPRESSION_NAME
    L.values_data = np.asarray(values, np.float32).tobytes()
    L.indices_data = np.packbits(P._bits_of(np.asarray(codes, np.uint64), b), bitorder="little").tobytes()
    L.values_dtype = "torch.float32"
    L.indices_dtype = f"packed.u{b}"
    L.original_shape.extend(list(shape))
    L.width = b
    return L


def test_code_out_of_range_names_its_layer(gpu, rounds):
    r = rounds[0]
    bad = _raw_packed_layer("t3", (33,), [1.0, 2.0, 3.0], [5, 40, 0])  # b = 6: 40 is a code, not an index
    msg = [L if L.layer_name != "t3" else bad for L in r["packed"]]
    with pytest.raises(IndexError, match="'t3'.*out of bounds for size 33"):
        decode_layer_tensor(bad, device=gpu)
    with pytest.raises(IndexError, match="'t3'.*out of bounds for size 33"):
        decode_updates_dict(msg, device=gpu)
    targets = {n: torch.ones(*s, device=gpu) for n, s in zip(NAMES, SHAPES)}
    with pytest.raises(IndexError, match="'t3'.*out of bounds for size 33"):
        decode_updates_into(msg, targets)
    assert all(bool((t == 1).all()) for t in targets.values())  # raised before any target was written
    agg = DeviceAggregator(list(zip(NAMES, SHAPES)), device=gpu)
    agg.accumulate_layers(r["packed"], number_samples=1)
    before = _bytes(agg.acc)
    with pytest.raises(IndexError, match="'t3'.*out of bounds for size 33"):
        agg.accumulate_layers(msg, number_samples=1)
    assert _bytes(agg.acc) == before and agg.update_count == 1


def test_repeated_index_last_wins(gpu):
    """A layer that repeats an index (numpy's rule: the last value wins), and one with more values than
    elements, which must: the packed wire takes the plain wire's paths."""
    vals, idx = [1.0, 2.0, 9.0, 4.0], [3, 7, 3, 32]
    many_v, many_i = np.arange(1, 8, dtype=np.float32), [4, 0, 3, 4, 1, 0, 2]  # k = 7 > n = 5
    pa, pb_ = _raw_packed_layer("a", (33,), vals, idx), _raw_packed_layer("b", (5,), many_v, many_i)
    la = topk_layer_from_payload("a", (33,), np.float32(vals), np.int64(idx))
    lb = topk_layer_from_payload("b", (5,), many_v, np.int64(many_i))
    for device in ("cpu", "cuda"):
        got = {**decode_updates_dict([pa], device=device), **decode_updates_dict([pb_], device=device)}
        want = {**decode_updates_dict([la], device=device), **decode_updates_dict([lb], device=device)}
        _same_dicts(got, want)
        assert got["a"][3] == 9.0 and got["a"][7] == 2.0 and got["a"][32] == 4.0
        assert got["b"].tolist() == [6.0, 5.0, 7.0, 3.0, 4.0]
    assert _bytes(decode_layer_tensor(pb_, device=gpu)) == _bytes(decode_layer_tensor(lb, device=gpu))
    base = torch.full((5,), 8.0, device=gpu)
    assert decode_layer_tensor(pb_, base_tensor=base).tolist() == [6.0, 5.0, 7.0, 3.0, 4.0]
    ta = {"a": torch.ones(33, device=gpu), "b": torch.ones(5, device=gpu)}
    tb = {n: t.clone() for n, t in ta.items()}
    for msg, t in (([pa], ta), ([pb_], ta), ([la], tb), ([lb], tb)):
        decode_updates_into(msg, t)
    _same_dicts(ta, tb)
    assert ta["a"][3] == 9.0 and ta["a"][0] == 1.0
    aggs = []
    for msg in ([pa, pb_], [la, lb]):
        agg = DeviceAggregator([("a", (33,)), ("b", (5,))], device=gpu)
        agg.accumulate_layers(msg, number_samples=2)
        aggs.append(agg.apply())
    _same_dicts(*aggs)
    assert aggs[0]["a"][3] == 4.5 and aggs[0]["b"].tolist() == [3.0, 2.5, 3.5, 1.5, 2.0]


def test_mixed_wires_raise_at_the_ps(gpu, rounds):
    r = rounds[0]
    agg = DeviceAggregator(list(zip(NAMES, SHAPES)), device=gpu)
    with pytest.raises(ValueError, match="mixed Top-K wires"):
        agg.accumulate_layers([r["packed"][0], r["plain"][1]], number_samples=1)
    assert not agg.acc.any() and agg.update_count == 0
    wrong = _raw_packed_layer("t3", (32,), [1.0], [1])  # another shape than the PS's tensor: another width rule
    with pytest.raises(ValueError, match="'t3'.*32 elements, expected 33"):
        agg.accumulate_layers([wrong], number_samples=1)


def test_per_layer_path_gives_the_batched_layers(gpu, rounds):
    packed, _ = _compressors(gpu)
    for r in rounds:
        for L, (n, t) in zip(r["packed"], r["upd"].items()):
            one = encode_layer_state(n, t, packed)
            assert one.SerializeToString() == L.SerializeToString(), n
    # an integer tensor takes the per-tensor compress and is packed through a one-tensor plan
    packed2, plain2 = _compressors(gpu)
    t = torch.arange(-500, 500, device=gpu, dtype=torch.int32).reshape(10, 100)
    Lp, Ll = encode_layer_state("i", t, packed2), encode_layer_state("i", t, plain2)
    assert Lp.compression_type == TOPK_PACKED_COMPRESSION_NAME and Lp.values_data == Ll.values_data
    assert Lp.indices_data == P.pack_indices(np.frombuffer(Ll.indices_data, np.int64), 1000)


def test_fp16_round_trip(gpu):
    packed, plain = _compressors(gpu)
    for call in range(2):
        upd = _updates(gpu, 10 + call, torch.float16)
        lp, ll = encode_updates_dict(upd, packed), encode_updates_dict(upd, plain)
        for Lp, Ll, n in zip(lp, ll, P.WIRE_SIZES):
            assert Lp.values_data == Ll.values_data
            assert Lp.indices_data == P.pack_indices(np.frombuffer(Ll.indices_data, np.int64), n)
            assert _bytes(packed.residual.residuals[Lp.layer_name]) == _bytes(plain.residual.residuals[Lp.layer_name])
            assert packed.residual.residuals[Lp.layer_name].dtype == torch.float16
        dec = decode_updates_dict(lp, device=gpu)
        _same_dicts(dec, decode_updates_dict(ll, device=gpu))
        for Lp, n in zip(lp, NAMES):  # the selected values come back exactly, everything else is zero
            idx = torch.from_numpy(P.unpack_indices(Lp.indices_data, len(Lp.values_data) // 4, dec[n].numel()))
            vals = torch.from_numpy(np.frombuffer(Lp.values_data, np.float32).copy())
            flat = dec[n].reshape(-1).cpu()
            assert torch.equal(flat[idx], vals) and int((flat != 0).sum()) <= idx.numel()
