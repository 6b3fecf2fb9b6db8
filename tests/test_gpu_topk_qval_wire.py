"""The opt-in quantised Top-K value wire (``TopKQuantPackedCompression``) end to end against the CPU oracle.

A compressor with ``value_bits`` runs three error-feedback calls of ``encode_updates_dict`` on a dict of fp32
tensors of 70 000, 4 096, 33 and 1 elements, at ratio 0.01 and 0.25 and under both tie orders.  The oracle's loop
is ``oracle.topk.topk_ef_step`` per tensor, then the quantiser of tests/golden/topk_qval_inputs.py with the seed
and the call counter read from the compressor, then the error stored at the selected slots of the residual; the
layers' fields and payloads and the residuals are compared byte for byte, and every decoder's output with the
oracle's decoded values scattered at the oracle's indices.  No tolerance anywhere.
"""

import numpy as np
import pytest
import torch

import topk_packed_inputs as P
import topk_qval_inputs as Q
from omnifed_amd.hybrid.communicator import global_grpc_pb2 as pb
from omnifed_amd.hybrid.communicator.global_grpc_compression import (
    build_global_compressor,
    decode_layer_tensor,
    decode_updates_dict,
    decode_updates_into,
    encode_layer_state,
    encode_updates_dict,
    wire_size,
)
from omnifed_amd.hybrid.compression import TOPK_PACKED_COMPRESSION_NAME, TOPK_QUANT_COMPRESSION_NAME
from omnifed_amd.ps import DeviceAggregator
from oracle import topk as otopk

pytestmark = pytest.mark.gpu

SHAPES = [(700, 100), (4_096,), (33,), (1,)]
NAMES = [f"t{i}" for i in range(len(SHAPES))]
SIZES = [int(np.prod(s)) for s in SHAPES]
assert SIZES == Q.WIRE_SIZES
CASES = [(0.01, "index", 4), (0.01, "torch", 2), (0.25, "index", 8), (0.25, "torch", 5)]
assert {c[0] for c in CASES} == set(Q.WIRE_RATIOS)
CALLS = 3


def _inputs(call, plant_inf=False):
    g = torch.Generator().manual_seed(300 + call)
    upd = {n: (torch.randn(*s, generator=g) * 1e-3).contiguous() for n, s in zip(NAMES, SHAPES)}
    flat = upd["t0"].view(-1)
    flat[5], flat[9] = 7.0e-3, -7.0e-3  # two equal magnitudes inside the selection
    if plant_inf:
        upd["t1"][77] = float("inf")
    return upd


def _compressor(gpu, ratio, tie, s):
    c = build_global_compressor(enabled=True, scheme="topk", compress_ratio=ratio, device=gpu, packed_wire=True,
                                value_bits=s)
    c.tie_order = tie
    return c


def _oracle_call(upd, res, ratio, tie, s, seed, offset, stream_of=lambda t: t):
    """One call of the oracle's loop over the dict: per tensor the selection, the quantiser, the residual."""
    out = []
    for t, (n, x) in enumerate(upd.items()):
        xn = x.numpy().reshape(-1).astype(np.float32)
        k = otopk.topk_k(xn.size, ratio)
        v, idx, r = otopk.topk_ef_step(xn, res.get(n), 2 if res.get(n) is None else 1, 1.0, k, tie)
        m, q, d, e = Q.quantize(v, s, seed, offset, stream_of(t))
        if q is not None and m != 0:
            r[idx] = e
        res[n] = r
        out.append(dict(n=xn.size, k=k, v=v, idx=idx, m=m, q=q, d=v if q is None else d, res=r.copy()))
    return out


def _run(gpu, ratio, tie, s, plant_inf=False):
    comp = _compressor(gpu, ratio, tie, s)
    seed = comp.philox_key()
    res, rounds = {}, []
    for call in range(CALLS):
        upd = _inputs(call, plant_inf and call == 1)
        assert comp._calls == call
        stats = {}
        layers = encode_updates_dict({n: t.to(gpu) for n, t in upd.items()}, comp, stats=stats)
        got_res = [comp.residual.residuals[n].cpu().numpy().tobytes() for n in NAMES]
        want = _oracle_call(upd, res, ratio, tie, s, seed, call)
        rounds.append(dict(layers=layers, want=want, res=got_res, stats=stats))
    assert comp._calls == CALLS
    return rounds


@pytest.fixture(scope="module")
def runs(gpu):
    return {c: _run(gpu, *c) for c in CASES}


@pytest.fixture(scope="module")
def mixed(gpu):
    """Ratio 0.01, s = 4, an infinity planted in t1 at the second call: that layer falls back."""
    return _run(gpu, 0.01, "index", 4, plant_inf=True)


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _check_layers(rounds, s, key):
    for call, r in enumerate(rounds):
        total = 0
        for L, w, name, shape, got_res in zip(r["layers"], r["want"], NAMES, SHAPES, r["res"]):
            at = (key, call, name)
            n, k, bi = w["n"], w["k"], P.index_bits(w["n"])
            assert L.layer_name == name and tuple(L.original_shape) == shape, at
            assert L.indices_data == P.pack_indices(w["idx"], n), at
            assert (L.indices_dtype, L.width) == (f"packed.u{bi}", bi), at
            if w["q"] is None:  # the fallback: the packed-index wire with fp32 values
                assert L.compression_type == TOPK_PACKED_COMPRESSION_NAME, at
                assert L.values_data == w["v"].tobytes() and L.values_dtype == "torch.float32", at
                assert not L.meta_tensor and L.level == 0 and not L.param_shape, at
                total += 4 * k + len(L.indices_data)
            else:
                assert L.compression_type == TOPK_QUANT_COMPRESSION_NAME, at
                assert L.values_data == Q.pack_codes(w["q"], s), at
                assert len(L.values_data) == (k * (s + 2) + 7) // 8, at
                assert L.values_dtype == f"packed.q{s + 2}" and L.level == 2**s and list(L.param_shape) == [k], at
                assert L.meta_tensor == np.float32(w["m"]).tobytes() and L.meta_tensor_dtype == "torch.float32", at
                total += len(L.values_data) + len(L.indices_data) + 4
            assert got_res == w["res"].tobytes(), at
        assert r["stats"]["payload_bytes"] == total and r["stats"]["layers"] == len(NAMES), (key, call)


@pytest.mark.parametrize("case", CASES, ids=[f"r{c[0]}-{c[1]}-s{c[2]}" for c in CASES])
def test_encode_matches_the_oracle_loop(runs, case):
    rounds = runs[case]
    _check_layers(rounds, case[2], case)
    assert all(w["q"] is not None for r in rounds for w in r["want"])
    # the error feedback is live: the residual at a selected slot holds the quantisation error, not 0
    w = rounds[0]["want"][0]
    assert np.count_nonzero(w["res"][w["idx"]]) > 0
    assert rounds[0]["res"] != rounds[1]["res"] != rounds[2]["res"]


def _scatter(w, base=None):
    out = np.zeros(w["n"], np.float32) if base is None else np.array(base, np.float32).reshape(-1)
    out[w["idx"]] = w["d"]
    return out


@pytest.mark.parametrize("case", CASES, ids=[f"r{c[0]}-{c[1]}-s{c[2]}" for c in CASES])
def test_round_trips(gpu, runs, case):
    g = torch.Generator().manual_seed(8)
    for r in runs[case]:
        for device in ("cpu", "cuda"):
            dec = decode_updates_dict(r["layers"], device=device)
            for n, shape, w in zip(NAMES, SHAPES, r["want"]):
                assert dec[n].shape == torch.Size(shape) and dec[n].device.type == device
                assert _bytes(dec[n]) == _scatter(w).tobytes(), (device, n)
    r = runs[case][2]
    for L, shape, w in zip(r["layers"], SHAPES, r["want"]):
        for dev in (None, gpu):
            assert _bytes(decode_layer_tensor(L, device=dev)) == _scatter(w).tobytes(), L.layer_name
        base = torch.randn(*shape, generator=g)
        got = decode_layer_tensor(L, base_tensor=base.to(gpu))
        assert got.is_cuda and _bytes(got) == _scatter(w, base.numpy()).tobytes(), L.layer_name
    start = {n: torch.randn(*s, generator=g) for n, s in zip(NAMES, SHAPES)}
    for kind in ("cuda", "cpu"):
        targets = {n: t.clone().to(kind) for n, t in start.items()}
        decode_updates_into(r["layers"], targets)
        for n, w in zip(NAMES, r["want"]):
            assert _bytes(targets[n]) == _scatter(w, start[n].numpy()).tobytes(), (kind, n)


def _oracle_mean(clients, samples):
    """The PS's sum in fp32, client by client, then one fp32 division by the samples."""
    acc = [np.zeros(n, np.float32) for n in SIZES]
    with np.errstate(all="ignore"):
        for want in clients:
            for a, w in zip(acc, want):
                a[w["idx"]] = (a[w["idx"]] + w["d"]).astype(np.float32)
        return [(a / np.float32(samples)).astype(np.float32) for a in acc]


def test_ps_accumulates_the_oracle_sum(gpu, runs, mixed):
    rounds = runs[CASES[0]]
    clients = [(rounds[0], 3), (rounds[1], 5)]
    want = _oracle_mean([r["want"] for r, _ in clients], 8)
    agg = DeviceAggregator(list(zip(NAMES, SHAPES)), device=gpu)
    for r, ns in clients:
        agg.accumulate_layers(r["layers"], number_samples=ns)
    one = agg.apply()
    agg2 = DeviceAggregator(list(zip(NAMES, SHAPES)), device=gpu)
    agg2.accumulate_many([(r["layers"], ns) for r, ns in clients])
    many = agg2.apply()
    for n, w in zip(NAMES, want):
        assert _bytes(one[n]) == w.tobytes() and _bytes(many[n]) == w.tobytes(), n
    # an update that mixes a fallback layer (fp32 values, an infinity among them) with quantised ones
    r = mixed[1]
    kinds = [L.compression_type for L in r["layers"]]
    assert kinds == [TOPK_QUANT_COMPRESSION_NAME, TOPK_PACKED_COMPRESSION_NAME] + [TOPK_QUANT_COMPRESSION_NAME] * 2
    agg3 = DeviceAggregator(list(zip(NAMES, SHAPES)), device=gpu)
    agg3.accumulate_layers(r["layers"], number_samples=2)
    agg3.accumulate_layers(rounds[2]["layers"], number_samples=2)
    got = agg3.apply()
    for n, w in zip(NAMES, _oracle_mean([r["want"], rounds[2]["want"]], 4)):
        assert _bytes(got[n]) == w.tobytes(), n
    assert torch.isinf(got["t1"]).sum() == 1
    # plain Top-K with either packed type stays refused
    plain = encode_updates_dict({n: t.to(gpu) for n, t in _inputs(0).items()},
                                build_global_compressor(enabled=True, scheme="topk", device=gpu))
    with pytest.raises(ValueError, match="mixed Top-K wires"):
        agg3.accumulate_layers([r["layers"][0], plain[1]], number_samples=1)


def test_fallback_layer_in_a_mixed_message(gpu, mixed):
    _check_layers(mixed, 4, "mixed")
    assert [w["q"] is None for w in mixed[1]["want"]] == [False, True, False, False]
    w = mixed[1]["want"][1]
    assert np.isinf(w["m"]) and np.isnan(w["res"][77])  # inf - inf at the selected slot, the encoder's own store
    # the NaN the encoder left at that slot is selected by every later call: the layer keeps falling back
    assert [x["q"] is None for x in mixed[2]["want"]] == [False, True, False, False] and np.isnan(mixed[2]["want"][1]["m"])
    for device in ("cpu", "cuda"):
        dec = decode_updates_dict(mixed[1]["layers"], device=device)
        for n, x in zip(NAMES, mixed[1]["want"]):
            assert _bytes(dec[n]) == _scatter(x).tobytes(), (device, n)
    targets = {n: torch.ones(*s, device=gpu) for n, s in zip(NAMES, SHAPES)}
    decode_updates_into(mixed[1]["layers"], targets)
    for n, x in zip(NAMES, mixed[1]["want"]):
        assert _bytes(targets[n]) == _scatter(x, np.ones(x["n"], np.float32)).tobytes(), n


def _raw_quant_layer(name, shape, codes, idx_codes, scale, s):
    """A quantised layer whose index codes need not be below n (no encoder writes one)."""
    n = int(np.prod(shape))
    bi = P.index_bits(n)
    L = pb.layer_state(layer_name=name)
    L.compression_type = TOPK_QUANT_COMPRESSION_NAME
    L.values_data = np.packbits(Q.bits_of(np.asarray(codes, np.uint64), s + 2), bitorder="little").tobytes()
    L.indices_data = np.packbits(P._bits_of(np.asarray(idx_codes, np.uint64), bi), bitorder="little").tobytes()
    L.values_dtype, L.indices_dtype = f"packed.q{s + 2}", f"packed.u{bi}"
    L.original_shape.extend(list(shape))
    L.width, L.level = bi, 2**s
    L.meta_tensor, L.meta_tensor_dtype = np.float32([scale]).tobytes(), "torch.float32"
    L.param_shape.append(len(codes))
    return L


def test_index_code_out_of_range_names_its_layer(gpu, runs):
    r = runs[CASES[0]][0]
    bad = _raw_quant_layer("t2", (33,), [1, 30, 16], [5, 40, 0], 2.0, 4)  # b = 6: 40 is a code, not an index
    msg = [L if L.layer_name != "t2" else bad for L in r["layers"]]
    with pytest.raises(IndexError, match="'t2'.*out of bounds for size 33"):
        decode_layer_tensor(bad, device=gpu)
    with pytest.raises(IndexError, match="'t2'.*out of bounds for size 33"):
        decode_updates_dict(msg, device=gpu)
    targets = {n: torch.ones(*s, device=gpu) for n, s in zip(NAMES, SHAPES)}
    with pytest.raises(IndexError, match="'t2'.*out of bounds for size 33"):
        decode_updates_into(msg, targets)
    assert all(bool((t == 1).all()) for t in targets.values())
    agg = DeviceAggregator(list(zip(NAMES, SHAPES)), device=gpu)
    with pytest.raises(IndexError, match="'t2'.*out of bounds for size 33"):
        agg.accumulate_layers(msg, number_samples=1)
    assert not agg.acc.any() and agg.update_count == 0
    # the same layer with its indices in range decodes by the linear rule, every code of the field
    good = _raw_quant_layer("t2", (33,), [0, 32, 16, 63], [5, 32, 0, 7], 2.0, 4)
    want = np.zeros(33, np.float32)
    want[[5, 32, 0, 7]] = Q.dequantize(np.int64([0, 32, 16, 63]) - 16, 2.0, 4)
    assert _bytes(decode_layer_tensor(good, device=gpu)) == want.tobytes()
    assert _bytes(decode_updates_dict([good], device=gpu)["t2"]) == want.tobytes()
    # two levels in one message: decoded layer by layer
    other = _raw_quant_layer("t3", (1,), [3], [0], 4.0, 2)
    dec = decode_updates_dict([good, other], device=gpu)
    assert _bytes(dec["t2"]) == want.tobytes() and dec["t3"].tolist() == [-1.0]
    with pytest.raises(ValueError, match="different levels"):
        DeviceAggregator([("t2", (33,)), ("t3", (1,))], device=gpu).accumulate_layers([good, other], number_samples=1)


def test_value_bits_none_is_the_packed_wire(gpu):
    upd = {n: t.to(gpu) for n, t in _inputs(0).items()}
    a = build_global_compressor(enabled=True, scheme="topk", compress_ratio=0.01, device=gpu, packed_wire=True)
    b = build_global_compressor(enabled=True, scheme="topk", compress_ratio=0.01, device=gpu, packed_wire=True,
                                value_bits=None)
    la, lb = encode_updates_dict(upd, a), encode_updates_dict(upd, b)
    assert [L.SerializeToString() for L in la] == [L.SerializeToString() for L in lb]
    assert all(L.compression_type == TOPK_PACKED_COMPRESSION_NAME and len(L.values_data) % 4 == 0 for L in lb)
    assert b._calls == 0  # no draw was taken


def test_per_layer_path_and_refused_dtypes(gpu):
    """encode_layer_state: one counter step per layer and stream 0 — other, equally valid codes than the batched
    path's; an integer tensor goes through the per-tensor compress; fp16 / bf16 are refused at the sender."""
    ratio, tie, s = 0.25, "index", 3
    comp = _compressor(gpu, ratio, tie, s)
    seed = comp.philox_key()
    res = {}
    for call in range(2):
        upd = _inputs(call)
        layers = [encode_layer_state(n, t.to(gpu), comp) for n, t in upd.items()]
        want = []
        for j, (n, t) in enumerate(upd.items()):
            want += _oracle_call({n: t}, res, ratio, tie, s, seed, call * len(NAMES) + j, stream_of=lambda _t: 0)
        got_res = [comp.residual.residuals[n].cpu().numpy().tobytes() for n in NAMES]
        _check_layers([dict(layers=layers, want=want, res=got_res, stats=wire_size(layers))], s, ("layer", call))
    assert comp._calls == 2 * len(NAMES)
    ints = torch.arange(-500, 500, dtype=torch.int32).reshape(10, 100)
    c2 = _compressor(gpu, ratio, tie, s)
    L = encode_layer_state("i", ints.to(gpu), c2)
    w, = _oracle_call({"i": ints.float()}, {}, ratio, tie, s, c2.philox_key(), 0)
    assert L.compression_type == TOPK_QUANT_COMPRESSION_NAME and L.values_data == Q.pack_codes(w["q"], s)
    assert L.indices_data == P.pack_indices(w["idx"], 1000) and L.meta_tensor == np.float32(500).tobytes()
    assert _bytes(c2.residual.residuals["i"]) == w["res"].tobytes()
    for dt in (torch.float16, torch.bfloat16):
        half = {n: t.to(gpu, dt) for n, t in _inputs(0).items()}
        c3 = _compressor(gpu, ratio, tie, s)
        with pytest.raises(ValueError, match="value_bits quantises fp32"):
            encode_updates_dict(half, c3)
        with pytest.raises(ValueError, match="value_bits quantises fp32"):
            encode_layer_state("t1", half["t1"], c3)
        assert c3._calls == 0 and not c3.residual.residuals


def test_miniature_llama_message_size(gpu):
    """Llama-400M's 183 tensors with every element count divided by 1 024, shapes only (zeros but one element per
    tensor): the value bytes are sum ceil(k_t b / 8), and with 4 bytes of scale per layer and the packed indices
    that is the whole payload."""
    sizes = Q.llama400m_miniature()
    assert len(sizes) == 183 and sizes[:2] == [32_000] * 2 and sizes[-1] == 1
    s, ratio = 4, 0.01
    upd = {}
    for t, n in enumerate(sizes):
        x = torch.zeros(n, device=gpu)
        x[n // 2] = 1.0 + t
        upd[f"p{t}"] = x
    comp = _compressor(gpu, ratio, "index", s)
    stats = {}
    layers = encode_updates_dict(upd, comp, stats=stats)
    ks = [otopk.topk_k(n, ratio) for n in sizes]
    vbytes = sum((k * (s + 2) + 7) // 8 for k in ks)
    ibytes = sum((k * P.index_bits(n) + 7) // 8 for k, n in zip(ks, sizes))
    assert all(L.compression_type == TOPK_QUANT_COMPRESSION_NAME for L in layers)
    assert sum(len(L.values_data) for L in layers) == vbytes
    assert sum(len(L.values_data) + len(L.meta_tensor) for L in layers) == vbytes + 4 * len(sizes)
    assert stats["payload_bytes"] == vbytes + 4 * len(sizes) + ibytes
    assert stats["wire_bytes"] == sum(L.ByteSize() for L in layers) > stats["payload_bytes"]
    dec = decode_updates_dict(layers, device=gpu)
    for t, n in enumerate(sizes):  # the one non-zero element is the scale: it comes back exactly
        assert float(dec[f"p{t}"][n // 2]) == 1.0 + t and int((dec[f"p{t}"] != 0).sum()) == 1
