"""The opt-in quantised Top-K value wire without a GPU: the numpy oracle of tests/golden/topk_qval_inputs.py (the
worked vector, the layout, the error bound, the maximum decoding to the scale), the field checks of a received
``TopKQuantPackedCompression`` layer, the ``value_bits`` argument rules, and the host side of the kernels — the
value-word layout rule and the group pack / unpack of omnifed_amd/csrc/omf_topk_layout.{h,cpp} at every code
width b = 3..10 — run by tests/host/topk_qval_check.cpp under AddressSanitizer and UBSan against vectors the
oracle wrote.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import topk_qval_inputs as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnifed_amd", "csrc")
CHECKER = os.path.join(ROOT, "tests", "host", "topk_qval_check.cpp")


# ------------------------------------------------------------------ the oracle itself

def test_worked_vector():
    """s = 2 (L = 4, b = 4), v = [3, -1.5, 0.75]: m = 3, q = [4, -2, 1], codes [8, 2, 5] -> b"\\x28\\x05"."""
    from omnifed_amd import codec

    W = Q.WORKED
    assert Q.code_bits(W["s"]) == codec.topk_value_bits(W["s"]) == codec.packed_bits(2**W["s"]) == 4
    for seed in (0, 1, 2**63 + 5):  # whole levels: no draw matters
        m, q, d, e = Q.quantize(W["v"], W["s"], seed, 3, 0)
        assert float(m) == W["m"] and q.tolist() == W["q"] and d.tolist() == W["d"] and not e.any()
    assert Q.pack_codes(W["q"], W["s"]) == W["data"]
    assert Q.unpack_codes(W["data"], 3, W["s"]).tolist() == W["q"]
    assert Q.unpack_codes(b"\x28\xf5", 3, W["s"]).tolist() == W["q"]  # the unused high bits are ignored
    # bit by bit: value i at bits [4 i, 4 i + 4), LSB first
    want = bytearray(2)
    for i, c in enumerate([8, 2, 5]):
        for j in range(4):
            if (c >> j) & 1:
                want[(4 * i + j) // 8] |= 1 << ((4 * i + j) % 8)
    assert bytes(want) == W["data"]


@pytest.mark.parametrize("s", range(1, 9))
def test_error_bound_and_exact_maximum(s):
    """|v - d| <= m / L everywhere (a level is at most one step off), the maximum decodes to exactly m with its
    sign, +-0 decode to 0, and the error is what the residual gets."""
    from omnifed_amd import codec

    L = 2**s
    assert codec.topk_value_bits(s) == Q.code_bits(s)
    for t, v in enumerate(Q.matrix_values()):
        m, q, d, e = Q.quantize(v, s, 77, 5, t)
        if t in Q.UNUSABLE:
            assert q is None and not Q.usable(m, s) and not codec.topk_scale_usable(float(m), s)
            continue
        assert Q.usable(m, s) and codec.topk_scale_usable(float(m), s) and q.size == v.size
        if v.size == 0:
            continue
        assert np.abs(q).max() <= L
        step = np.float64(m) / L
        assert (np.abs(v.astype(np.float64) - d.astype(np.float64)) <= step * (1 + 2**-20)).all(), t
        if m > 0:
            top = np.abs(v) == m
            assert top.any() and (d[top] == v[top]).all() and (np.abs(q[top]) == L).all()
        assert not d[v == 0].any()
        assert (e == (v - d).astype(np.float32)).all()
        data = Q.pack_codes(q, s)
        assert len(data) == (v.size * (s + 2) + 7) // 8
        assert (Q.unpack_codes(data, v.size, s) == q).all()


def test_scale_rule():
    assert Q.scale_of([]) == 0 and Q.scale_of([0.0, -0.0]) == 0 and not np.signbit(Q.scale_of([-0.0]))
    assert Q.scale_of([1.0, -3.5, 2.0]) == 3.5
    assert np.isnan(Q.scale_of([1.0, np.nan, np.inf])) and np.isinf(Q.scale_of([1.0, -np.inf]))
    from omnifed_amd import codec

    for s in range(1, 9):
        edge = np.float32(Q.FLT_MAX / 2**s)
        over = np.nextafter(edge, np.float32(np.inf))
        for m, ok in ((0.0, True), (1e-45, True), (edge, True), (over, False), (np.inf, False), (np.nan, False),
                      (-1.0, False)):
            assert Q.usable(m, s) == codec.topk_scale_usable(float(m), s) == ok, (s, m)
        with np.errstate(over="ignore"):
            assert np.isfinite(edge * np.float32(2**s)) and np.isinf(over * np.float32(2**s))


def test_draws_are_the_selection_positions():
    """Tensor t's draws are philox_uniforms(seed, offset, t, k): another t, offset or seed moves the codes of
    values between levels, and a prefix of the selection has the prefix's codes."""
    from omnifed_amd.hybrid.compression import TopKCompression

    rng = np.random.default_rng(1)
    v = rng.standard_normal(5000).astype(np.float32)
    m = Q.scale_of(v)
    comp = TopKCompression(packed_wire=True, value_bits=3)  # a compressor's key and counter are such a (seed, offset)
    assert 0 <= comp.philox_key() < 2**64 and comp._calls == 0
    base = Q.quantize(v, 3, 9, 4, 2)[1]
    assert (Q.quantize(v, 3, 9, 4, 3)[1] != base).any() and (Q.quantize(v, 3, 9, 5, 2)[1] != base).any()
    assert (Q.quantize(v, 3, 10, 4, 2)[1] != base).any()
    assert (Q.quantize(v[:1234], 3, 9, 4, 2, m=m)[1] == base[:1234]).all()


def test_arena_layout_rule():
    from omnifed_amd import codec

    counts = [3, 0, 700, 33, 65]
    assert Q.group_offsets(counts) == [0, 1, 1, 23, 25, 28]
    for s in range(1, 9):
        b = codec.topk_value_bits(s)
        assert b == s + 2
        codes = [np.arange(k, dtype=np.uint64) % (2**(s + 1) + 1) for k in counts]
        words = Q.value_arena(counts, codes, s)
        assert words.size == 28 * b
        for t, k in enumerate(counts):
            off, n = Q.stream_bytes(counts, t, s)
            assert (off, n) == (4 * b * Q.group_offsets(counts)[t], (k * b + 7) // 8)
            got = Q.unpack_codes(words.view(np.uint8)[off:off + n].tobytes(), k, s) + 2**s
            assert (got == codes[t].astype(np.int64)).all()
        dirty = Q.value_arena(counts, codes, s, pad_ones=True)
        assert (dirty != words).any() and ((dirty & words) == words).all()


def test_llama400m_value_bytes():
    """The issue's table: one Llama-400M update at 1 % with s = 4 (6-bit codes), from the shapes."""
    from omnifed_amd import codec
    from oracle.topk import topk_k

    sizes = Q.llama400m_miniature(div=1)
    ks = [topk_k(n, 0.01) for n in sizes]
    assert sorted(set(ks)) == [10, 10_485, 41_943, 327_680] and 4 * sum(ks) == 16_044_600
    b = codec.topk_value_bits(4)
    rows = {k: sum((kk * b + 7) // 8 for kk in ks if kk == k) for k in set(ks)}
    assert rows == {327_680: 491_520, 10_485: 629_120, 41_943: 1_887_480, 10: 328}
    assert sum(rows.values()) == 3_008_448


# ------------------------------------------------------------------ a received layer's fields

def _layer(n=5, idx=(4, 0, 3), s=2, q=(4, -2, 1), scale=3.0, **over):
    import topk_packed_inputs as P
    from omnifed_amd.hybrid.communicator import global_grpc_pb2 as pb

    bi = P.index_bits(n)
    L = pb.layer_state(layer_name="w")
    L.compression_type = "TopKQuantPackedCompression"
    L.values_data = Q.pack_codes(q, s)
    L.indices_data = P.pack_indices(idx, n)
    L.values_dtype = f"packed.q{s + 2}"
    L.indices_dtype = f"packed.u{bi}"
    L.original_shape.extend([n])
    L.width = bi
    L.level = 2**s
    L.meta_tensor = np.float32([scale]).tobytes()
    L.meta_tensor_dtype = "torch.float32"
    L.param_shape.extend(over.pop("param_shape", [len(q)]))
    for k, v in over.items():
        setattr(L, k, v)
    return L


def test_names_are_exported():
    from omnifed_amd.hybrid.compression import TOPK_QUANT_COMPRESSION_NAME

    assert TOPK_QUANT_COMPRESSION_NAME == "TopKQuantPackedCompression"


def test_layer_builder_and_reader():
    from omnifed_amd.hybrid.communicator import global_grpc_compression as G

    L = G.topk_quant_layer_from_bytes("w", (5,), 3, b"\x28\x05", b"\xc4\x00", 3.0, 2)
    assert L == _layer()
    assert (L.compression_type, L.values_dtype, L.indices_dtype, L.width, L.level, list(L.param_shape)) == (
        "TopKQuantPackedCompression", "packed.q4", "packed.u3", 3, 4, [3])
    assert L.meta_tensor == np.float32([3.0]).tobytes() and L.meta_tensor_dtype == "torch.float32"
    for fn in (G.read_topk_layer, G._validate_layer):
        v, i, k = fn(L)
        assert isinstance(v, G.QuantValues) and (v.codes, v.k, v.scale, v.bits) == (b"\x28\x05", 3, 3.0, 2)
        assert (i, k) == (b"\xc4\x00", 3)
    assert G.wire_size([L])["payload_bytes"] == 2 + 2 + 4
    assert G.wire_size([L])["wire_bytes"] == L.ByteSize()
    G.read_topk_layer(_layer(scale=0.0, q=(0, 0, 0)))  # a zero scale is a scale


@pytest.mark.parametrize("over, msg", [
    (dict(values_data=b""), "missing values/indices"),
    (dict(indices_data=b""), "missing values/indices"),
    (dict(level=0), "invalid level=0"),
    (dict(level=1), "invalid level=1"),
    (dict(level=6), "invalid level=6"),
    (dict(level=512), "invalid level=512"),
    (dict(level=8), "unsupported values_dtype='packed.q4'"),
    (dict(values_dtype="packed.q5"), "unsupported values_dtype='packed.q5'"),
    (dict(values_dtype="torch.float32"), "unsupported values_dtype='torch.float32'"),
    (dict(param_shape=[]), "param_shape must hold the value count"),
    (dict(param_shape=[3, 1]), "param_shape must hold the value count"),
    (dict(param_shape=[6]), "6 values for 5 elements"),
    (dict(values_data=b"\x28"), "1 value bytes, expected 2"),
    (dict(values_data=b"\x28\x05\x00"), "3 value bytes, expected 2"),
    (dict(param_shape=[2]), "2 value bytes, expected 1"),
    (dict(indices_data=b"\xc4"), "1 index bytes, expected 2"),
    (dict(indices_data=b"\xc4\x00\x00"), "3 index bytes, expected 2"),
    (dict(width=4), "unsupported width=4"),
    (dict(indices_dtype="torch.int64"), "unsupported indices_dtype='torch.int64'"),
    (dict(meta_tensor=b""), "meta_tensor .* must be one float32, not 0 bytes"),
    (dict(meta_tensor=b"\x00" * 8), "meta_tensor .* must be one float32, not 8 bytes"),
    (dict(scale=-1.0), "invalid scale=-1.0"),
    (dict(scale=-0.0), "invalid scale=-0.0"),
    (dict(scale=float("inf")), "invalid scale=inf"),
    (dict(scale=float("nan")), "invalid scale=nan"),
])
def test_field_errors(over, msg):
    from omnifed_amd.hybrid.communicator import global_grpc_compression as G

    L = _layer(**over)
    for fn in (G.read_topk_layer, G._validate_layer, G.decode_layer_tensor, lambda x: G.decode_updates_dict([x])):
        with pytest.raises(ValueError, match="Compressed layer 'w'.*" + msg):
            fn(L)


# ------------------------------------------------------------------ the value_bits argument

def test_value_bits_rules():
    from omnifed_amd.hybrid.communicator import global_grpc_compression as G
    from omnifed_amd.hybrid.compression import TopKCompression

    assert TopKCompression().value_bits is None and TopKCompression(packed_wire=True).value_bits is None
    assert G.build_global_compressor(enabled=True, scheme="topk", packed_wire=True).value_bits is None
    for s in range(1, 9):
        assert TopKCompression(packed_wire=True, value_bits=s).value_bits == s
    c = G.build_global_compressor(enabled=True, scheme="topk", compress_ratio=0.02, packed_wire=True, value_bits=4)
    assert isinstance(c, TopKCompression) and (c.packed_wire, c.value_bits, c.compress_ratio) == (True, 4, 0.02)
    with pytest.raises(ValueError, match="requires packed_wire=True"):
        TopKCompression(value_bits=4)
    with pytest.raises(ValueError, match="requires packed_wire=True"):
        G.build_global_compressor(enabled=True, scheme="topk", value_bits=4)
    with pytest.raises(ValueError, match="requires scheme='topk'"):
        G.build_global_compressor(enabled=True, scheme="qsgd", packed_wire=True, value_bits=4)
    for bad in (0, 9, -1, 2.5, True, "4"):
        with pytest.raises((ValueError, TypeError)):
            TopKCompression(packed_wire=True, value_bits=bad)
    assert G.build_global_compressor(enabled=False, scheme="topk", value_bits=4) is None
    gc = {"enabled": True, "scheme": "topk", "packed_wire": True, "value_bits": 6}
    got = G.hybrid_global_compressor_from_cfg({"engine": {"hybrid": {"global_compression": gc}}})
    assert (got.packed_wire, got.value_bits) == (True, 6)
    del gc["value_bits"]
    assert G.hybrid_global_compressor_from_cfg({"engine": {"hybrid": {"global_compression": gc}}}).value_bits is None


def test_key_and_call_counter():
    """QSGDQuantCompression.philox_key's derivation, and a counter that starts at 0."""
    import torch

    from omnifed_amd.hybrid.compression import TopKCompression
    from omnifed_amd.hybrid.compression.qsgd import philox_key

    torch.manual_seed(1234)
    a, b = TopKCompression(packed_wire=True, value_bits=4), TopKCompression(packed_wire=True, value_bits=4)
    a.client_id, b.client_id = 3, 3
    assert a.philox_key() == philox_key(a._instance, 3) and a.philox_key() != b.philox_key()
    b.client_id = 4
    assert b.philox_key() == philox_key(b._instance, 4)
    assert (a._calls, a._next_call(), a._next_call(), a._calls) == (0, 0, 1, 2)


# ------------------------------------------------------------------ the shared host routines, sanitized

def _arena_record(sizes, counts, s, seed):
    rng = np.random.default_rng(seed)
    L = 2**s
    codes = [rng.integers(0, 2 * L + 1, k).astype(np.uint64) for k in counts]
    for c in codes:
        if c.size:
            c[0], c[-1] = 2 * L, 0 if c.size > 1 else 2 * L
    sent = Q.value_arena(counts, codes, s)
    dirty = Q.value_arena(counts, codes, s, pad_ones=True)
    assert sent.size == Q.group_offsets(counts)[-1] * (s + 2)
    cells = [len(sizes)] + [x for nk in zip(sizes, counts) for x in nk] + [s, sent.size]
    cells += np.concatenate(codes).tolist() if sum(counts) else []
    cells += sent.tolist() + dirty.tolist()
    return "V " + " ".join(str(int(c)) for c in cells)


def vector_lines():
    lines = [f"S {s} {s + 2}" for s in range(1, 9)] + [f"S {s} -1" for s in (0, 9, -3, 32)]
    for s in range(1, 9):
        for k in (1, 31, 32, 33, 97):
            lines.append(_arena_record([100], [k], s, seed=100 * s + k))
        sizes = [7, 1, 40, 32, 100, 5000, 300, 64]
        lines.append(_arena_record(sizes, [0, 1, 31, 32, 33, 4097, 0, 64], s, seed=900 + s))
        lines.append(_arena_record(sizes, [0] * len(sizes), s, seed=950 + s))
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_routines_under_sanitizers(tmp_path):
    exe = str(tmp_path / "topk_qval_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(CSRC, "omf_topk_layout.cpp"),
                    os.path.join(CSRC, "omf_plan_layout.cpp"), CHECKER], check=True)
    lines = vector_lines()
    table = tmp_path / "vectors.txt"
    table.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(table)], check=False, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1].split()
    n_bits = sum(line.startswith("S") for line in lines)
    assert last[0] == "0" and int(last[2]) == n_bits and int(last[5]) == len(lines) - n_bits, out.stdout
    assert int(last[7]) == 8, out.stdout  # groups of every code width b = 3..10 were packed and unpacked
