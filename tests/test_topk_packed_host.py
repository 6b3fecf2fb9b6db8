"""The opt-in bit-packed Top-K index wire without a GPU: the numpy oracle of tests/golden/topk_packed_inputs.py,
the field checks of a received ``TopKBitPackedCompression`` layer, and the host side of the kernels — index_bits,
pack_group / unpack_group and pack_tables_host of omnifed_amd/csrc/omf_topk_layout.{h,cpp} — run by
tests/host/topk_pack_check.cpp under AddressSanitizer and UBSan against vectors the oracle wrote, at every width
b = 1..32 (the device matrix reaches b = 26), with partial last groups, tensors without a value and every bit
past a tensor's k b set.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import topk_packed_inputs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnifed_amd", "csrc")
CHECKER = os.path.join(ROOT, "tests", "host", "topk_pack_check.cpp")


# ------------------------------------------------------------------ the oracle itself

def test_worked_vector():
    """n = 5 (b = 3), indices [4, 0, 3]: 0b011_000_100 little-endian, 9 bits in 2 bytes."""
    from omnifed_amd import codec

    assert P.index_bits(5) == codec.topk_index_bits(5) == 3
    assert P.pack_indices([4, 0, 3], 5) == b"\xc4\x00"
    assert P.unpack_indices(b"\xc4\x00", 3, 5).tolist() == [4, 0, 3]
    assert P.unpack_indices(b"\xc4\xfe", 3, 5).tolist() == [4, 0, 3]  # the unused high bits are ignored


def test_index_bits_rule():
    """The oracle's rule at its edges, and the product's two statements of it (Python, and the C ABI's
    host-only omf_topk_index_bits) equal to the oracle's."""
    from omnifed_amd import _lib, codec

    assert [P.index_bits(n) for n in (1, 2, 3, 4, 5)] == [1, 1, 2, 2, 3]
    for j in range(1, 33):
        assert P.index_bits(2**j) == j, j
        if j < 32:
            assert P.index_bits(2**j + 1) == j + 1, j
    L = _lib.lib()
    for n in [1, 2, 3, 4, 5] + [2**j for j in range(1, 33)] + [2**j + 1 for j in range(1, 32)]:
        assert codec.topk_index_bits(n) == L.omf_topk_index_bits(n) == P.index_bits(n), n
    for n in (0, -1, 2**32 + 1):
        with pytest.raises(ValueError):
            P.index_bits(n)
        with pytest.raises(ValueError):
            codec.topk_index_bits(n)
        assert L.omf_topk_index_bits(n) == -1


@pytest.mark.parametrize("b", range(1, 33))
def test_oracle_round_trip(b):
    from omnifed_amd import codec

    rng = np.random.default_rng(100 + b)
    n = P.size_of_width(b, rng)
    assert P.index_bits(n) == codec.topk_index_bits(n) == b
    for k in (1, 2, 31, 32, 33, 100):
        idx = P.draw_indices([n], [min(k, n)], seed=b * 1000 + k)
        k = idx.size
        data = P.pack_indices(idx, n)
        assert len(data) == (k * b + 7) // 8
        assert (P.unpack_indices(data, k, n) == idx).all()
        # against a bit-by-bit restatement of the format
        want = bytearray(len(data))
        for i, v in enumerate(idx.tolist()):
            for j in range(b):
                if (v >> j) & 1:
                    want[(i * b + j) // 8] |= 1 << ((i * b + j) % 8)
        assert data == bytes(want)
        # the arena form: the same stream, zero-padded to whole groups
        words = P.pack_arena([n], [k], idx)
        assert words.size == -(-k // 32) * b
        assert words.view(np.uint8)[:len(data)].tobytes() == data and not words.view(np.uint8)[len(data):].any()
        dirty = P.pack_arena([n], [k], idx, pad_ones=True)
        assert (P.unpack_arena([n], [k], dirty) == idx).all()
        assert k * b % 32 == 0 or dirty[-1] >> (k * b % 32) == 2**(32 - k * b % 32) - 1


def test_arena_layout_rule():
    sizes, counts = [5, 1, 70000, 33, 2**32], [3, 0, 700, 33, 65]
    from omnifed_amd import codec

    lay = P.arena_layout(sizes, counts)
    assert lay.bits == [codec.topk_index_bits(n) for n in sizes] == [3, 1, 17, 6, 32]
    assert lay.goff == [0, 1, 1, 23, 25, 28]
    assert lay.woff == [0, 3, 3, 3 + 22 * 17, 3 + 22 * 17 + 12, 3 + 22 * 17 + 12 + 96]
    assert lay.words == lay.woff[-1]


# ------------------------------------------------------------------ a received layer's fields

def _layer(n=5, idx=(4, 0, 3), **over):
    from omnifed_amd.hybrid.communicator import global_grpc_pb2 as pb

    b = P.index_bits(n)
    L = pb.layer_state(layer_name="w")
    L.compression_type = "TopKBitPackedCompression"
    L.values_data = np.arange(1, len(idx) + 1, dtype=np.float32).tobytes()
    L.indices_data = P.pack_indices(idx, n)
    L.values_dtype = "torch.float32"
    L.indices_dtype = f"packed.u{b}"
    L.original_shape.extend([n])
    L.width = b
    for k, v in over.items():
        setattr(L, k, v)
    return L


def test_names_are_exported():
    from omnifed_amd.hybrid.compression import TOPK_COMPRESSION_NAME, TOPK_PACKED_COMPRESSION_NAME

    assert TOPK_COMPRESSION_NAME == "TopKCompression" and TOPK_PACKED_COMPRESSION_NAME == "TopKBitPackedCompression"


def test_layer_builder_and_reader():
    from omnifed_amd.hybrid.communicator import global_grpc_compression as G

    vals = np.float32([1.5, -2.0, 3.0]).tobytes()
    L = G.topk_packed_layer_from_bytes("w", (5,), vals, b"\xc4\x00")
    assert (L.compression_type, L.indices_dtype, L.width, L.values_dtype) == (
        "TopKBitPackedCompression", "packed.u3", 3, "torch.float32")
    assert L.indices_data == b"\xc4\x00" and L.values_data == vals and list(L.original_shape) == [5]
    assert G.read_topk_layer(L) == (vals, b"\xc4\x00", 3)
    assert G._validate_layer(L) == (vals, b"\xc4\x00", 3)
    assert G.wire_size([L])["payload_bytes"] == 12 + 2
    with pytest.raises(ValueError):
        G.topk_packed_layer_from_bytes("w", (2**32 + 1,), vals, b"\x00" * 13)


@pytest.mark.parametrize("over, msg", [
    (dict(values_data=b""), "missing values/indices"),
    (dict(indices_data=b""), "missing values/indices"),
    (dict(values_data=b"\x00" * 13), "multiple of element size"),
    (dict(width=4), "unsupported width=4"),
    (dict(width=0), "unsupported width=0"),
    (dict(indices_dtype="packed.u4"), "unsupported indices_dtype='packed.u4'"),
    (dict(indices_dtype="torch.int64"), "unsupported indices_dtype='torch.int64'"),
    (dict(indices_data=b"\xc4"), "1 index bytes, expected 2"),
    (dict(indices_data=b"\xc4\x00\x00"), "3 index bytes, expected 2"),
])
def test_field_errors(over, msg):
    from omnifed_amd.hybrid.communicator import global_grpc_compression as G

    L = _layer(**over)
    for fn in (G.read_topk_layer, G._validate_layer, G.decode_layer_tensor, lambda x: G.decode_updates_dict([x])):
        with pytest.raises(ValueError, match="Compressed layer 'w'.*" + msg):
            fn(L)


def test_shape_outside_the_width_rule():
    from omnifed_amd.hybrid.communicator import global_grpc_compression as G

    L = _layer()
    del L.original_shape[:]
    L.original_shape.extend([0])
    with pytest.raises(ValueError, match="Compressed layer 'w'.*1 to 2\\^32 elements"):
        G.read_topk_layer(L)


def test_packed_wire_option_reaches_topk():
    from omnifed_amd.hybrid.communicator import global_grpc_compression as G
    from omnifed_amd.hybrid.compression import TopKCompression

    assert TopKCompression().packed_wire is False
    c = G.build_global_compressor(enabled=True, scheme="topk", compress_ratio=0.02, packed_wire=True)
    assert isinstance(c, TopKCompression) and c.packed_wire is True and c.compress_ratio == 0.02
    assert G.build_global_compressor(enabled=True, scheme="topk").packed_wire is False
    cfg = {"engine": {"hybrid": {"global_compression": {"enabled": True, "scheme": "topk", "packed_wire": True}}}}
    assert G.hybrid_global_compressor_from_cfg(cfg).packed_wire is True


# ------------------------------------------------------------------ the shared host routines, sanitized

def _arena_record(sizes, counts, seed):
    lay = P.arena_layout(sizes, counts)
    idx = P.draw_indices(sizes, counts, seed)
    sent = P.pack_arena(sizes, counts, idx)
    dirty = P.pack_arena(sizes, counts, idx, pad_ones=True)
    assert (P.unpack_arena(sizes, counts, dirty) == idx).all()
    cells = [len(sizes)] + [x for nk in zip(sizes, counts) for x in nk] + lay.bits + lay.goff + lay.woff
    cells += [lay.words] + idx.tolist() + sent.tolist() + dirty.tolist()
    return "A " + " ".join(str(int(c)) for c in cells)


def vector_lines():
    lines = []
    for n in [1, 2, 3, 4, 5] + [2**j for j in range(1, 33)] + [2**j + 1 for j in range(1, 32)]:
        lines.append(f"B {n} {P.index_bits(n)}")
    for n in (0, -5, 2**32 + 1, 2**40):
        lines.append(f"B {n} -1")
    rng = np.random.default_rng(7)
    # every width, one tensor: whole groups, partial last groups, one index
    for b in range(1, 33):
        n = P.size_of_width(b, rng)
        for k in sorted({1, min(n, 31), min(n, 32), min(n, 33), min(n, 97)}):
            lines.append(_arena_record([n], [k], seed=b * 100 + k))
    # several tensors of every width at once: tensors without a value at the start, inside and at the end
    sizes = [P.size_of_width(b, rng) for b in range(1, 33)]
    for v in range(4):
        counts = [int(rng.choice([0, 1, min(n, 31), min(n, 32), min(n, 33), min(n, 65)])) for n in sizes]
        if v == 0:
            counts[0] = counts[5] = counts[-1] = 0
        if v == 1:
            counts = [0] * len(sizes)
        lines.append(_arena_record(sizes, counts, seed=9000 + v))
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_routines_under_sanitizers(tmp_path):
    exe = str(tmp_path / "topk_pack_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(CSRC, "omf_topk_layout.cpp"),
                    os.path.join(CSRC, "omf_plan_layout.cpp"), CHECKER], check=True)
    lines = vector_lines()
    table = tmp_path / "vectors.txt"
    table.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(table)], check=False, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1].split()
    n_bits = sum(line.startswith("B") for line in lines)
    assert last[0] == "0" and int(last[2]) == n_bits and int(last[5]) == len(lines) - n_bits, out.stdout
    assert int(last[7]) == 32, out.stdout  # groups of every width b = 1..32 were packed and unpacked
